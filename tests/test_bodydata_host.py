"""xrnerf_amd/bodydata.py without a GPU: the registries and reprs, the dataset's selection logic on a generated ZJU-shaped directory, the
transforms on their own (numpy on the host) against tests/golden/ref_bodydata.npz, the host restatements of the prepared picture and the
box silhouette, the planner, and the agreement of the header, the ctypes table and the build recipe."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import bodydata_cases as K  # noqa: E402
import bodydata_restatement as RS  # noqa: E402
from xrnerf_amd import bodydata, pipelines  # noqa: E402

CPU = torch.device('cpu')
REF_CONFIGS = '/root/reference/configs'


def test_registries_reprs_and_planner():
    K.check_plans()


def _reduced(data):
    """a config's data dict with what a test must vary taken out: the callables, the directory, the sizes"""
    out = {}
    for split in ('train', 'val', 'test'):
        d = data[split]
        cfg = {k: v for k, v in d['cfg'].items() if not callable(v)}
        out[split] = (d['type'], sorted(cfg), [(s['type'], s.get('enable', True), s.get('sel_all', False), sorted(s.get('keys', []))) for s in d['pipeline']])
    return out


@pytest.mark.parametrize('path,dataset,lists', [('neuralbody/nb_zjumocap_313.py', 'NeuralBodyDataset', 'nb_lists'),
                                                ('animatable_nerf/an_h36m_s9_novel_pose.py', 'AniNeRFDataset', 'ani_lists')])
def test_the_data_dicts_are_the_reference_configs_reduced(path, dataset, lists):
    p = os.path.join(REF_CONFIGS, path)
    if not os.path.exists(p):
        return                                                # (the comparison needs the reference tree; the lists are used either way)
    import runpy
    ref = _reduced(runpy.run_path(p)['data'])
    tr, te = getattr(K, lists)(1024)
    mine = {}
    for split, steps in (('train', tr), ('val', te), ('test', te)):
        mine[split] = (dataset, None, [(s['type'], s.get('enable', True), s.get('sel_all', False), sorted(s.get('keys', []))) for s in steps])
    for split in ref:
        assert ref[split][0] == mine[split][0] and ref[split][0] in pipelines.DATASETS
        assert [s[0] for s in ref[split][2]] == [s[0] for s in mine[split][2]], split
        assert [s[2] for s in ref[split][2]] == [s[2] for s in mine[split][2]], split
        for a, b in zip(ref[split][2], mine[split][2]):
            if a[0] == 'DeleteUseless':
                assert a[3] == b[3], (split, a, b)
        needed = set(ref[split][1]) - {'num_train_frame', 'num_train_pose', 'num_novel_pose', 'novel_pose_frame', 'phase', 'frame_idx'}
        assert needed <= set(K.base_cfg('x')), needed - set(K.base_cfg('x'))


def test_header_table_and_build_recipe_agree():
    K.check_symbols(loaded=False)


def test_transforms_on_their_own_are_the_fixture():
    K.check_host_path()


def test_get_rigid_transformation_and_rodrigues():
    g = K.gold()
    A, joints = bodydata.get_rigid_transformation(g['skel.poses'], g['skel.joints'], g['skel.parents'], return_joints=True)
    K.same_bits(A, g['skel.A'], 'get_rigid_transformation')
    assert A.dtype == np.float32 and joints.shape == (24, 3)
    for rvec in ([0.3, -0.2, 0.9], [0, 0, 0], [np.pi / 2, 0, 0]):
        R = bodydata.rodrigues(np.array([rvec]))
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
    assert np.abs(bodydata.rodrigues([np.pi / 2, 0, 0]) - np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]])).max() < 1e-15


def test_host_prepare_against_the_specification():
    K.check_host_prepare()


def test_host_fill_is_the_specification_and_keeps_the_quirk():
    for name in K.SCENES:
        s = K.scene(name)
        c = K.corners(s)
        K.same_bits(bodydata.bound_mask(c, s['H'], s['W']), RS.fill(c, s['H'], s['W']), name)
    # the list that closes on 5, alone: the triangle 5 7 6 plus the segment 4 5, not the quadrilateral
    c = np.zeros((8, 2), int)
    c[4], c[5], c[7], c[6] = (1, 1), (9, 1), (9, 9), (1, 9)
    quirk = RS.fill_one(c[[4, 5, 7, 6, 5]], 11, 11)
    assert quirk[1, 1:10].all() and quirk[5, 5] and quirk[8, 3] and not quirk[3, 2] and not quirk[5, 1]
    assert RS.fill_one(c[[4, 5, 7, 6, 4]], 11, 11)[3, 2]


def test_corner_behind_the_camera_raises():
    s = K.scene('oblique')
    with pytest.raises(ValueError):
        bodydata.box_corners_2d(s['bounds'], s['K'], np.concatenate([s['R'], s['T'] - np.array([[0], [0], [2.2]])], axis=1))
    with pytest.raises(NotImplementedError, match='0.3'):
        bodydata.host_prepare(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8), s['K'], np.zeros(5), 0.3, False)


def test_dataset_selection_and_items_on_the_host(tmp_path):
    ds = K.check_dataset(CPU, str(tmp_path))
    assert not ds['train'].store.native and ds['train'].store.prepared == 0
