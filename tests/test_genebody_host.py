"""GeneBody data without a GPU and without the kernels: tests/genebody_restatement.py (the specification of the frame preparation)
against the items the reference's own GeneBodyDataset produced (tests/golden/ref_genebody.npz, tests/golden/make_golden_genebody.py), the
.obj / .ply loaders, the index arithmetic and the inputs that are refused."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import genebody_cases as K  # noqa: E402
import genebody_restatement as RS  # noqa: E402
from xrnerf_amd import genebody  # noqa: E402


def test_fixture_still_holds_every_case_it_was_made_for():
    K.coverage()


@pytest.mark.parametrize('name', sorted(K.ITEMS))
def test_restatement_equals_the_recorded_reference_items(name):
    g = K.gold()
    spec = K.spec_item(name)
    p = 'item.%s.' % name
    K.same_bits(np.stack(spec['img']), np.concatenate([g[p + 'img'], g[p + 'render_gt'].reshape((-1,) + g[p + 'img'].shape[1:])]), 'img and render_gt')
    K.same_bits(np.stack(spec['mask']), g[p + 'mask'], 'mask')
    K.same_bits(np.stack(spec['depth']), g[p + 'smpl_depth'], 'smpl_depth')
    K.same_bits(spec['bbox'], g[p + 'bbox'], 'bbox')
    K.same_bits(spec['center'], g[p + 'center'], 'center')
    s, f, vids, S, white, is_train = K.item_views(name)
    K.same_bits(np.stack([np.linalg.inv(np.array(g['tree.%s.c2w' % s][v], dtype=np.float32)) for v in vids]), g[p + 'calib'], 'calib')
    want, got = g[p + 'persps'], np.stack(spec['persps'])
    nd = want.shape[1] - 6
    K.same_bits(got[:, :4 + nd].astype(np.float32), want[:, :4 + nd], 'K entries and D')
    for i in range(len(vids)):
        for j in (4 + nd, 5 + nd):
            assert abs(float(want[i, j]) - got[i, j]) <= spec['near_bound'][i], (i, j, float(want[i, j]), got[i, j], spec['near_bound'][i])
    assert min(spec['rel']) >= 0.25
    assert abs(min(spec['sf']) / float(g[p + 'spatial_freq']) - 1) <= 1e-5
    assert int(g[p + 'idx']) == ITEM_INDEX(name)


def ITEM_INDEX(name):
    phase, S, white, skip, index, rnd = K.ITEMS[name]
    return index if phase == 'train' else index * skip


def test_cubic_resize_identity_upscale_and_coefficients():
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (16, 16, 3)).astype(np.uint8)
    assert np.array_equal(RS.resize_cubic_u8(src, 16), src)                         # f = 0: coefficients 0, 2048, 0, 0
    idx, coef = RS.cubic_taps(7, 16)
    assert (np.abs(coef.sum(axis=1) - 2048) <= 2).all()                          # each coefficient is rounded on its own
    assert idx.min() == 0 and idx.max() == 6 and (idx[0] == [0, 0, 0, 1]).all()
    flat = np.full((7, 9, 3), 201, np.uint8)
    assert (RS.resize_cubic_u8(flat, 16) == 201).all()
    assert RS.nearest_index(37, 16).tolist() == [int(np.floor(x * 37 / 16)) for x in range(16)]


def test_loaders_match_the_reference_arrays(tmp_path):
    g = K.gold()
    K.write_tree(str(tmp_path))
    v, f = genebody.load_obj_mesh(str(tmp_path / 'data' / 'dannier' / 'smpl' / '0001.obj'))
    assert v.dtype == np.float64 and f.dtype == np.int64
    K.same_bits(v.astype(np.float32), g['item.val0.smpl_verts'], '.obj vertices')
    K.same_bits(f.astype(np.int32), g['item.val0.smpl_faces'], '.obj faces (quad split, 1-based)')
    assert f[:2].tolist() == [[0, 1, 2], [2, 3, 0]]
    v, f = genebody.load_ply(str(tmp_path / 'data' / 'amanda' / 'smpl' / '0005.ply'))
    K.same_bits(v.astype(np.float32), g['item.val2.smpl_verts'], 'binary little-endian .ply vertices')
    K.same_bits(f.astype(np.int32), g['item.val2.smpl_faces'], 'binary little-endian .ply faces')
    for form in ('ascii', 'binary_big_endian'):
        K.write_ply(str(tmp_path / 'x.ply'), g['tree.amanda.0005.verts'], g['tree.amanda.0005.faces'], form)
        v2, f2 = genebody.load_ply(str(tmp_path / 'x.ply'))
        K.same_bits(v2, v, form + ' vertices')
        K.same_bits(f2.astype(np.int32), f.astype(np.int32), form + ' faces')
    tv, tf = genebody.load_obj_mesh(str(tmp_path / 't_pose' / 'smplx.obj'))
    K.same_bits(tv.astype(np.float32), g['item.val0.smpl_t_verts'], 'T-pose vertices')
    K.same_bits(tf.astype(np.int32), g['item.val0.smpl_t_faces'], 'T-pose faces')


def test_rodrigues_is_the_documented_formula_in_double():
    from xrnerf_amd.bodydata import rodrigues
    g = K.gold()
    r = g['tree.dannier.0001.orient'].astype(np.float64).reshape(3)
    t = np.linalg.norm(r)
    k = r / t
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    want = np.cos(t) * np.eye(3) + (1 - np.cos(t)) * np.outer(k, k) + np.sin(t) * kx
    assert np.abs(rodrigues(r) - want).max() <= 4 * 2.0 ** -52
    K.same_bits(rodrigues(r).astype(np.float32), g['item.val0.smpl_rot'], 'smpl_rot')


def test_lengths_and_index_arithmetic(tmp_path):
    K.check_lengths(str(tmp_path))
    g = K.gold()
    for name, (phase, S, white, skip, index, rnd) in K.ITEMS.items():
        ds, _ = K.build(str(tmp_path), name, 'cpu')
        assert len(ds) == int(g['item.%s.len' % name]), name
        i = index if phase == 'train' else index * skip
        sid = i % len(ds.frames)
        assert (ds.subjects[sid], ds.frames[sid]) == (str(g['item.%s.subject' % name]), str(g['item.%s.frame' % name])), name
        if not rnd:
            assert ds.view_ids(sid, (i // len(ds.frames)) % len(ds.test_views)) == g['item.%s.view_ids' % name].tolist(), name
    ds, _ = K.build(str(tmp_path), 'train_random', 'cpu')
    np.random.seed(K.RANDOM_SEED)
    assert ds.view_ids(1, 2, True) == g['item.train_random.view_ids'].tolist()


def test_render_phase_and_moving_camera_are_refused(tmp_path):
    from xrnerf_amd.pipelines import build_dataset
    opt = K.write_tree(str(tmp_path))
    with pytest.raises(NotImplementedError):
        build_dataset(dict(type='GeneBodyDataset', opt=opt, phase='render', pipeline=[]))
    with pytest.raises(NotImplementedError):
        build_dataset(dict(type='GeneBodyDataset', opt=opt, phase='val', move_cam=150, pipeline=[]))
    build_dataset(dict(type='GeneBodyDataset', opt=opt, phase='train', move_cam=150, pipeline=[], device='cpu'))       # a training set ignores move_cam


def test_masks_and_crops_the_reference_breaks_on_are_refused():
    store = genebody.ViewStore('cpu', 16)
    img = np.zeros((48, 40, 3), np.uint8)
    for bad in (np.zeros((48, 40, 3), np.uint8), np.zeros((48, 40), np.uint16), np.zeros((48, 40), bool)):
        with pytest.raises(ValueError):
            store.prepare([(img, bad, None)])
        with pytest.raises(ValueError):
            RS.prepare_view(img, bad, None, 16)
    tall = np.zeros((48, 40), np.uint8)
    tall[1:47, 30:38] = 255                                                         # a 46-row box in a 40-column picture, against the right edge
    box = RS.crop_box(tall)
    assert box[1] < 0
    with pytest.raises(ValueError):
        RS.prepare_view(img, tall, None, 16)
    low = np.zeros((48, 40), np.uint8)
    low[1:47, 2:8] = 255                                                            # the same against the left edge: right = size > w
    assert RS.crop_box(low)[3] > 40
    with pytest.raises(ValueError):
        RS.prepare_view(img, low, None, 16)
