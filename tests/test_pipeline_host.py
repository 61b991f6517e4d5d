"""xrnerf_amd/pipelines.py without a GPU: the tensor-op path on host tensors against tests/golden/ref_pipeline.npz, the agreement of the
header, the ctypes table and the build recipe, the registries, and SceneBaseDataset on a tiny Blender-format scene."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pipeline_cases as K  # noqa: E402
import pipeline_scene as SC  # noqa: E402
from xrnerf_amd import pipelines  # noqa: E402

CPU = torch.device('cpu')


@pytest.mark.parametrize('name', K.CASE_NAMES)
def test_tensor_op_path_on_host_tensors_is_the_fixture(name):
    """a fusable run, but the inputs are host tensors: the transforms run one by one and give the fixture's bits"""
    K.check_fixture_compose(CPU, name, fused=False)


def test_restatement_in_float32_is_within_the_stored_deviation_scale():
    """tests/pipeline_restatement.py run in float32 stays within a few ulp of the fixture (the generator asserts the float64 side)"""
    import pipeline_restatement as RS
    c = K.CASES['mip_H6_test']
    pose, _, _ = K.inputs('mip_H6_test')
    got = RS.ray_front(c['H'], c['W'], K.intrinsics(c), c2w=pose[:3, :4], with_viewdirs=True, with_radii=True, near=2., far=6., S=5, dtype=np.float32)
    outs, _ = K.expected('mip_H6_test')
    for k in ('rays_d', 'viewdirs', 'radii', 'z_vals'):
        assert np.abs(got[k].astype(np.float64) - outs[k][0]).max() <= 16 * 2.0 ** -24 * max(1.0, np.abs(outs[k][0]).max()), k
    with pytest.raises(ValueError):
        RS.ray_front(2, 5, K.intrinsics(c), c2w=pose[:3, :4], with_radii=True)


def test_header_table_and_build_recipe_agree():
    from xrnerf_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_pipeline.h')).read()
    declared = set(re.findall(r'^(?:int|size_t) (xr_pipe_\w+)\(', header, re.M))
    assert declared == set(_lib.PIPELINE_SIGNATURES) == {'xr_pipe_ray_front'}
    for name, (res, args) in _lib.PIPELINE_SIGNATURES.items():
        text = header[header.index(' %s(' % name):]
        assert text[:text.index(');')].count(',') + 1 == len(args), name
    others = [v for k, v in vars(_lib).items() if k.endswith('SIGNATURES') and k != 'PIPELINE_SIGNATURES']
    assert len(others) >= 11 and not any(k.startswith('xr_pipe_') for t in others for k in t)
    assert 'xr_pipe_' not in open(os.path.join(ROOT, 'include', 'xrnerf_mi355.h')).read()
    assert build.SOURCES['xr_pipeline.hip'] == ['-ffp-contract=off']
    source = open(os.path.join(ROOT, 'xrnerf_amd', 'csrc', 'xr_pipeline.hip')).read()
    assert set(re.findall(r'extern "C" int (xr_\w+)\(', source)) == declared


def test_registries():
    with pytest.raises(KeyError):
        pipelines.Compose([dict(type='NoSuchTransform')])
    with pytest.raises(KeyError):
        pipelines.build_dataset(dict(type='NoSuchDataset', cfg={}, pipeline=[]))
    with pytest.raises(TypeError):
        pipelines.Compose([3])
    with pytest.raises(NotImplementedError, match='deepvoxels'):
        pipelines.build_dataset(dict(type='SceneBaseDataset', cfg=dict(dataset_type='deepvoxels', datadir='.'), pipeline=[]))
    for name in ('ToTensor', 'Sample', 'BatchSample', 'GetRays', 'SelectRays', 'FlattenRays', 'GetViewdirs', 'ToNDC', 'GetBounds', 'GetZvals',
                 'PerturbZvals', 'GetPts', 'DeleteUseless', 'Compose'):
        assert name in pipelines.PIPELINES, name
    assert 'SceneBaseDataset' in pipelines.DATASETS and 'SceneBaseDataset' not in pipelines.PIPELINES
    assert pipelines.Compose([lambda r: None, dict(type='DeleteUseless', keys=['a'])])({'a': 1}) is None
    assert pipelines.Compose([dict(type='DeleteUseless', enable=False, keys=['a'])])({'a': 1}) == {'a': 1}
    t = pipelines.ToTensor(keys=['a', 'b', 'c', 'd'])({'a': np.zeros(2, np.float32), 'b': [1, 2], 'c': 3, 'd': 0.5})
    assert [t[k].dtype for k in 'abcd'] == [torch.float32, torch.int64, torch.int64, torch.float32]


def test_planning():
    """which lists are fused: the three configs' chains are; a foreign callable, a step out of order or a doubled perturbation is not"""
    for name, c in K.CASES.items():
        comp = pipelines.Compose([dict(s, **K.datainfo(c)) for s in K.pipeline_list(c)])
        assert comp.fused is not None and type(comp.transforms[comp.fused.start]).__name__ in ('GetRays', 'BatchSample'), name
        assert type(comp.transforms[comp.fused.end]).__name__ == ('GetZvals' if c['radius'] else 'GetPts' if c['pts'] else 'GetZvals'), name
    c = K.CASES['llff_ndc_test']
    steps = [dict(s, **K.datainfo(c)) for s in K.pipeline_list(c)]
    assert pipelines.Compose(steps[:3] + [steps[4], steps[3]] + steps[5:]).fused is None                     # ToNDC before GetViewdirs
    assert pipelines.Compose(steps[:2] + steps[3:]).fused is None                                             # no FlattenRays
    assert pipelines.Compose(steps[:5] + steps[6:]).fused is None                                             # GetZvals without GetBounds
    assert pipelines.Compose([dict(s, randomized=True) if s['type'] == 'GetZvals' else dict(s, enable=True) if s['type'] == 'PerturbZvals' else s
                              for s in steps]).fused is None


@pytest.mark.parametrize('kind', ['blender', 'blender_batching', 'mip'])
def test_scene_base_dataset(tmp_path, kind):
    ds = SC.datasets(CPU, str(tmp_path), kind)
    tr, va, te = ds['train'], ds['val'], ds['test']
    H, W, (n_train, n_val, n_test) = SC.H, SC.W, SC.N_SPLIT
    assert len(tr) == (n_train * H * W // SC.N_RAND if kind == 'blender_batching' else n_train) and len(va) == 1 and len(te) == n_test
    info = tr.get_info()
    assert sorted(info) == ['H', 'K', 'W', 'far', 'focal', 'hwf', 'near', 'render_poses'] and (info['H'], info['W'], info['near'], info['far']) == (H, W, 2., 6.)
    assert np.allclose(info['K'], [[info['focal'], 0, 0.5 * W], [0, info['focal'], 0.5 * H], [0, 0, 1]]) and tuple(info['render_poses'].shape) == (40, 4, 4)
    assert tuple(tr.images.shape) == (n_train + n_val + n_test, H, W, 3) and tr.images.dtype == torch.float32      # white background: RGB
    fetch = tr._fetch_train_data(1)
    if kind == 'blender_batching':
        assert sorted(fetch) == ['idx', 'iter_n', 'rays_rgb'] and tuple(fetch['rays_rgb'].shape) == (n_train * H * W, 3, 3)
        rows = fetch['rays_rgb']
        # the table holds every training pixel once, shuffled: one origin per training image, the colours of the training images
        assert torch.allclose(rows[:, 2].sum(0), tr.images[tr.i_train].reshape(-1, 3).sum(0), rtol=1e-5)
        assert not torch.equal(rows[:H * W, 2], tr.images[tr.i_train[0]].reshape(-1, 3))
        assert rows[:, 0].unique(dim=0).shape[0] == n_train
    else:
        assert sorted(fetch) == ['i_data', 'idx', 'images', 'iter_n', 'poses'] and fetch['idx'] == 1 and fetch['iter_n'] == 0
    assert sorted(va._fetch_val_data(0)) == ['images', 'poses', 'spiral_poses'] and tuple(va[0]['poses'].shape) == (n_test, 4, 4)
    one = te[2]
    assert sorted(one) == ['idx', 'image', 'pose'] and one['idx'] == 2 and torch.equal(one['image'], te.images[te.i_test[2]])
    item = tr[0]
    want = {'rays_o': (SC.N_RAND, 3), 'rays_d': (SC.N_RAND, 3), 'viewdirs': (SC.N_RAND, 3), 'near': (SC.N_RAND, 1), 'far': (SC.N_RAND, 1),
            'z_vals': (SC.N_RAND, SC.S), 'target_s': (SC.N_RAND, 3)}
    want.update({'radii': (SC.N_RAND, 1)} if kind == 'mip' else {'pts': (SC.N_RAND, SC.S, 3)})
    assert {k: tuple(v.shape) for k, v in item.items()} == want
    if kind == 'blender':                       # set_iter reaches SelectRays' precrop: iteration 0 draws from the 4 x 2 centre window
        code = torch.arange(H * W, dtype=torch.float32).reshape(1, H, W, 1) * torch.ones(3)
        tr.images = code.expand(tr.images.shape[0], H, W, 3).contiguous()
        window = {h * W + w for h in range(H // 2 - 2, H // 2 + 2) for w in range(W // 2 - 1, W // 2 + 1)}
        assert {int(v) for v in tr[0]['target_s'][:, 0]} == window
        tr.set_iter(1)
        tr.pipeline.transforms[4].sel_n = 40
        assert len({int(v) for v in tr[0]['target_s'][:, 0]}) == 40
    frame = va.pipeline({'pose': va.poses[0]})
    assert tuple(frame['rays_o'].shape) == (H * W, 3) and frame['src_shape'].tolist() == [H, W, 3] and 'pose' not in frame
    batched = next(iter(pipelines.iterate(te)))
    assert tuple(batched['pose'].shape) == (1, 4, 4) and batched['idx'].tolist() == [0] and batched['image'].data_ptr() == te.images[te.i_test[0]].data_ptr()


@pytest.mark.parametrize('no_ndc', [True, False])
def test_scene_base_dataset_llff(tmp_path, no_ndc):
    """configs/nerf/nerf_llff_base01.py's data dicts on a tiny forward-facing scene: the hold-out split, the bounds of both no_ndc
    settings, the batching table and an item; the NDC item's points start on the near plane z = -1 -> ndc z = -1"""
    SC.write_llff_scene(str(tmp_path))
    data = SC.llff_data_cfg(str(tmp_path), no_ndc)
    tr, va, te = (pipelines.build_dataset(dict(data[k], device=CPU)) for k in ('train', 'val', 'test'))
    assert te.i_test.tolist() == [0, 3] and tr.i_train.tolist() == [1, 2, 4, 5] and tr.hwf[:2] == [6, 8] and abs(tr.hwf[2] - 75.0) < 1e-4
    if no_ndc:
        assert 0 < tr.near < tr.far and tr.far > 5 * tr.near and isinstance(tr.near, float)
    else:
        assert (tr.near, tr.far) == (0., 1.)
    assert tuple(tr.rays_rgb.shape) == (4 * 48, 3, 3) and len(tr) == 4 * 48 // SC.N_RAND and len(va) == 1 and len(te) == 2
    item = tr[1]
    assert sorted(item) == ['far', 'near', 'pts', 'rays_d', 'rays_o', 'target_s', 'viewdirs', 'z_vals'] and tuple(item['pts'].shape) == (SC.N_RAND, SC.S, 3)
    assert torch.equal(item['target_s'], tr.rays_rgb[SC.N_RAND:2 * SC.N_RAND, 2])
    if not no_ndc:
        assert torch.allclose(item['rays_o'][:, 2], torch.full((SC.N_RAND,), -1.0), atol=1e-5) and float(item['pts'][..., 2].max()) <= 1.0 + 1e-5
    frame = te.pipeline({'pose': te[1]['pose']})
    assert tuple(frame['pts'].shape) == (48, SC.S, 3) and frame['src_shape'].tolist() == [6, 8, 3]


@pytest.mark.parametrize('kind', ['blender', 'blender_batching'])
def test_nerf_network_trains_and_validates_from_build_dataset_on_the_host(tmp_path, kind):
    SC.check_train_and_validate(CPU, str(tmp_path), kind)
