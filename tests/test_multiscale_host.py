"""xrnerf_amd/multiscale.py without a GPU: the host path of MipMultiScaleDataset (the reference's tables, materialised from the float64
restatement) and of the converter against tests/golden/ref_multiscale.npz, MipMultiScaleSample on plain tensors, the planners, the
registries, and the agreement of the header, the ctypes table and the build recipe."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import multiscale_cases as K  # noqa: E402
import multiscale_restatement as RS  # noqa: E402
from xrnerf_amd import multiscale, pipelines  # noqa: E402

CPU = torch.device('cpu')


def test_registries_hold_the_config_names():
    assert 'MipMultiScaleDataset' in pipelines.DATASETS and 'MipMultiScaleSample' in pipelines.PIPELINES
    assert multiscale.MipMultiScaleDataset.mode == 'train' and repr(multiscale.MipMultiScaleSample()) == 'MipMultiScaleSample:slice a batch of rays from all rays'
    p = '/root/reference/configs/mipnerf/mipnerf_multiscale.py'
    if os.path.exists(p):                                    # the data dicts the tests build are the reference config's, reduced
        import runpy
        ref = runpy.run_path(p)['data']
        mine = K.data_cfg('data/multiscale/#DATANAME#', n_rand=1024, num_samples=128)
        assert ref == mine


def test_header_table_and_build_recipe_agree():
    K.check_symbols(loaded=False)


def test_existing_pipelines_plan_as_before():
    K.check_existing_plans_unchanged()


def test_sample_on_plain_tensors_is_the_fixture():
    K.check_tensor_sample(CPU)


def test_host_tables_are_the_reference_tables():
    """the package's own host restatement (what the dataset materialises without the library) and the tests' give the fixture's bits"""
    g = K.gold()
    meta = {k: np.array(v) for k, v in K.fixture_meta(K.conv_meta()).items()}
    spec = RS.tables(meta)
    for i in range(10):
        f = multiscale._frame_rays(meta['pix2cam'][i], meta['cam2world'][i], meta['height'][i], meta['width'][i], meta['lossmult'][i], meta['near'][i], meta['far'][i])
        lo = int(np.sum(meta['height'][:i] * meta['width'][:i]))
        for k in K.RAY_KEYS:
            got = np.ascontiguousarray(f[k].reshape(-1, f[k].shape[-1]).astype(np.float32))
            K.same_bits(got, g['table.' + k][lo:lo + got.shape[0]], 'host frame %d %s' % (i, k))
    for k in K.RAY_KEYS:
        K.same_bits(spec[k], g['table.' + k], 'restatement %s' % k)
    base = K.base_views()
    saved, packed = multiscale._host_pyramid(base, K.N_DOWN, True)
    K.same_bits(saved, g['pyramid.bytes'], 'host pyramid bytes')
    K.same_bits(packed, g['pyramid.pixels'], 'host pyramid pixels')


def test_dataset_on_the_host_is_the_fixture(tmp_path):
    ds = K.check_dataset(CPU, str(tmp_path))
    tr, te = ds['train'], ds['test']
    assert not tr.native and tr.table is None and sorted(tr.rays) == sorted(K.RAY_KEYS) and tuple(tr.images.shape) == (791, 3)
    assert sorted(tr._fetch_train_data(0)) == sorted(K.ALL_KEYS) and sorted(te._fetch_test_data(1)) == sorted(['image', 'idx'] + K.RAY_KEYS)
    assert isinstance(te.images, list) and tuple(te.rays['radii'][9].shape) == (5, 7, 1)
    with pytest.raises(NotImplementedError):
        pipelines.build_dataset(dict(type='MipMultiScaleDataset', cfg=dict(dataset_type='blender', datadir=str(tmp_path), white_bkgd=True), pipeline=[]))


def test_converter_on_the_host_and_round_trip(tmp_path):
    K.check_converter(CPU, str(tmp_path))


def test_h2_and_odd_sizes_raise():
    K.check_h2_raises(CPU)
    from xrnerf_amd import ops
    for hw in ((12, 18), (10, 16), (13, 16)):
        with pytest.raises(ValueError):
            ops.ms_pyramid_sizes(hw[0], hw[1], 3)
    with pytest.raises(ValueError):
        ops.ms_pyramid_sizes(16, 16, 9)
    assert ops.ms_pyramid_sizes(800, 800, 4) == [(800, 800), (400, 400), (200, 200), (100, 100)]
