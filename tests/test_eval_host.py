"""The tensor-op path of xrnerf_amd/evaluate.py (host tensors and numpy arrays, torch float64) through the bodies of tests/eval_cases.py,
the fixture against its own references, and the header / table / build recipe of the kernels -- no GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import eval_cases as K  # noqa: E402
import eval_restatement as RS  # noqa: E402
from xrnerf_amd import evaluate  # noqa: E402

CPU = torch.device('cpu')


@pytest.mark.parametrize('name', K.CASE_NAMES)
def test_fixture_is_what_its_maker_generates_and_not_vacuous(name):
    """the stored inputs are the generated ones; the scipy composition of this machine reproduces the stored maps to within the
    witnesses' own distance; float64 differs from long double; means in (0.5, 1)"""
    c = K.case(name)
    rgb, gt = K.generate(name)
    K.same_bits(rgb, c['rgb'], name + ' rgb')
    K.same_bits(gt, c['gt'], name + ' gt')
    assert c['witness'][0] > 0 and c['witness'][1] > 0 and c['map_bar'] < 1e-10
    assert ((c['mean_truth'] > 0.5) & (c['mean_truth'] < 1)).all()
    scipy_here = np.stack([RS.scipy_ssim_map(rgb[b], gt[b], 7, c['gauss'], K.DATA_RANGE) for b in range(c['B'])])
    assert np.abs(scipy_here - c['truth']).max() <= c['map_bar']
    assert bool((gt == 1.0).reshape(c['B'], -1).mean(1).min() >= 0.4), 'the flat white half is missing'
    for b in range(c['B']):
        K.same_bits(RS.to8b(np.hstack((rgb[b], gt[b]))), c['to8b'][b], name + ' to8b')


def test_reflection_is_scipys_not_torchs():
    i = evaluate._reflect_index(5, 3, CPU).tolist()
    assert i == [2, 1, 0, 0, 1, 2, 3, 4, 4, 3, 2]
    assert np.array_equal(np.pad(np.arange(5), 3, mode='symmetric'), np.array(i))


def test_windows():
    taps, cov = evaluate.window(7)
    assert taps == [1.0 / 7] * 7 and cov == 49.0 / 48.0
    taps, cov = evaluate.window(7, True)
    ref, _ = RS.window(7, True)
    assert len(taps) == 11 and cov == 1.0 and abs(sum(taps) - 1) < 1e-15 and np.abs(np.array(taps) - ref).max() < 1e-16
    from scipy.ndimage import gaussian_filter1d
    delta = np.zeros(21)
    delta[10] = 1
    assert np.abs(gaussian_filter1d(delta, 1.5, truncate=3.5)[5:16] - np.array(taps)).max() < 1e-16


@pytest.mark.parametrize('name', K.CASE_NAMES)
def test_tensor_ops_fixture_cases_under_their_bars(name):
    K.check_fixture(CPU, name)


def test_numpy_arrays_take_the_same_path():
    c = K.case('7x9')
    a = evaluate.calculate_ssim(c['rgb'][0], c['gt'][0], data_range=K.DATA_RANGE)
    b = evaluate.calculate_ssim(torch.from_numpy(c['rgb'][0]), torch.from_numpy(c['gt'][0]), data_range=K.DATA_RANGE)
    K.same_bits(a, b, 'numpy against tensor')
    K.same_bits(evaluate.img2mse(c['rgb'][0], c['gt'][0]), evaluate.img2mse(torch.from_numpy(c['rgb'][0]), torch.from_numpy(c['gt'][0])), 'img2mse')
    assert isinstance(evaluate.to8b(c['rgb'][0]), np.ndarray)
    K.same_bits(evaluate.to8b(c['rgb'][0]), RS.to8b(c['rgb'][0]), 'to8b of an array')
    # the other documented parameters: the data range, the population covariance, K1 / K2
    x, y = c['rgb'][0], c['gt'][0]
    for kw, ref in ((dict(data_range=1.0), dict(data_range=1.0)), (dict(data_range=None), dict(data_range=2.0))):
        got = float(evaluate.calculate_ssim(x, y, **kw))
        assert abs(got - float(RS.ssim_map(x, y, 7, False, ref['data_range']).mean())) < 1e-12
    pop = float(evaluate.calculate_ssim(x, y, data_range=2.0, use_sample_covariance=False))
    assert pop != float(evaluate.calculate_ssim(x, y, data_range=2.0))


def test_tensor_ops_channel_first_views_and_slices():
    K.check_views_and_slices(CPU)


def test_tensor_ops_identical_images_and_odd_values():
    K.check_degenerate(CPU)


def test_refusals_on_host_tensors():
    K.check_refusals(CPU)
    from xrnerf_amd import _lib, ops
    x = torch.rand((1, 9, 9, 3))
    with pytest.raises(_lib.XrError):                               # host tensors handed to ops.*: there is no quiet CPU run
        ops.eval_ssim(x, x, [1.0 / 7] * 7, 49.0 / 48, 1e-4, 9e-4)
    with pytest.raises(_lib.XrError):
        ops.eval_to8b_pair(x[0], x[0])


@pytest.mark.parametrize('kind', ('numpy', 'tensor'))
def test_validate_hook_on_host_frames(kind):
    K.check_validate_hook(CPU, kind)


@pytest.mark.parametrize('kind', ('numpy', 'tensor'))
def test_test_hook_on_host_frames(kind):
    K.check_test_hook(CPU, kind)


def test_evaluate_frames_on_host_frames():
    K.check_evaluate_frames(CPU, *K.fixture_renderer(CPU))


def test_metrics_serve_gnr_cal_metrics():
    """psnr_metric / ssim_metric as the 'psnr' and 'ssim' entries of the dict GnrNetwork.cal_metrics takes"""
    from xrnerf_amd.gnr_network import GnrNetwork
    c = K.case('9x13')
    rgbs = torch.from_numpy(c['rgb'][..., :3].copy())                       # [3,9,13,3], as render_path returns them
    gts = torch.from_numpy(c['gt'][..., :3].copy()).permute(0, 3, 1, 2)    # [3,3,9,13], as the loader's render_gt
    out = GnrNetwork.cal_metrics(None, {'psnr': evaluate.psnr_metric, 'ssim': evaluate.ssim_metric}, rgbs, gts)
    assert sorted(out) == ['psnr', 'ssim'] and tuple(out['psnr'].shape) == (3,) and tuple(out['ssim'].shape) == (3,)
    for b in range(3):
        want = evaluate.calculate_ssim(rgbs[b], gts[b].permute(1, 2, 0), data_range=evaluate.REFERENCE_SSIM_DATA_RANGE)
        K.same_bits(out['ssim'][b], want, 'ssim_metric %d' % b)


def test_table_header_and_recipe_name_the_same_entry_points():
    import re
    from xrnerf_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_eval.h')).read()
    assert set(re.findall(r'^(?:int|size_t) (xr_eval_\w+)\(', header, re.M)) == set(_lib.EVAL_SIGNATURES)
    others = [v for k, v in vars(_lib).items() if k.endswith('SIGNATURES') and k != 'EVAL_SIGNATURES']
    assert len(others) >= 10 and not any(set(t) & set(_lib.EVAL_SIGNATURES) for t in others)
    assert build.SOURCES['xr_eval.hip'] == ['-ffp-contract=off']
    source = open(os.path.join(ROOT, 'xrnerf_amd', 'evaluate.py')).read()
    assert not re.search(r'^\s*(?:import|from)\s+(?:scipy|skimage)', source, re.M), 'the package imports neither scipy nor skimage'


def test_library_exports_the_declared_symbols():
    """the built library (loading it needs no GPU) exports every xr_eval_* the header declares"""
    K.check_symbols()
