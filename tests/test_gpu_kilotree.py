"""xr_kilotree_val_metrics on the MI355X (xrnerf_amd/csrc/xr_kilotree.hip through ops.kilo_val_metrics): against the float64 restatement
(tests/kilotree_restatement.py) and against the reference's own calculate_error_metrics / get_equal_error_split_threshold
(tests/golden/ref_kilotree.npz).  The bodies and their bounds are tests/kilotree_cases.py's."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kilotree_cases as K  # noqa: E402
import kilotree_restatement as R  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('P', K.SMALL_P + K.BLOCK_P)
@pytest.mark.parametrize('N', (1, 5))
def test_shapes_against_the_restatement(dev, N, P):
    K.check_shape(dev, N, P)


def test_validation_size_against_the_restatement(dev):
    """N = 3, P = 20000: the shipped configs' validation size, the only large case"""
    N, P = 3, 20000
    out, tgt, pts = K.inputs(N, P, 99)
    qi = int(P * 0.99)
    axis = [0, 1, 2]
    got, _ = K.run(dev, out, tgt, pts, qi, axis, 'mse')
    assert K.compare(got, R.val_metrics(out, tgt, qi, pts, axis, 'mse'), P, 'N 3 P 20000') == 0


def test_tied_coordinates_and_tied_errors(dev):
    K.check_ties(dev)


def test_nan_zero_total_and_no_split(dev):
    K.check_odd_values(dev)


def test_crafted_saturation_rows(dev):
    K.check_saturation(dev)


def test_two_runs_and_permuted_points_give_the_same_bits(dev):
    K.check_repeat_and_permutation(dev)


def test_refusals(dev):
    K.check_refusals(dev)


@pytest.mark.parametrize('key', ['p%d' % p for p in K.SMALL_P] + ['p20000'])
def test_against_the_reference(dev, key):
    K.check_reference_metrics(dev, key)


def test_python_entry_points_against_the_reference(dev):
    """kilo_tree.calculate_error_metrics / get_equal_error_split_threshold: the reference's signatures and return values on the kernel"""
    from xrnerf_amd import kilo_tree as T
    from xrnerf_amd.builder import ConfigDict
    g = K.gold()
    key = 'p300'
    out, tgt, pts = (torch.from_numpy(g[key + '.' + k]).to(dev) for k in ('out', 'targets', 'points'))
    cfg = ConfigDict.wrap(dict(outputs='color_and_density', quantile_se=0.99, equal_split_metric='mse'))
    per_point, per_net, per_color, per_density, sat = T.calculate_error_metrics(out, tgt, cfg)
    ref = g[key + '.table']
    for i, m in enumerate(('mse', 'mae', 'mape')):
        for j, d in enumerate((per_net, per_color, per_density)):
            assert not d[m].is_cuda and np.allclose(d[m].numpy(), ref[:, 3 * i + j], rtol=1e-6, atol=0), (m, j)
    assert np.array_equal(per_density['quantile_se'].numpy(), ref[:, 11]) and per_point['quantile_se'] is None
    assert np.array_equal(sat.numpy(), g[key + '.saturation'])
    *_, thr = T.calculate_error_metrics(out, tgt, cfg, test_points=pts, split_axis=[1] * out.shape[0])
    assert np.array_equal(np.asarray(thr, np.float32), g[key + '.threshold'][:, 1])
    one = T.get_equal_error_split_threshold(pts[2].cpu(), per_point['mse'][2], 0)
    assert np.float32(one) == g[key + '.threshold'][2, 0]
    with pytest.raises(IndexError):
        T.calculate_error_metrics(out, tgt, ConfigDict.wrap(dict(outputs='color_and_density', quantile_se=1.0)))
