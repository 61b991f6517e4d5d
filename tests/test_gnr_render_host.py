"""GNR's renderer stages on the host path of xrnerf_amd/gnr_render.py (the reference's lines as tensor ops): the bodies of
tests/test_gpu_gnr_render.py on host tensors.  Also holds tests/gnr_render_restatement.py to the fixture, so that the shapes the
fixture does not store are checked against something the reference itself has checked."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_gnr_render as T  # noqa: E402

G = os.path.join(ROOT, 'tests', 'golden')
CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_gnr_render.npz'))


@pytest.mark.parametrize('R,V', T.HULL_CASES)
def test_hull_flags_order_and_rows(gold, R, V):
    T.check_hull(CPU, gold, R, V)


def test_hull_with_the_training_draws(gold):
    T.check_hull(CPU, gold, 48, 4, 'trn')


def test_hull_nan_ray_camera_behind_and_nothing_to_do(gold):
    T.check_hull_edges(CPU, gold)


@pytest.mark.parametrize('N,C', T.GATHER_CASES)
def test_gather_against_float64_grid_sample(gold, N, C):
    T.check_gather(CPU, gold, N, C)


@pytest.mark.parametrize('mode', T.MODES)
def test_gather_holds_the_fixture(gold, mode):
    T.check_gather_fixture(CPU, gold, mode)


@pytest.mark.parametrize('N,C', T.GATHER_BWD_CASES)
def test_gather_backward_to_the_feature_maps(gold, N, C):
    T.check_gather_backward(CPU, gold, N, C)


@pytest.mark.parametrize('mode', T.MODES)
def test_compositor_holds_the_fixture_forward_and_backward(gold, mode):
    T.check_composite_fixture(CPU, gold, mode)


@pytest.mark.parametrize('V,white,S', T.COMPOSITE_CASES)
def test_compositor_empty_full_and_opaque_rays(gold, V, white, S):
    T.check_composite_cases(CPU, gold, V, white, S)


@pytest.mark.parametrize('mode', T.MODES)
def test_stages_chained_on_the_fixture(gold, mode):
    T.check_end_to_end_stages(CPU, gold, mode)


@pytest.mark.parametrize('mode', T.MODES)
def test_the_restatement_holds_the_fixture(gold, mode):
    """the float64 restatement against the reference's float64 run: hull decisions and rows, gathered columns, compositor and its
    gradient"""
    import gnr_render_restatement as RS
    inp = T.hull_inputs(CPU, gold, mode, 48, 4)
    h = T.hull64(inp)
    compared = gold[mode + '.boundary'] > 1e-3
    assert np.array_equal(h['inside'].numpy()[compared], gold[mode + '.inside'][compared])
    assert np.array_equal(h['boundary'].numpy() > 1e-3, compared), 'the same points are left out'
    if np.array_equal(h['inside'].numpy(), gold[mode + '.inside']):
        for k in ('pts', 'xy', 'z', 'attdirs'):
            T.held(h[k].numpy(), gold['%s.%s' % (mode, k)], gold['%s.%s64' % (mode, k)], 'restatement %s' % k, columns=(k == 'attdirs'))
        sure = gold[mode + '.vis_margin'] > 1e-4
        assert np.array_equal(h['vis'].numpy()[sure], gold[mode + '.smpl_vis'][sure])
        assert np.array_equal(h['vis_margin'].numpy() > 1e-4, sure)
    sc = T.scene()
    ni = gold[mode + '.nerf_input']
    C = sc['feats'].shape[1]
    g = RS.gather(torch.from_numpy(gold[mode + '.xy64']), sc['feats'].double(), sc['images'].double()).numpy()
    T.held(g, ni[..., ni.shape[-1] - C - 3:], gold[mode + '.gathered64'], 'restatement gather', columns=True)
    ci = T.composite_inputs(CPU, gold, mode)
    ci['net'], ci['source_rgb'] = torch.from_numpy(gold[mode + '.net64']), torch.from_numpy(gold[mode + '.source_rgb64'])
    ci['t_vals'] = torch.from_numpy(gold[mode + '.t_vals'])
    rgb_map, depth, acc, weights, d_net = T.dense(ci, torch.float64)
    for name, got in (('rgb_map', rgb_map), ('depth', depth), ('weights', weights), ('d_net', d_net)):
        T.held(got, gold['%s.%s' % (mode, name)], gold['%s.%s64' % (mode, name)], 'restatement %s' % name, columns=(name in ('rgb_map', 'd_net')))


@pytest.fixture(scope='module')
def params():
    return T.load_params()


def test_gnrmlp_strict_load_output_alpha_only_and_parameter_gradients(gold, params):
    T.check_mlp(CPU, gold, params)


def test_gnrmlp_with_two_views_against_the_restatement(gold, params):
    T.check_mlp_two_views(CPU, gold, params)


@pytest.mark.parametrize('mode', T.MODES)
def test_render_rays_on_the_fixture(gold, params, mode):
    T.check_render_rays(CPU, gold, params, mode)


def test_config_builds_refusals_and_empty_hull(gold, params):
    T.check_renderer_contract(CPU, gold, params)


def test_header_table_and_library_name_the_same_entry_points():
    T.check_tables_in_step()


def test_the_mlp_restatement_holds_the_fixture(gold, params):
    """tests/gnr_render_restatement.gnr_mlp in float64 against the reference's float64 network output"""
    import gnr_render_restatement as RS
    sd = {k[2:]: torch.from_numpy(params[k]).double() for k in params.files if k.startswith('w.')}
    for mode in T.MODES:
        out = RS.gnr_mlp(sd, torch.from_numpy(gold[mode + '.nerf_input']).double(), torch.from_numpy(gold[mode + '.attdirs64']),
                         torch.from_numpy(gold[mode + '.smpl_vis']))
        T.held(out.numpy()[:, :9], gold[mode + '.net'], gold[mode + '.net64'], 'restatement GNRMLP %s' % mode, columns=True)
