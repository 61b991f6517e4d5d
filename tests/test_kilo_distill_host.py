"""KiloNeRF distillation (xrnerf_amd/kilo_distill.py, the student / occupancy kernels of xrnerf_amd/csrc/xr_kilo.hip) without a
GPU: the registry surface and initialisation against the reference's own StudentNerfNetwork / KiloNerfMultiNetwork
(tests/golden/ref_kilo_distill.npz, tests/golden/make_golden_kilo_distill.py), and the new kernels' host build (tests/hip_emu)
against the same fixture."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
G = os.path.join(ROOT, 'tests', 'golden', 'ref_kilo_distill.npz')


@pytest.fixture(scope='module')
def gold():
    return np.load(G)


def distill_model_cfg(num_networks):
    """configs/kilonerf/kilonerf_distill_Synthetic_NeRF_base01.py:76-124, pretrained_kwargs=None"""
    return dict(type='StudentNerfNetwork', cfg=dict(outputs='color_and_density', test_batch_size=512, query_batch_size=80000),
                pretrained_kwargs=None,
                multi_network=dict(type='KiloNerfMultiNetwork', num_networks=num_networks, alpha_rgb_initalization='pass_actual_nonlinearity',
                                   bias_initialization_method='standard', direction_layer_size=32, hidden_layer_size=32,
                                   late_feed_direction=True, network_rng_seed=8078673, nonlinearity_initalization='pass_actual_nonlinearity',
                                   num_hidden_layers=2, num_output_channels=4, refeed_position_index=None,
                                   use_same_initialization_for_all_networks=False, weight_initialization_method='kaiming_uniform',
                                   embedder=dict(type='KiloNerfFourierEmbedder', num_networks=num_networks, input_ch=3, multires=10,
                                                 multires_dirs=4)),
                render=dict(type='KiloNerfSimpleRender', alpha_distance=0.0211, convert_density_to_alpha=True))


def teacher_from(gold):
    from xrnerf_amd.vanilla import NerfMLP
    t = NerfMLP(skips=[4], netdepth=8, netwidth=64, output_ch=4, use_viewdirs=True,
                embedder=dict(type='BaseEmbedder', i_embed=0, multires=10, multires_dirs=4, input_ch=3))
    t.load_state_dict({k[len('teacher.'):]: torch.tensor(gold[k]) for k in gold.files if k.startswith('teacher.')})
    return t


def build_pair(gold):
    """the fixture's two consecutive constructions, from a fresh class-level generator state"""
    import xrnerf_amd
    from xrnerf_amd import kilo_distill as KD
    KD.MultiNetworkLinear.rng_state = None
    net = xrnerf_amd.build_network(distill_model_cfg(8))
    second_cfg = dict(distill_model_cfg(8)['multi_network'], use_same_initialization_for_all_networks=True)
    second = xrnerf_amd.build_mlp(second_cfg)
    return net, second


def test_distill_model_builds_through_the_registry_with_a_teacher(gold):
    from xrnerf_amd import kilo_distill as KD
    net, _ = build_pair(gold)
    assert isinstance(net, KD.StudentNerfNetwork) and isinstance(net.multi_network, KD.KiloNerfMultiNetwork)
    assert isinstance(net.render, KD.KiloNerfSimpleRender) and net.render.alpha_distance == 0.0211
    assert getattr(net, 'teacher_nerf', None) is None
    net2 = KD.StudentNerfNetwork(distill_model_cfg(8)['cfg'], multi_network=distill_model_cfg(8)['multi_network'],
                                 render=distill_model_cfg(8)['render'], teacher=teacher_from(gold))
    assert net2.teacher_nerf is not None and net2.get_params() == list(net2.multi_network.parameters())


def test_state_dict_keys_and_shapes_match_the_reference(gold):
    net, second = build_pair(gold)
    want = [k[len('init.'):] for k in gold.files if k.startswith('init.')]
    sd = net.multi_network.state_dict()
    assert list(sd.keys()) == want
    for k in want:
        assert tuple(sd[k].shape) == gold['init.' + k].shape, k
    assert list(second.state_dict().keys()) == want


def test_initialisation_is_bit_identical_for_both_constructions(gold):
    net, second = build_pair(gold)
    for tag, m in (('init.', net.multi_network), ('init2.', second)):
        for k, v in m.state_dict().items():
            assert np.array_equal(v.numpy().view(np.uint32), gold[tag + k].view(np.uint32)), tag + k
    # the second construction continued the stream and copied network 0 everywhere
    w = second.state_dict()['multi_network.pts_linears.0.weight']
    assert torch.equal(w[1:], w[:1].expand_as(w[1:]))
    assert not np.array_equal(gold['init.multi_network.pts_linears.0.weight'][0], gold['init2.multi_network.pts_linears.0.weight'][0])


def test_simple_render_keeps_the_two_activations():
    from xrnerf_amd.kilo_distill import KiloNerfSimpleRender
    r = KiloNerfSimpleRender(alpha_distance=0.5)
    raw2 = torch.tensor([[0., 0., 0., -2.]])
    raw3 = raw2[None]
    assert float(r({'raw': raw2})[1][0, 3]) == 0.                      # relu: no density below zero
    assert float(r({'raw': raw3})[1][0, 0, 3]) < 0.                    # leaky_relu: a small negative alpha


def emu_state(gold):
    """fixture tensors for the emulated kernels: examples, teacher raw, domains, the initial packed blocks"""
    net, _ = build_pair(gold)
    mn = net.multi_network.multi_network
    return (torch.tensor(gold['examples']), torch.tensor(gold['teacher_raw']), torch.tensor(gold['domain_mins']),
            torch.tensor(gold['domain_maxs']), mn)


def test_student_step_kernel_on_the_emulator_matches_the_reference(gold):
    import emulib
    from xrnerf_amd import kilo_distill as KD
    ex, tr, dmin, dmax, mn = emu_state(gold)
    with emulib.emulated_ops():
        params = mn.packed().clone()
        loss, grad = KD.student_step(ex, tr, dmin, dmax, params, 10, 4, 2, 0.0211)
        loss2, grad2 = KD.student_step(ex, tr, dmin, dmax, params, 10, 4, 2, 0.0211)
    assert abs(float(loss.sum()) - float(gold['loss'])) <= 1e-5 * max(1., abs(float(gold['loss'])))
    assert torch.equal(grad, grad2) and torch.equal(loss, loss2)
    grads = mn.grads_from_blocks(grad)
    for (k, _), g in zip(mn.named_parameters(), grads):
        ref = gold['grad.multi_network.' + k]
        scale = max(np.abs(ref).max(), 1e-6)
        assert np.abs(g.numpy() - ref).max() <= 2e-4 * scale, k
    # the fused Adam step vs the reference's first torch.optim.Adam(lr=1e-3) step: a step is ~lr * g / (|g| + eps), so where a
    # gradient is within fp32 noise of zero its direction may differ -- the bar is 2 % of lr
    with emulib.emulated_ops():
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        KD.student_step(ex, tr, dmin, dmax, params, 10, 4, 2, 0.0211, adam=dict(m=m, v=v, step=1, lr=1e-3))
    mn.load_packed(params)
    for k, p in mn.named_parameters():
        ref = gold['adam1.multi_network.' + k]
        assert np.abs(p.detach().numpy() - ref).max() <= 2e-5, k


def test_student_forward_and_occupancy_kernels_on_the_emulator(gold):
    import emulib
    from xrnerf_amd import kilo_distill as KD
    ex, tr, dmin, dmax, mn = emu_state(gold)
    res, sub = [int(v) for v in gold['occ_res']], [int(v) for v in gold['occ_sub']]
    with emulib.emulated_ops():
        out = KD.student_forward(ex, mn.packed(), 10, 4, 2, domain_mins=dmin, domain_maxs=dmax, render=True, alpha_distance=0.0211)
        total = int(np.prod(res))
        pts = KD.occupancy_points(gold['gmin'].tolist(), gold['gmax'].tolist(), res, sub, 0, total, torch.device('cpu'))
        pts_tail = KD.occupancy_points(gold['gmin'].tolist(), gold['gmax'].tolist(), res, sub, 7, 5, torch.device('cpu'))
        raw = torch.zeros((total * 27, 4))
        raw[:, 3] = torch.tensor(gold['occ_density']).reshape(-1)
        occ = torch.empty(res, dtype=torch.bool)
        KD.occupancy_reduce(raw, 27, float(gold['occ_threshold']), occ.view(-1))
    assert np.abs(out.numpy() - gold['student_out']).max() <= 1e-5
    ref_pts = gold['occ_points'].reshape(-1, 3)
    assert np.array_equal(pts.numpy().view(np.uint32), ref_pts.view(np.uint32))
    assert np.array_equal(pts_tail.numpy(), ref_pts[7 * 27:12 * 27])
    assert np.array_equal(occ.numpy(), gold['occ_grid'])


def test_example_generator_on_the_emulator():
    import emulib
    from xrnerf_amd import kilo_distill as KD
    dmin = torch.tensor([[-1., -1., -1.], [0., 0., 0.5]])
    dmax = torch.tensor([[0., 0., 0.], [0.25, 2., 0.75]])
    with emulib.emulated_ops():
        a = KD.distill_examples(dmin, dmax, 64, 3, 11, 1000)
        b = KD.distill_examples(dmin, dmax, 64, 3, 11, 1000)
        c = KD.distill_examples(dmin, dmax, 64, 3, 12, 1000)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert bool((a[..., :3] >= dmin[:, None]).all() and (a[..., :3] <= dmax[:, None]).all())
    assert torch.allclose(a[..., 3:6].norm(dim=-1), torch.ones(2, 64), atol=1e-5)


def test_host_tensors_raise():
    from xrnerf_amd import _lib, kilo_distill as KD
    with pytest.raises(_lib.XrError):
        KD.distill_examples(torch.zeros(1, 3), torch.ones(1, 3), 4, 0, 0)
