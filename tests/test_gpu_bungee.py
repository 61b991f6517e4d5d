"""BungeeNeRF on the MI355X (xrnerf_amd/bungee.py, csrc/xr_bungee.hip) against the reference's own code (tests/golden/ref_bungee.npz,
made by tests/golden/make_golden_bungee.py) and the float64 restatement (tests/bungee_restatement.py).  Bars as in test_gpu_mip.py.

Measured sphere-bounds gap on the fixture scene: the bounds subtract squares of earth-radius-sized fp32 numbers (xr_bungee.hip's
header); the kernel rounds the reference's expressions in the reference's order, and the fixture's near / far agree to <= 1e-4
relative (the bar is not loosened)."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm device')
    return torch.device('cuda')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_bungee.npz'))


def _t(a, dev, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=dev)


def model_cfg(netwidth=64, cur_stage=2):
    cfg = json.load(open(os.path.join(G, 'bungee_model_cfg.json')))
    m = copy.deepcopy(cfg['model'])
    m['mlp']['netwidth'], m['mlp']['cur_stage'] = netwidth, cur_stage
    return m


def build(dev, netwidth=64, cur_stage=2, gold=None):
    import xrnerf_amd
    net = xrnerf_amd.build_network(model_cfg(netwidth, cur_stage))
    if gold is not None:
        net.load_state_dict({k[5:]: torch.tensor(gold[k]) for k in gold.files if k.startswith('init/')})
    return net.to(dev)


def batch(gold, dev, prefix='b_'):
    b = {k: _t(gold[prefix + k], dev) for k in ('rays_o', 'rays_d', 'viewdirs', 'radii', 'target_s')}
    b['scale_code'] = _t(gold[prefix + 'scale_code'], dev, torch.int64)
    return b


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def check_zvals(dev, gold):
    from xrnerf_amd import ops
    b = batch(gold, dev)
    for mode in ('sphere', 'flat'):
        near, far, z = ops.bungee_zvals(b['rays_o'], b['viewdirs'], None, None, gold['sphere_z'].shape[1], mode,
                                        gold['scene_origin'], float(gold['scene_scale']))
        assert rel(near.cpu(), gold[mode + '_near']) <= 1e-4, mode
        assert rel(far.cpu(), gold[mode + '_far']) <= 1e-4, mode
        # z-values given the fixture's bounds
        _, _, z2 = ops.bungee_zvals(None, b['viewdirs'], _t(gold[mode + '_near'], dev), _t(gold[mode + '_far'], dev),
                                    gold['sphere_z'].shape[1], None)
        g = gold[mode + '_z']
        assert np.abs(z2.cpu().numpy() - g).max() <= 1e-6 * np.abs(g).max(), mode


def check_encode(dev, gold):
    from xrnerf_amd import ops
    b = batch(gold, dev)
    z = _t(gold['sphere_z'], dev)
    for shape, key in (('cone', 'embedded'), ('cylinder', 'embedded_cyl')):
        e = ops.bungee_encode(b['viewdirs'], 10, 4, frustum=(b['rays_o'], b['rays_d'], b['radii'], z), ray_shape=shape)
        assert e.shape[1] == 90
        assert np.abs(e.cpu().numpy() - gold[key]).max() <= 5e-6, shape
    e = ops.bungee_encode(b['viewdirs'], 10, 4, gaussians=(_t(gold['means'], dev), _t(gold['covs'], dev)))
    assert np.abs(e.cpu().numpy() - gold['embedded']).max() <= 5e-6


def check_render(dev, gold):
    from xrnerf_amd import ops
    b = batch(gold, dev)
    raw, z, G = _t(gold['raw'], dev), _t(gold['sphere_z'], dev), _t(gold['G'], dev)
    for st in range(3):
        rgb, disp, acc, w = ops.bungee_render_forward(raw, z, b['viewdirs'], st)
        assert np.abs(w.cpu().numpy() - gold['r%d_weights' % st]).max() <= 2e-6
        for k, v in (('rgb', rgb), ('disp', disp), ('acc', acc)):
            assert rel(v.cpu(), gold['r%d_%s' % (st, k)]) <= 1e-5, (st, k)
        g = ops.bungee_render_backward(raw, z, b['viewdirs'], G, st).cpu().numpy()
        og = gold['r%d_graw' % st]
        assert np.abs(g - og).max() <= 1e-5 * np.abs(og).max(), st
        assert (g[:, :, st + 1:] == 0).all()
    kw = dict(density_bias=-1.0, rgb_padding=0.001, white_bkgd=True, density_activation='relu', noise=_t(gold['noise'], dev))
    rgb, disp, acc, w = ops.bungee_render_forward(raw, z, b['viewdirs'], 1, **kw)
    assert np.abs(w.cpu().numpy() - gold['rn_weights']).max() <= 2e-6
    assert rel(rgb.cpu(), gold['rn_rgb']) <= 1e-5 and rel(acc.cpu(), gold['rn_acc']) <= 1e-5
    g = ops.bungee_render_backward(raw, z, b['viewdirs'], G, 1, **kw).cpu().numpy()
    assert np.abs(g - gold['rn_graw']).max() <= 1e-5 * np.abs(gold['rn_graw']).max()


_RAYS = {}
GLOBE = (0., 0., -6371011.0)
SCALE = 1 / 400


def restatement_rays(R, S):
    """seeded cameras above the globe looking down, raw [R, S, 3 heads, 4], density noise and dL/drgb as float32 numpy; drawn once per
    shape and shared (tests/test_emu_bungee.py runs its kernels on the same rays)"""
    if (R, S) not in _RAYS:
        rng = np.random.default_rng(R * 1000 + S)
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        o = f32(np.stack([rng.uniform(-1, 1, R), rng.uniform(-1, 1, R), rng.uniform(1.5, 8, R)], -1))
        d = rng.normal(0, 0.2, (R, 3)) - [0, 0, 1]
        d = f32(d / np.linalg.norm(d, axis=-1, keepdims=True))
        radii = f32(rng.uniform(1e-4, 1e-3, (R, 1)))
        raw = f32(rng.normal(0, 1.5, (R, S, 3, 4)))
        noise = f32(rng.normal(0, 1, (R, S)))
        g = f32(rng.normal(0, 1, (R, 3)))
        _RAYS[(R, S)] = dict(o=o, d=d, vd=d.copy(), radii=radii, raw=raw, noise=noise, g=g)
    return _RAYS[(R, S)]


def check_render_restatement(dev, R, S):
    """renderer forward / backward of R rays x S intervals against the float64 restatement: stages 0, 1 with noise, 2 and 5 of 3 heads
    (softplus, density_bias -1, no padding, black background).  S = 64 is exactly one sweep of the wave, S = 100 two with a ragged last."""
    import bungee_restatement as RS
    from xrnerf_amd import ops
    sc = restatement_rays(R, S)
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    vd, raw, g = _t(sc['vd'], dev), _t(sc['raw'], dev), _t(sc['g'], dev)
    _, _, z = ops.bungee_zvals(_t(sc['o'], dev), vd, None, None, S + 1, 'sphere', GLOBE, SCALE)
    z64 = t64(z.cpu().numpy())
    for stage, nz in ((0, None), (1, sc['noise']), (2, None), (5, None)):
        noise = None if nz is None else _t(nz, dev)
        rgb, disp, acc, w = [v.cpu().numpy() for v in ops.bungee_render_forward(raw, z, vd, stage, noise=noise)]
        r64 = t64(sc['raw']).requires_grad_(True)
        orgb, odisp, oacc, ow = RS.render(r64, z64, t64(sc['vd']), stage, None if nz is None else t64(nz))
        (orgb * t64(sc['g'])).sum().backward()
        od, og = odisp.detach().numpy(), r64.grad.numpy()
        e_w, e_rgb = np.abs(w - ow.detach().numpy()).max(), np.abs(rgb - orgb.detach().numpy()).max()
        e_acc, e_disp = np.abs(acc - oacc.detach().numpy()).max(), np.abs(disp - od).max()
        graw = ops.bungee_render_backward(raw, z, vd, g, stage, noise=noise).cpu().numpy()
        e_g = np.abs(graw - og).max()
        print('bungee render R=%d S=%d stage=%d: w %.3g rgb %.3g acc %.3g disp %.3g of max %.3g  grad %.3g of max %.3g' % (
            R, S, stage, e_w, e_rgb, e_acc, e_disp, np.abs(od).max(), e_g, np.abs(og).max()))
        assert e_w <= 2e-6
        assert e_rgb <= 1e-5 and e_acc <= 1e-5
        assert e_disp <= 1e-5 * np.abs(od).max()
        assert e_g <= 1e-5 * max(1.0, np.abs(og).max())
        assert (graw[:, :, stage + 1:] == 0).all()


def check_resample(dev, gold):
    from xrnerf_amd import mip
    b = batch(gold, dev)
    data = dict(b, z_vals=_t(gold['sphere_z'], dev), weights=_t(gold['r2_weights'], dev))
    d = mip.resample_along_rays(dict(data), True, 'cone', 0.01, rand=_t(gold['resample_rand'], dev))
    assert np.abs(d['z_vals'].cpu().numpy() - gold['resample_z']).max() <= 5e-5
    d = mip.resample_along_rays(dict(data), False, 'cone', 0.01)
    assert np.abs(d['z_vals'].cpu().numpy() - gold['resample_z_det']).max() <= 5e-5


def loader(d):
    return {k: v[None] for k, v in d.items()}


def check_network(dev, gold):
    """network raw, the stage-1 train_step (loss, psnr, every parameter gradient) against the reference"""
    from conftest import grad_close
    from xrnerf_amd import bungee
    net = build(dev, gold=gold)
    keys = [str(k) for k in gold['keys']]
    assert list(net.state_dict().keys()) == keys
    b = batch(gold, dev)
    b['near'], b['far'], b['z_vals'] = _t(gold['sphere_near'], dev), _t(gold['sphere_far'], dev), _t(gold['sphere_z'], dev)
    d = bungee.sample_along_rays(dict(b), 'cone')
    with torch.no_grad():
        raw = net.mlp(d)['raw']
    assert tuple(raw.shape) == gold['raw'].shape
    assert np.abs(raw.cpu().numpy() - gold['raw']).max() <= 1e-4 * max(1.0, np.abs(gold['raw']).max())
    o = net.train_step(loader(b), None, stage=1, rand=_t(gold['step_rand'], dev))
    assert abs(o['log_vars']['loss'] - float(gold['step_loss'])) <= 1e-4 * float(gold['step_loss'])
    assert abs(o['log_vars']['psnr'] - float(gold['step_psnr'])) <= 1e-3
    o['loss'].backward()
    for k, p in net.named_parameters():
        g = gold['grad/' + k]
        assert p.grad is not None, k
        got = p.grad.cpu().numpy()
        grad_close(got, g, k)
        assert np.abs(got - g).max() <= 1e-3 * np.abs(g).max(), k         # tighter than grad_close's absolute floor
        if k.startswith('mlp.resblocks.1.'):
            assert not got.any(), k                                         # the head above the stage: zero tensors
    return net


def check_stage_loop(dev, gold):
    from xrnerf_amd import bungee
    net = build(dev, gold=gold)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.9, 0.999))
    rands = list(gold['loop_rand'])
    for it in range(3):
        b = batch(gold, dev, 'it%d_' % it)
        b['z_vals'] = _t(gold['it%d_z_vals' % it], dev)
        n = int(b['scale_code'].max()) + 1
        nb = b['rays_o'].shape[0]                 # the third batch is the table's short last one
        outs = bungee.train_iteration(net, loader(b), opt, rands=[_t(r[:nb], dev) for r in rands[:n]])
        rands = rands[n:]
        losses = [o['log_vars']['loss'] for o in outs]
        assert np.allclose(losses, gold['it%d_losses' % it], rtol=1e-4, atol=0), (it, losses)
    # bar: parameters within 1e-4 * max|parameter|.  Adam divides every gradient element by its own running rms, so an element whose
    # gradient is a near-cancelling sum moves by a noticeable fraction of lr on the two sides whenever its few last bits differ: measured
    # on the emulator, 1 entry of 63 084 lies above the bar (8.0e-5 = 0.16 lr; bar 1.8e-5).  Such entries are allowed up to 1e-4 of the
    # parameters and 0.5 lr each -- stated here rather than loosening the bar for all.
    top = max(np.abs(gold['loop/' + k]).max() for k, _ in net.named_parameters())
    over, total = 0, 0
    for k, p in net.named_parameters():
        d = np.abs(p.detach().cpu().numpy() - gold['loop/' + k])
        over, total = over + int((d > 1e-4 * top).sum()), total + d.size
        assert d.max() <= 0.5 * 5e-4, k
    assert over <= 1e-4 * total, (over, total)


def test_zvals_against_reference(dev, gold):
    check_zvals(dev, gold)


def test_encode_against_reference(dev, gold):
    check_encode(dev, gold)


def test_render_against_reference(dev, gold):
    check_render(dev, gold)


@pytest.mark.parametrize('R,S', [(5, 7), (3, 64), (9, 100)])
def test_render_against_restatement_across_sweeps(dev, R, S):
    """a partial block of waves, exactly one 64-interval sweep, two sweeps with a ragged last one"""
    check_render_restatement(dev, R, S)


def test_resample_against_reference(dev, gold):
    check_resample(dev, gold)


def test_network_and_train_step_against_reference(dev, gold):
    check_network(dev, gold)


def test_three_stage_loop_iterations_with_adam(dev, gold):
    check_stage_loop(dev, gold)


def test_config_sizes_against_restatement(dev):
    """netwidth 256, cur_stage 3, 2048 rays x 65 edges: zvals, encoding, MLP, render forward / backward against float64 torch"""
    import bungee_restatement as RS
    from xrnerf_amd import bungee, ops
    torch.manual_seed(0)
    sc = bungee.synthetic_city(H=32, W=40, n_per_scale=4, seed=1)
    table = bungee.BungeeRayTable(sc['H'], sc['W'], sc['focal'], sc['poses'], sc['images'], sc['scale_split'], 2, device=dev)
    b = table.batch(0, 2048)
    d64 = {k: v.double() for k, v in b.items() if k != 'scale_code'}
    near, far, z = ops.bungee_zvals(b['rays_o'], b['viewdirs'], None, None, 65, 'sphere', sc['scene_origin'], sc['scene_scale'])
    n64, f64 = RS.bounds(d64['rays_o'], d64['viewdirs'], 'sphere', sc['scene_origin'], sc['scene_scale'])
    # fp32 cancellation (xr_bungee.hip header): bounded by ~6e-8 * r / (2 h); the scene's lowest cameras sit at 480 m
    assert rel(near.cpu(), n64.cpu()) <= 2e-3 and rel(far.cpu(), f64.cpu()) <= 2e-3
    z64 = RS.zvals(near.double(), far.double(), 65)
    assert rel(z.cpu(), z64.cpu()) <= 1e-6
    means, covs = RS.gaussians(z64, d64['rays_o'], d64['rays_d'], d64['radii'])
    e64 = RS.embed(means, covs, d64['viewdirs'])
    e = ops.bungee_encode(b['viewdirs'], 10, 4, frustum=(b['rays_o'], b['rays_d'], b['radii'], z))
    # sin / cos of arguments up to 512 |x| in fp32: the mean's own rounding (1 ulp of |x| ~ 20) times 2^9 dominates
    assert np.abs(e.cpu().numpy() - e64.cpu().numpy()).max() <= 2e-3
    net = build(dev, 256, 3)
    ref = RS.RestatedMLP(3, 256).double().to(dev)
    ref.load_state_dict({k[4:]: v.double() for k, v in net.state_dict().items() if k.startswith('mlp.')})
    x = e.detach()
    raw = net.mlp.run_mlp(x)
    raw64 = ref(x.double())
    assert rel(raw.detach().cpu(), raw64.detach().cpu()) <= 1e-4
    raw = raw.detach().reshape(2048, 64, 4, 4)
    g = torch.randn(2048, 3, device=dev)
    for st in range(4):
        rgb, disp, acc, w = ops.bungee_render_forward(raw, z, b['viewdirs'], st)
        r64 = raw.double().requires_grad_(True)
        orgb, odisp, oacc, ow = RS.render(r64, z.double(), d64['viewdirs'], st)
        (orgb * g.double()).sum().backward()
        assert np.abs(w.cpu().numpy() - ow.detach().cpu().numpy()).max() <= 2e-6
        assert rel(rgb.cpu(), orgb.detach().cpu()) <= 1e-5 and rel(acc.cpu(), oacc.detach().cpu()) <= 1e-5
        gr = ops.bungee_render_backward(raw, z, b['viewdirs'], g, st)
        assert np.abs(gr.cpu().numpy() - r64.grad.cpu().numpy()).max() <= 1e-5 * r64.grad.abs().max().item()
        assert (gr[:, :, st + 1:] == 0).all()


def test_growth_loads_previous_stage_non_strictly(dev):
    """a stage-0 network's state loaded non-strictly into a stage-1 network: identical rgb when rendered at stage 0"""
    from xrnerf_amd import bungee
    torch.manual_seed(3)
    n0, n1 = build(dev, 64, 0), build(dev, 64, 1)
    missing, unexpected = n1.load_state_dict(n0.state_dict(), strict=False)
    assert not unexpected and all(k.startswith('mlp.resblocks.0.') for k in missing)
    sc = bungee.synthetic_city(H=8, W=10, n_per_scale=2, seed=2)
    b = bungee.BungeeRayTable(sc['H'], sc['W'], sc['focal'], sc['poses'], sc['images'], sc['scale_split'], 2, device=dev).batch(0, 100)
    b = bungee.bungee_zvals(b, 17, 'sphere', sc['scene_origin'], sc['scene_scale'])
    outs = []
    for net in (n0, n1):
        net.render.stage = 0
        with torch.no_grad():
            outs.append(net.forward(dict(b), is_test=True)['rgb'].cpu())
    assert torch.equal(outs[0], outs[1])


def _city_run(dev, n_iter, fused=True, seed=5, netwidth=64, cur_stage=2, n_rays=512, n_z=33):
    import bungee_restatement as RS
    from xrnerf_amd import bungee
    sc = bungee.synthetic_city(H=24, W=32, n_per_scale=3, seed=seed)
    torch.manual_seed(seed)
    table = bungee.BungeeRayTable(sc['H'], sc['W'], sc['focal'], sc['poses'], sc['images'], sc['scale_split'], cur_stage, device=dev)
    torch.manual_seed(seed)
    net = build(dev, netwidth, cur_stage)
    net.mlp.chunk = None
    ref = RS.RestatedNetwork(cur_stage, netwidth, 0.01, n_z).to(dev)
    ref.mlp.load_state_dict({k[4:]: v for k, v in net.state_dict().items() if k.startswith('mlp.')})
    model = net if fused else ref
    opt = torch.optim.Adam(model.parameters(), lr=5e-4, betas=(0.9, 0.999))
    g = torch.Generator(device='cpu').manual_seed(seed)
    n_b = len(table) // n_rays
    hist = []
    for it in range(n_iter):
        b = bungee.bungee_zvals(table.batch(it % n_b, n_rays), n_z, 'sphere', sc['scene_origin'], sc['scene_scale'])
        n = int(b['scale_code'].max()) + 1
        rands = [torch.rand((n_rays, n_z), generator=g).to(dev) for _ in range(n)]
        if fused:
            outs = bungee.train_iteration(net, loader(b), opt, rands=rands)
            hist.append(np.mean([o['log_vars']['loss'] for o in outs]))
        else:
            hist.append(np.mean(RS.train_iteration(ref, b, opt, rands=rands)))
    return net if fused else ref, np.array(hist)


def test_train_iteration_is_reproducible(dev):
    a, _ = _city_run(dev, 2)
    b, _ = _city_run(dev, 2)
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), k


def test_trajectory_against_restatement(dev):
    """200 stage-loop iterations on synthetic_city from the same init, batches and draws: losses within 2 %, and falling"""
    _, hf = _city_run(dev, 200, True)
    _, hr = _city_run(dev, 200, False)
    tail_f, tail_r = hf[-20:].mean(), hr[-20:].mean()
    assert abs(tail_f - tail_r) <= 0.02 * tail_r, (tail_f, tail_r)
    assert tail_f < 0.7 * hf[:10].mean(), (hf[:10].mean(), tail_f)
