"""Vanilla NeRF (BASELINE config #1) on the device: the kernels of xrnerf_amd/csrc/xr_vanilla.hip (xr_nerf_encode, xr_nerf_render_train_forward,
xr_nerf_render_backward, xr_nerf_sample_pdf) against the float64 restatement (tests/vanilla_restatement.py), and the registry modules of
xrnerf_amd/vanilla.py over them against one training step of the reference's own modules (tests/golden/ref_vanilla_train.npz).

The bodies are `check_*(dev, ...)` functions: tests/test_emu_vanilla.py runs the same bodies on the CPU through the HIP-on-CPU shim.

Bars.  Encode 1e-6 absolute (p 2^k is exact, sinf / cosf ~2 ulp of a value <= 1).  Renderer: weights 2e-6, rgb / acc / disp
1e-5 max(1, |ref|), backward 1e-5 max|ref| (the bars of test_gpu_mip.py / test_gpu_bungee.py for the same stages).  Resampling: the
reference algorithm is discontinuous at its `denom < 1e-5 -> 1` rule (almost-empty bins of an opaque ray sit inside fp32 rounding of the
threshold), so no plain bar on z can hold; checked instead: (a) every sample inverts the float64 cdf to 1.2e-5 (the 1e-5 the rule grants
plus fp32 cdf rounding), (b) samples whose float64 bin has denom >= 1e-3 agree with the float64 samples to 5e-5, and those are at
least 75 % of every case, (c) the merge is a bit-exact sort and pts = o + d z un-fused, (d) sizes out of range return -22."""
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

SHAPES = [(1, 3), (5, 7), (3, 64), (9, 100), (66, 16), (130, 192)]
RESAMPLE = [(3, 1), (5, 7), (16, 24), (64, 128), (100, 200)]
MCFG = dict(skips=[2], netdepth=4, netwidth=32, output_ch=5, use_viewdirs=True, netchunk=1024 * 32,
            embedder=dict(type='BaseEmbedder', i_embed=0, multires=10, multires_dirs=4))


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_vanilla_train.npz'))


def _dt(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


_SCENES = {}


def scene(R, S):
    """rays, sorted sample positions and raw [R,S,4] whose density is a Gaussian blob of random depth and width times a scale of
    {0.05, 1, 30}, minus 2 % of that scale.  Ray 1: density <= 0 everywhere (0 at the even samples); ray 2: opaque at its first sample
    (raw_3 = 50); ray 3: two equal sample positions.  Computed once per shape and shared."""
    if (R, S) in _SCENES:
        return _SCENES[(R, S)]
    rng = np.random.default_rng(1000 * R + S)
    o = (rng.normal(0, 0.1, (R, 3)) + [0, 0, 4]).astype(np.float32)
    d = rng.normal(0, 0.2, (R, 3)) - [0, 0, 1]
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.7, 1.5, (R, 1))).astype(np.float32)
    edges = np.linspace(2.0, 6.0, S + 1)
    z = (edges[:-1] + (edges[1:] - edges[:-1]) * rng.uniform(0.05, 0.95, (R, S))).astype(np.float32)
    raw = rng.normal(0, 1.5, (R, S, 4)).astype(np.float32)
    c, wd = rng.uniform(2.5, 5.5, (R, 1)), rng.uniform(0.1, 0.8, (R, 1))
    scale = np.array([0.05, 1.0, 30.0])[np.arange(R) % 3][:, None]
    raw[..., 3] = scale * (np.exp(-0.5 * ((z - c) / wd) ** 2) - 0.02)
    if R > 1:
        raw[1, :, 3] = np.where(np.arange(S) % 2 == 0, 0.0, -1.0)
    if R > 2:
        raw[2, 0, 3] = 50.0
    if R > 3:
        z[3, 1] = z[3, 0]
    noise = rng.normal(0, 1, (R, S)).astype(np.float32)
    g = rng.normal(0, 1, (R, 3)).astype(np.float32)
    _SCENES[(R, S)] = dict(o=o, d=d, z=z, raw=raw, noise=noise, g=g)
    return _SCENES[(R, S)]


# ------------------------------------------------------------------------------------------ kernels against the restatement
def check_encode(dev, R, S):
    import vanilla_restatement as RS
    from xrnerf_amd import ops
    rng = np.random.default_rng(7 * R + S)
    pts = rng.uniform(-6, 6, (R, S, 3)).astype(np.float32)              # arguments up to 2^9 * 6
    dirs = rng.normal(0, 1, (R, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)
    L, Ld, ch = 10, 4, 90
    buf = torch.full((R * S, 96), float('nan'), dtype=torch.float32, device=dev)
    e = ops.nerf_encode(_dt(pts, dev), _dt(dirs, dev), L, Ld, out=buf)
    assert tuple(e.shape) == (R * S, ch)
    want = RS.embed(pts.reshape(-1, 3), np.repeat(dirs, S, axis=0), L, Ld).numpy()
    err = np.abs(_np(e).astype(np.float64) - want).max()
    print('encode R=%d S=%d max err %.3g' % (R, S, err))
    assert err <= 1e-6
    assert (_np(buf)[:, ch:] == 0).all()                                # the padding is WRITTEN as zeros
    # the default output: rows padded to a multiple of 4 floats; one direction per row gives the same bits
    e1 = ops.nerf_encode(_dt(pts, dev), _dt(dirs, dev), L, Ld)
    assert e1.stride(0) == 92 and torch.equal(e1, e)
    e2 = ops.nerf_encode(_dt(pts.reshape(-1, 3), dev), _dt(np.repeat(dirs, S, axis=0), dev), L, Ld)
    assert torch.equal(e2, e)
    # other frequency counts (another row width, no padding columns at ch = 12 + ...): multires 1 / 0
    e3 = ops.nerf_encode(_dt(pts, dev), _dt(dirs, dev), 1, 0)
    assert np.abs(_np(e3) - RS.embed(pts.reshape(-1, 3), np.repeat(dirs, S, axis=0), 1, 0).numpy()).max() <= 1e-6


def check_render(dev, R, S):
    import vanilla_restatement as RS
    from xrnerf_amd import ops
    sc = scene(R, S)
    raw, z, d = _dt(sc['raw'], dev), _dt(sc['z'], dev), _dt(sc['d'], dev)
    g = _dt(sc['g'], dev)
    first = True
    for white in (False, True):
        for noise in (None, sc['noise']):
            nz = None if noise is None else _dt(noise, dev)
            rgb, disp, acc, w = ops.nerf_render_train_forward(raw, z, d, white, nz)
            r64 = RS.t64(sc['raw']).requires_grad_(True)
            o_rgb, o_disp, o_acc, o_w = RS.render(r64, RS.t64(sc['z']), RS.t64(sc['d']), white, None if noise is None else RS.t64(noise))
            (o_rgb * RS.t64(sc['g'])).sum().backward()
            o_rgb, o_disp, o_acc, o_w = [t.detach().numpy() for t in (o_rgb, o_disp, o_acc, o_w)]
            e_w = np.abs(_np(w) - o_w).max()
            e_rgb = (np.abs(_np(rgb) - o_rgb) / np.maximum(1, np.abs(o_rgb))).max()
            e_acc = (np.abs(_np(acc) - o_acc) / np.maximum(1, np.abs(o_acc))).max()
            assert e_w <= 2e-6 and e_rgb <= 1e-5 and e_acc <= 1e-5, (white, noise is not None, e_w, e_rgb, e_acc)
            dn = _np(disp)
            assert (np.isfinite(dn) == np.isfinite(o_disp)).all()       # the all-transparent ray: 0 / 0 on both sides
            m = (o_acc > 1e-3) & np.isfinite(o_disp)
            if m.any():
                assert (np.abs(dn[m] - o_disp[m]) / np.maximum(1, np.abs(o_disp[m]))).max() <= 1e-5
            graw = ops.nerf_render_backward(raw, z, d, g, white, nz)
            og = r64.grad.numpy()
            e_g = np.abs(_np(graw) - og).max()
            print('render R=%d S=%d white=%d noise=%d: w %.3g rgb %.3g acc %.3g  grad %.3g of max %.3g' % (
                R, S, white, noise is not None, e_w, e_rgb, e_acc, e_g, np.abs(og).max()))
            assert np.isfinite(_np(graw)).all() and e_g <= 1e-5 * np.abs(og).max()
            if noise is None:
                # the inference kernel (k_nerf_render, xr_kilo.hip) is the same arithmetic: the same bits
                i_rgb, _, i_acc, i_w = ops.nerf_render_forward(raw, z, d, white)
                assert torch.equal(i_w, w) and torch.equal(i_rgb, rgb) and torch.equal(i_acc, acc)
            if first:
                # the same bits on a second launch, forward and backward
                again = ops.nerf_render_train_forward(raw, z, d, white, nz)
                for a, b in zip((rgb, acc, w), (again[0], again[2], again[3])):
                    assert torch.equal(a, b)
                assert np.array_equal(_np(again[1]), dn, equal_nan=True)
                assert torch.equal(ops.nerf_render_backward(raw, z, d, g, white, nz), graw)
                first = False


def _inversion_checks(z, w, u, zs, what):
    """(a) and (b) of the module docstring; z, w, u, zs: float32 numpy"""
    import vanilla_restatement as RS
    z64, w64, u64 = RS.t64(z), RS.t64(w), RS.t64(u)
    Fz = RS.cdf_at(z64, w64, RS.t64(zs)).numpy()
    e_a = np.abs(Fz - u64.numpy()).max()
    want, denom = RS.sample_pdf(z64, w64, u64)
    m = denom.numpy() >= 1e-3
    e_b = np.abs(zs.astype(np.float64) - want.numpy())[m].max() if m.any() else 0.0
    print('%s: |F(z) - u| %.3g; |z - z64| %.3g on %.1f %% of the samples' % (what, e_a, e_b, 100 * m.mean()))
    assert np.isfinite(zs).all()
    assert e_a <= 1.2e-5, what
    assert e_b <= 5e-5, what
    assert m.mean() >= 0.75, what


def check_resample(dev, S, N):
    import vanilla_restatement as RS
    from xrnerf_amd import ops
    R = 13
    sc = scene(R, S)
    w64 = RS.render(RS.t64(sc['raw']), RS.t64(sc['z']), RS.t64(sc['d']), False)[3]
    w = w64.numpy().astype(np.float32)
    w[4] = 0.0                                                          # a ray with all-zero weights (ray 1 has none either)
    z, o, d = _dt(sc['z'], dev), _dt(sc['o'], dev), _dt(sc['d'], dev)
    wt = _dt(w, dev)
    u = np.random.default_rng(S * 31 + N).uniform(0, 1, (R, N)).astype(np.float32)
    lin = torch.linspace(0., 1., N, device=dev).expand(R, N).contiguous()
    for name, ut in (('random u', _dt(u, dev)), ('linspace u', lin)):
        z_all, pts, zs = ops.nerf_sample_pdf(z, wt, o, d, N, ut, want_samples=True)
        assert tuple(z_all.shape) == (R, S + N) and tuple(pts.shape) == (R, S + N, 3) and tuple(zs.shape) == (R, N)
        _inversion_checks(sc['z'], w, _np(ut), _np(zs), 'S=%d N=%d %s' % (S, N, name))
        # (c) the merge
        assert torch.equal(z_all, torch.sort(torch.cat([z, zs], -1), -1)[0])
        assert bool((z_all[:, 1:] >= z_all[:, :-1]).all())
        assert torch.equal(pts, o[:, None, :] + d[:, None, :] * z_all[:, :, None])
        # z_samples_out is optional
        z2, p2 = ops.nerf_sample_pdf(z, wt, o, d, N, ut)
        assert torch.equal(z2, z_all) and torch.equal(p2, pts)
    # u = NULL is linspace(0, 1, N), bit for bit
    z3, p3, zs3 = ops.nerf_sample_pdf(z, wt, o, d, N, None, want_samples=True)
    assert torch.equal(z3, z_all) and torch.equal(p3, pts) and torch.equal(zs3, zs)


def check_resample_size_limits(dev):
    """(d): sizes outside 3 <= S <= 1024, 1 <= N <= 1024 are refused with -22 and a message; the limits themselves run"""
    from xrnerf_amd import _lib, ops
    for S, N in ((2, 4), (1025, 4), (8, 1025), (8, 0)):
        z = torch.linspace(2., 6., S, device=dev).expand(2, S).contiguous()
        o = torch.zeros((2, 3), device=dev)
        with pytest.raises(_lib.XrError, match=r'\(-22\).*sample count'):
            ops.nerf_sample_pdf(z, torch.ones_like(z), o, o + 1, N)
    S = N = 1024
    z = torch.linspace(2., 6., S, device=dev).expand(2, S).contiguous()
    o = torch.zeros((2, 3), device=dev)
    z_all, _, zs = ops.nerf_sample_pdf(z, torch.ones_like(z), o, o + 1, N, None, want_samples=True)
    assert torch.equal(z_all, torch.sort(torch.cat([z, zs], -1), -1)[0])
    # uniform weights: the cdf is linear between the first and the last bin midpoint
    assert np.abs(_np(zs)[0] - np.interp(np.linspace(0, 1, N), [0, 1], [_np(z)[0, :2].mean(), _np(z)[0, -2:].mean()])).max() <= 5e-5


@pytest.mark.parametrize('R,S', SHAPES)
def test_encode_against_float64(dev, R, S):
    check_encode(dev, R, S)


@pytest.mark.parametrize('R,S', SHAPES)
def test_render_forward_and_backward_against_float64_autograd(dev, R, S):
    check_render(dev, R, S)


@pytest.mark.parametrize('S,N', RESAMPLE)
def test_resampling_inverts_the_cdf_and_merges_exactly(dev, S, N):
    check_resample(dev, S, N)


def test_resampling_size_limits(dev):
    check_resample_size_limits(dev)


# ------------------------------------------------------------------------------------------ the reference's training step
def _modules(dev, gold):
    from xrnerf_amd import builder
    import xrnerf_amd  # noqa: F401  (registers the modules)
    mlp = builder.build_mlp(dict(type='NerfMLP', **copy.deepcopy(MCFG)))
    fine = builder.build_mlp(dict(type='NerfMLP', **copy.deepcopy(MCFG)))
    mlp.load_state_dict({k[len('sd_coarse.'):]: torch.tensor(gold[k]) for k in gold.files if k.startswith('sd_coarse.')}, strict=True)
    fine.load_state_dict({k[len('sd_fine.'):]: torch.tensor(gold[k]) for k in gold.files if k.startswith('sd_fine.')}, strict=True)
    render = builder.build_render(dict(type='NerfRender', white_bkgd=True, raw_noise_std=0))
    return mlp.to(dev), fine.to(dev), render


def _step(dev, gold, mlp, fine, render, fine_z=None):
    """the fixture's training step through the modules, with the recorded draws -> everything the fixture records.  fine_z: sample
    positions for the fine pass in place of the resampler's own (the reference's, so that the fine pass can be compared value by value:
    two correct fp32 resamplers differ by a few ulp of z, which the 2^9 frequency of the encoding turns into 1e-3 of a feature)"""
    from xrnerf_amd import vanilla
    for m in (mlp, fine):
        for p in m.parameters():
            p.grad = None
    rays_o, rays_d, z = _dt(gold['rays_o'], dev), _dt(gold['rays_d'], dev), _dt(gold['z_vals'], dev)
    tgt = _dt(gold['target'], dev)
    data = {'pts': vanilla.get_pts(rays_o, rays_d, z), 'viewdirs': _dt(gold['viewdirs'], dev), 'z_vals': z, 'rays_o': rays_o,
            'rays_d': rays_d}
    out = {}
    data = mlp(data)
    raw_c = data['raw']
    raw_c.retain_grad()
    data, ret = render(data, False)
    out['coarse_raw'], out['coarse_weights'] = raw_c, data['weights']
    data = vanilla.sample_pdf(data, gold['u'].shape[1], True, False, u=_dt(gold['u'], dev))
    out['fine_z'] = data['z_vals']
    if fine_z is not None:
        data['z_vals'], data['pts'] = fine_z, vanilla.get_pts(rays_o, rays_d, fine_z)
    data = fine(data)
    raw_f = data['raw']
    raw_f.retain_grad()
    data, fret = render(data, False)
    out['fine_raw'], out['fine_weights'] = raw_f, data['weights']
    for k in ('rgb', 'disp', 'acc'):
        out['coarse_' + k], out['fine_' + k] = ret[k], fret[k]
    loss = vanilla.img2mse(fret['rgb'], tgt) + vanilla.img2mse(ret['rgb'], tgt)
    loss.backward()
    out['loss'] = loss.detach()
    out['d_coarse_raw'], out['d_fine_raw'] = raw_c.grad, raw_f.grad
    return out


def check_fixture_step(dev, gold, repeat=False):
    """one training step of the reference's own modules (tests/golden/ref_vanilla_train.npz) through the registry's modules with the
    reference's state dicts and draws.  The chain at the resampler's own samples: coarse pass, renders, loss, and the resampler's
    (a) / (b) / merge checks.  Then the same step with the fine pass at the reference's fine samples: fine raw / weights / renders, the
    loss, dL/draw of both passes (1e-5 max) and every parameter gradient (2e-4 max(1e-3, |ref|max) + 1e-7, Mip-NeRF's network bar)."""
    from xrnerf_amd import ops
    mlp, fine, render = _modules(dev, gold)

    def close(out, key, bar, rel=True):
        got, ref = _np(out[key]).astype(np.float64), gold[key].astype(np.float64)
        err = np.abs(got - ref) / (np.maximum(1, np.abs(ref)) if rel else 1.0)
        print('%s: %.3g (bar %.3g)' % (key, err.max(), bar))
        assert got.shape == ref.shape and err.max() <= bar, key

    # ---- the whole chain, the fine pass at the resampler's own samples
    out = _step(dev, gold, mlp, fine, render)
    close(out, 'coarse_raw', 1e-5, rel=False)
    close(out, 'coarse_weights', 2e-6, rel=False)
    for k in ('coarse_rgb', 'coarse_acc', 'coarse_disp', 'fine_rgb', 'fine_acc', 'fine_disp'):
        close(out, k, 1e-5)
    loss, ref = float(out['loss']), float(gold['loss'][0])
    print('loss %.9g against %.9g' % (loss, ref))
    assert abs(loss - ref) <= 1e-5 * max(1.0, abs(ref))
    # the resampler on the reference's own coarse pass: (a), (b) and the merge
    z, w = _dt(gold['z_vals'], dev), _dt(gold['coarse_weights'], dev)
    z_all, _, zs = ops.nerf_sample_pdf(z, w, _dt(gold['rays_o'], dev), _dt(gold['rays_d'], dev), gold['u'].shape[1], _dt(gold['u'], dev),
                                       want_samples=True)
    _inversion_checks(gold['z_vals'], gold['coarse_weights'], gold['u'], _np(zs), 'fixture')
    assert torch.equal(z_all, torch.sort(torch.cat([z, zs], -1), -1)[0])
    print('z_samples against the reference\'s fp32 samples: %.3g' % np.abs(_np(zs) - gold['z_samples']).max())

    # ---- the same step with the fine pass at the reference's samples: every value and every gradient
    out = _step(dev, gold, mlp, fine, render, fine_z=_dt(gold['fine_z'], dev))
    close(out, 'fine_raw', 1e-5, rel=False)
    close(out, 'fine_weights', 2e-6, rel=False)
    for k in ('fine_rgb', 'fine_acc', 'fine_disp'):
        close(out, k, 1e-5)
    loss = float(out['loss'])
    assert abs(loss - ref) <= 1e-5 * max(1.0, abs(ref))
    for k in ('d_coarse_raw', 'd_fine_raw'):
        got, want = _np(out[k]).astype(np.float64), gold[k].astype(np.float64)
        print('%s: %.3g of max %.3g' % (k, np.abs(got - want).max(), np.abs(want).max()))
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), k
    worst = (0.0, '')
    for name, m in (('grad_coarse.', mlp), ('grad_fine.', fine)):
        for k, p in m.named_parameters():
            want = gold[name + k].astype(np.float64)
            assert p.grad is not None and tuple(p.grad.shape) == want.shape, name + k
            err, bar = np.abs(_np(p.grad) - want).max(), 2e-4 * max(1e-3, np.abs(want).max()) + 1e-7
            worst = max(worst, (err / bar, name + k))
            assert err <= bar, (name + k, err, np.abs(want).max())
    print('parameter gradients: worst error / bar %.3g (%s)' % worst)
    if repeat:                                             # (check_repeatable with this step as the first of the two)
        first = [out['loss'].clone()] + [p.grad.clone() for m in (mlp, fine) for p in m.parameters()]
        out = _step(dev, gold, mlp, fine, render, fine_z=_dt(gold['fine_z'], dev))
        for a, b in zip(first, [out['loss']] + [p.grad for m in (mlp, fine) for p in m.parameters()]):
            assert torch.equal(a, b)
    # the second render case: raw_noise_std = 1 with the recorded draw
    raw, z, d = _dt(gold['coarse_raw'], dev), _dt(gold['z_vals'], dev), _dt(gold['rays_d'], dev)
    nz = _dt(gold['noise'], dev)
    rgb, disp, acc, w = ops.nerf_render_train_forward(raw, z, d, True, nz)
    assert np.abs(_np(w) - gold['noisy_weights']).max() <= 2e-6
    for got, k in ((rgb, 'rgb'), (acc, 'acc'), (disp, 'disp')):
        ref = gold['noisy_' + k]
        assert (np.abs(_np(got) - ref) / np.maximum(1, np.abs(ref))).max() <= 1e-5, k
    graw = ops.nerf_render_backward(raw, z, d, _dt(gold['noisy_g_rgb'], dev), True, nz)
    assert np.abs(_np(graw) - gold['noisy_d_raw']).max() <= 1e-5 * np.abs(gold['noisy_d_raw']).max()


def check_repeatable(dev, gold):
    """two identical training steps from the same state and draws: the same bits in the loss and in every parameter gradient"""
    mlp, fine, render = _modules(dev, gold)
    runs = []
    for _ in range(2):
        out = _step(dev, gold, mlp, fine, render)
        runs.append([out['loss'].clone()] + [p.grad.clone() for m in (mlp, fine) for p in m.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def small_network(dev, seed=0):
    import xrnerf_amd
    cfg = json.load(open(os.path.join(G, 'ngp_model_cfg.json')))['vanilla_model']
    for k in ('mlp', 'mlp_fine'):
        cfg[k].update(netdepth=4, netwidth=32, skips=[2])
    cfg['cfg']['N_importance'] = 24
    torch.manual_seed(seed)
    return xrnerf_amd.build_network(cfg).to(dev)


def check_path_taken(dev, gold):
    """a training step of the registry's NerfNetwork issues the vanilla kernels: encode, one MLP node, render forward / backward,
    resampling, and the same for the fine network"""
    from xrnerf_amd import ops, vanilla
    names = ('nerf_encode', 'nerf_render_train_forward', 'nerf_render_backward', 'nerf_sample_pdf')
    saved = {n: getattr(ops, n) for n in names}
    calls = []

    def wrap(n):
        def f(*a, **k):
            calls.append(n)
            return saved[n](*a, **k)
        return f
    net = small_network(dev)
    rays_o, rays_d, z = _dt(gold['rays_o'], dev), _dt(gold['rays_d'], dev), _dt(gold['z_vals'], dev)
    batch = {'rays_o': rays_o[None], 'rays_d': rays_d[None], 'viewdirs': _dt(gold['viewdirs'], dev)[None], 'z_vals': z[None],
             'pts': vanilla.get_pts(rays_o, rays_d, z)[None], 'target_s': _dt(gold['target'], dev)[None]}
    nodes = []
    apply = vanilla._NerfMlpFn.apply
    try:
        for n in names:
            setattr(ops, n, wrap(n))
        vanilla._NerfMlpFn.apply = staticmethod(lambda *a: (nodes.append(1), apply(*a))[1])
        out = net.train_step(batch, None)
        out['loss'].backward()
    finally:
        for n in names:
            setattr(ops, n, saved[n])
        del vanilla._NerfMlpFn.apply                       # back to the inherited classmethod
    assert calls == ['nerf_encode', 'nerf_render_train_forward', 'nerf_sample_pdf', 'nerf_encode', 'nerf_render_train_forward',
                     'nerf_render_backward', 'nerf_render_backward'], calls
    assert len(nodes) == 2
    assert np.isfinite(out['log_vars']['loss'])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


def check_full_config(dev, n_rays):
    """config #1's own widths (8 x 256, 63 + 27 channels, skip at 4): run_mlp is ONE autograd node on the embedder's padded rows and equals
    the layer-by-layer float64 graph (bars of test_gpu_linear.py's whole-MLP test); an input that requires a gradient takes the per-layer
    path and gets it"""
    from conftest import grad_close
    from xrnerf_amd import builder
    import xrnerf_amd  # noqa: F401
    cfg = json.load(open(os.path.join(G, 'ngp_model_cfg.json')))['vanilla_model']['mlp']
    torch.manual_seed(5)
    mlp = builder.build_mlp(cfg).to(dev)
    assert (mlp.input_ch, mlp.input_ch_dirs) == (63, 27) and mlp.skips == [4] and len(mlp.pts_linears) == 8
    ref = copy.deepcopy(mlp).double().cpu()
    S = 3
    pts = torch.randn(n_rays, S, 3) * 1.5
    dirs = torch.nn.functional.normalize(torch.randn(n_rays, 3), dim=-1)
    data = mlp.embedder({'pts': pts.to(dev), 'viewdirs': dirs.to(dev)})
    x = data['embedded']
    assert tuple(x.shape) == (n_rays * S, 90) and x.stride(0) == 92          # the kernel's padded rows
    assert mlp._device_graph_ok(x)
    M = x.shape[0]
    g = torch.randn(M, 4, dtype=torch.float64)
    out = mlp.run_mlp(x)
    assert out.grad_fn is not None and type(out.grad_fn).__name__ == '_NerfMlpFnBackward'
    out.backward(g.float().to(dev))
    x64 = x.detach().cpu().double().requires_grad_(True)
    want = ref.run_mlp(x64)
    want.backward(g)
    assert (out.detach().cpu().double() - want.detach()).abs().max() <= 1e-4 * max(1.0, float(want.detach().abs().max()))
    for (name, p), (_, q) in zip(mlp.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and p.grad.shape == q.grad.shape, name
        grad_close(p.grad.cpu().numpy(), q.grad.numpy(), name, kinks=True)
    # an input that requires a gradient: the per-layer graph, which provides it
    x2 = x.detach().clone().requires_grad_(True)
    assert not mlp._device_graph_ok(x2)
    out2 = mlp.run_mlp(x2)
    assert type(out2.grad_fn).__name__ != '_NerfMlpFnBackward'
    out2.backward(g.float().to(dev))
    assert x2.grad is not None
    grad_close(x2.grad.cpu().numpy(), x64.grad.numpy(), 'input gradient', kinks=True)
    # the node itself refuses to drop an input gradient silently
    from xrnerf_amd import _lib, vanilla
    params = []
    for layer in mlp.pts_linears:
        params += [layer.weight, layer.bias]
    v = mlp.views_linears[0]
    params += [v.weight, v.bias, mlp.feature_linear.weight, mlp.feature_linear.bias, mlp.alpha_linear.weight, mlp.alpha_linear.bias,
               mlp.rgb_linear.weight, mlp.rgb_linear.bias]
    x3 = x.detach().clone().requires_grad_(True)
    out3 = vanilla._NerfMlpFn.apply(x3, (4,), 63, 27, *params)
    with pytest.raises(_lib.XrError, match='no gradient with respect to its input'):
        out3.backward(g.float().to(dev))


def blob_targets(rays_o, rays_d, near=2.0, far=6.0, n=96):
    """a fixed synthetic scene: a coloured Gaussian blob at the origin, rendered by the float64 restatement on a white background"""
    import vanilla_restatement as RS
    o, d = RS.t64(rays_o), RS.t64(rays_d)
    z = torch.linspace(near, far, n, dtype=torch.float64).expand(o.shape[0], n)
    p = o[:, None, :] + d[:, None, :] * z[..., None]
    sigma = 6.0 * torch.exp(-0.5 * (p ** 2).sum(-1) / 0.6 ** 2)
    col = 0.5 + 0.45 * torch.sin(p * torch.tensor([1.5, 2.0, 2.5], dtype=torch.float64) + torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64))
    raw = torch.cat([torch.log(col / (1 - col)), sigma[..., None]], -1)
    return RS.render(raw, z, d, True)[0].float()


def check_convergence(dev, steps=200):
    from xrnerf_amd import vanilla
    net = small_network(dev, seed=1)
    net.is_perturb = True
    g = torch.Generator().manual_seed(3)
    n = 512
    cam = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 4.0
    rays_d = torch.nn.functional.normalize(-cam + torch.randn(n, 3, generator=g) * 0.6, dim=-1)
    tgt = blob_targets(cam, rays_d).to(dev)
    rays_o, rays_d = cam.to(dev), rays_d.to(dev)
    z = vanilla.get_z_vals(rays_o, 2., 6., 16)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    losses = []
    for _ in range(steps):
        zz = vanilla.perturb_z_vals(z)                                         # drawn on the device
        data = {'rays_o': rays_o, 'rays_d': rays_d, 'viewdirs': rays_d, 'z_vals': zz, 'pts': vanilla.get_pts(rays_o, rays_d, zz)}
        ret = net.forward(data, is_test=False)
        loss = vanilla.img2mse(ret['rgb'], tgt) + vanilla.img2mse(ret['coarse_rgb'], tgt)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    means = torch.stack(losses).reshape(-1, 20).mean(1).cpu().numpy()
    print('20-step loss means:', ' '.join('%.4g' % v for v in means))
    assert np.isfinite(means).all()
    assert (means[1:] < means[:-1]).all(), means
    assert means[-1] < 0.25 * means[0], means


def test_one_training_step_against_the_reference_fixture(dev, gold):
    check_fixture_step(dev, gold)


def test_training_step_issues_the_vanilla_kernels(dev, gold):
    check_path_taken(dev, gold)


def test_two_identical_steps_give_the_same_bits(dev, gold):
    check_repeatable(dev, gold)


def test_config1_mlp_is_one_node_and_equals_the_layer_by_layer_graph(dev):
    check_full_config(dev, 256)


def test_small_network_converges_on_a_synthetic_blob(dev):
    check_convergence(dev)
