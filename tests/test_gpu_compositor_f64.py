"""The compositor kernels -- xr_calc_rgb_forward / _backward / _inference, xr_composite_train in both forms (16 lanes per ray with the
loss accumulator, a wave per ray without), xr_render_slice_select / _composite -- against the float64 reference of
tests/ref64_compositor.py, element by element: |got - ref| <= 2 u e with e the first-order running rounding bound evaluated beside
the reference (derivation there).  Inputs: tests/compositor_cases.py -- rays longer than 128 samples, 64-ray groups wider than the
LDS stage of k_composite_train (its direct path), lengths on both sides of every chunking threshold, empty rays at group starts,
staged and direct workgroups in one launch, planted extremes.  Beside the numbers: rows behind a ray's compacted count stay zero,
the per-segment live counts of both fused forms equal the non-zero rows of that form's own dL/d(raw), xr_live_rows lists exactly
those rows in order, the loss scalars equal the float64 sums over the kernel's own rgb.

WORST collects the worst ratio per (kernel, case) of whatever ran (tools/compositor_f64_bounds.py prints it)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compositor_cases as CC  # noqa: E402
import ref64_compositor as R  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}
COMBOS = [('A', 2, 3), ('A', 3, 3), ('A', 1, 1), ('A', 0, 2), ('B', 2, 3), ('C', 2, 3), ('D', 2, 3), ('E', 2, 3),
          ('B', 0, 2), ('D', 0, 2)]     # logistic density: T stays above 0 along the long rays (background rule, suffix colours behind sample 128)
BG3 = [0.2, 0.5, 0.9]
SLICES = ((0, 16), (16, 64), (64, 2048))


def T(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def means(case):
    """density_grid_mean: both sides of the L1 switch (calc_rgb.cu:104), and exactly 0.01 (off) on case A"""
    return (0.001, 0.5, 0.01) if case == 'A' else (0.001, 0.5)


@functools.lru_cache(maxsize=None)
def walk(case, ra, da):
    c = CC.case(case)
    return R.Walk(CC.raw_for(c, da), c['coords'], c['numsteps'], ra, da)


@functools.lru_cache(maxsize=None)
def forward_ref(case, ra, da):
    c = CC.case(case)
    return walk(case, ra, da).forward(c['numsteps_c'], c['bg'], c['numsteps_c'][:, 0] == c['numsteps'][:, 0])


def hold(kernel, case, ra, da, got, ref, e, what=''):
    r = R.ratio(got, ref, e)
    key = (kernel, case)
    WORST[key] = max(WORST.get(key, 0.0), r)
    print('%-28s %s (%d,%d) %-10s worst |got - ref| / (u e) = %.3f' % (kernel, case, ra, da, what, r))
    assert r <= R.FACTOR, (kernel, case, ra, da, what, r)


def hold_forward(kernel, case, ra, da, rgb):
    F, eF, empty = forward_ref(case, ra, da)
    c = CC.case(case)
    assert np.array_equal(rgb[empty].view(np.uint32), c['bg'][empty].view(np.uint32))      # no samples: the background, bit for bit
    hold(kernel, case, ra, da, rgb, F, eF, 'rgb')


def hold_backward(kernel, case, ra, da, draw, f_tilde, g, mean):
    c = CC.case(case)
    d, e, wr = walk(case, ra, da).backward(c['numsteps_c'], f_tilde, g, mean)
    assert not draw[~wr].any()                                           # rows behind the compacted count: never written
    assert wr.sum() == c['numsteps_c'][:, 0].sum()
    hold(kernel, case, ra, da, draw[wr], d[wr], e[wr], 'mean=%g' % mean)


def inputs(case, da, dev):
    c = CC.case(case)
    t = {k: T(c[k], dev) for k in ('coords', 'numsteps', 'numsteps_c', 'bg', 'target', 'alpha', 'grad')}
    t['raw'] = T(CC.raw_for(c, da), dev)
    return c, t


def mean_t(mean, dev):
    return torch.tensor([mean] + [0.0] * 15, dtype=torch.float32, device=dev)


def separate_kernels(dev, case, ra, da):
    """xr_calc_rgb_forward, xr_calc_rgb_backward (given the float64 colour rounded to fp32, and a random dL/drgb), xr_calc_rgb_inference"""
    from xrnerf_amd import ops
    c, t = inputs(case, da, dev)
    rgb = N(ops.calc_rgb_forward(t['raw'], t['coords'], t['numsteps'], t['numsteps_c'], t['bg'], ra, da))
    hold_forward('xr_calc_rgb_forward', case, ra, da, rgb)
    f_tilde = forward_ref(case, ra, da)[0].astype(np.float32)
    for mean in means(case):
        draw = N(ops.calc_rgb_backward(t['raw'], t['numsteps_c'], t['coords'], t['grad'], T(f_tilde, dev), mean_t(mean, dev), ra, da))
        hold_backward('xr_calc_rgb_backward', case, ra, da, draw, f_tilde, c['grad'], mean)
    # inference: every marched sample, a constant background, always added
    W = walk(case, ra, da)
    rgb, alpha = ops.calc_rgb_inference(t['raw'], t['coords'], t['numsteps'], BG3, ra, da)
    F, eF, empty = W.forward(c['numsteps'], np.array(BG3, np.float32), np.ones(c['n_rays'], bool))
    rgb, alpha = N(rgb), N(alpha)[:, 0]
    assert np.array_equal(rgb[empty], np.tile(np.array(BG3, np.float32), (int(empty.sum()), 1))) and not alpha[empty].any()
    hold('xr_calc_rgb_inference', case, ra, da, rgb, F, eF, 'rgb')
    a, ea = W.alpha_out(c['numsteps'])
    hold('xr_calc_rgb_inference', case, ra, da, alpha, a, ea, 'alpha')


def fused(dev, case, ra, da, wave):
    """xr_composite_train: rgb against the reference, dL/d(raw) against the reference's backward at the kernel's OWN rgb (so the
    forward's error does not leak into the backward's bound), live counts, live-row list, loss scalars"""
    from xrnerf_amd import ops
    c, t = inputs(case, da, dev)
    S = c['S']
    kernel = 'xr_composite_train/wave' if wave else 'xr_composite_train/16-lane'
    for mean in means(case):
        draw = torch.zeros_like(t['raw'])
        lm = None if wave else torch.zeros(2, dtype=torch.float32, device=dev)
        seg = torch.zeros(ops.live_segments(S), dtype=torch.int32, device=dev)
        rgb_t = ops.composite_train(t['raw'], t['coords'], t['numsteps'], t['numsteps_c'], t['bg'], t['target'], t['alpha'], mean_t(mean, dev),
                                    ra, da, lm, draw, live_seg=seg)
        rows, n_live = ops.live_rows(draw, S, seg_counts=seg)
        if wave:
            lm = ops.train_loss_scalars(rgb_t, t['target'], t['alpha'], 0.1, 5.0)
        rgb, d, rows, nl, seg, lm = N(rgb_t), N(draw), N(rows), int(n_live[0]), N(seg), N(lm)
        hold_forward(kernel, case, ra, da, rgb)
        hold_backward(kernel, case, ra, da, d, rgb, R.huber_grad(rgb, c['target']), mean)
        live = (d != 0).any(1)
        assert seg.tolist() == [int(live[k:k + 1024].sum()) for k in range(0, S, 1024)]
        assert nl == int(live.sum()) and np.array_equal(rows[:nl], np.nonzero(live)[0])
        ref_lm = R.loss_scalars(rgb, c['target'], c['alpha'])
        assert np.allclose(lm, ref_lm, rtol=1e-5, atol=0), (lm, ref_lm)


def slices(dev, case, ra=2, da=3):
    """xr_render_slice_select + xr_render_slice_composite over depth slices with eps = 0: the full composite of every marched sample"""
    from xrnerf_amd import ops
    c, t = inputs(case, da, dev)
    n, S = c['n_rays'], c['S']
    Tr = torch.ones((n,), dtype=torch.float32, device=dev)
    acc = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    ray_off = torch.empty((n,), dtype=torch.int32, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    rows = torch.zeros((S,), dtype=torch.int32, device=dev)
    nf, reached = c['numsteps'][:, 0], []
    for s0, s1 in SLICES:
        ops.render_slice_select(t['numsteps'], Tr, s0, s1, 0.0, rows, ray_off, count)
        m = int(count.item())
        want = np.minimum(nf, s1) - s0
        assert m == int(want[(nf > s0) & (N(Tr) > 0)].sum())
        reached.append(m)
        if m == 0:                # every longer ray is at T == 0 exactly (what render_rays_ert does: nothing left to evaluate)
            break
        raw_s = t['raw'][rows[:m].long()].contiguous()
        ops.render_slice_composite(raw_s, t['coords'], t['numsteps'], ray_off, s0, s1, ra, da, Tr, acc)
    print('rows per slice:', reached)
    assert len(reached) >= 2 and reached[0] > 0 and reached[1] > 0        # the per-ray state is carried across a slice boundary
    if da == R.LOGISTIC:              # density <= 1: no T reaches 0, so the last slice holds every sample from the 64th on
        assert reached[2] == int(np.maximum(nf - 64, 0).sum()) > 0
    C, eC, Tn, eTn, empty = walk(case, ra, da).ends(c['numsteps'])
    acc, Tr = N(acc), N(Tr)
    assert not acc[empty].any() and (Tr[empty] == 1).all()
    hold('xr_render_slice_composite', case, ra, da, acc, C, eC + np.abs(C), 'rgb_acc')
    hold('xr_render_slice_composite', case, ra, da, Tr, Tn, eTn, 'T')


@pytest.mark.parametrize('case,ra,da', COMBOS)
def test_forward_backward_inference_against_float64(dev, case, ra, da):
    separate_kernels(dev, case, ra, da)


@pytest.mark.parametrize('case,ra,da', COMBOS)
def test_fused_16_lane_form_against_float64(dev, case, ra, da):
    fused(dev, case, ra, da, wave=False)


@pytest.mark.parametrize('case,ra,da', COMBOS)
def test_fused_wave_per_ray_form_against_float64(dev, case, ra, da):
    fused(dev, case, ra, da, wave=True)


@pytest.mark.parametrize('case', ['A', 'B'])
def test_depth_slices_equal_the_full_composite(dev, case):
    """(2, 3): the exponential density has every ray of these inputs at T == 0 exactly before its 64th sample -- the last slice selects
    nothing; (0, 2): the logistic density keeps every ray alive through all three slices"""
    slices(dev, case, 2, 3)
    slices(dev, case, 0, 2)
