"""Worst |got - ref| / (u e) of the compositor kernels against tests/ref64_compositor.py, per kernel and per case of
tests/compositor_cases.py (the table of profiles/compositor_f64_bounds.txt):

    python tools/compositor_f64_bounds.py gpu      the library on the GPU
    python tools/compositor_f64_bounds.py emu      the kernels' sources on the host (tests/hip_emu)
    python tools/compositor_f64_bounds.py oracle   the sequential fp32 oracle (oracle.calc_rgb_*), computed the same way

Runs the bodies of tests/test_gpu_compositor_f64.py on every case (A..E), i.e. it fails where they fail."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('tests/hip_emu', 'tests', 'oracle', ''):
    sys.path.insert(0, os.path.join(ROOT, p))
import compositor_cases as CC  # noqa: E402
import ref64_compositor as R  # noqa: E402
import test_gpu_compositor_f64 as G  # noqa: E402


def run_kernels(dev):
    for case, ra, da in G.COMBOS:
        G.separate_kernels(dev, case, ra, da)
        G.fused(dev, case, ra, da, wave=False)
        G.fused(dev, case, ra, da, wave=True)
    for case in ('A', 'B'):
        G.slices(dev, case, 2, 3)
        G.slices(dev, case, 0, 2)


def run_oracle():
    import oracle as O
    for case, ra, da in G.COMBOS:
        c = CC.case(case)
        raw = CC.raw_for(c, da)
        rgb = O.calc_rgb_forward(raw, c['coords'], c['numsteps'], c['numsteps_c'], c['bg'], ra, da)
        G.hold_forward('xr_calc_rgb_forward', case, ra, da, rgb)
        f_tilde = G.forward_ref(case, ra, da)[0].astype(np.float32)
        for mean in G.means(case):
            draw = O.calc_rgb_backward(raw, c['numsteps_c'], c['coords'], c['grad'], f_tilde, mean, ra, da)
            G.hold_backward('xr_calc_rgb_backward', case, ra, da, draw, f_tilde, c['grad'], mean)
        W = G.walk(case, ra, da)
        rgb, alpha = O.calc_rgb_inference(raw, c['coords'], c['numsteps'], G.BG3, ra, da)
        F, eF, _ = W.forward(c['numsteps'], np.array(G.BG3, np.float32), np.ones(c['n_rays'], bool))
        G.hold('xr_calc_rgb_inference', case, ra, da, rgb, F, eF, 'rgb')
        a, ea = W.alpha_out(c['numsteps'])
        G.hold('xr_calc_rgb_inference', case, ra, da, alpha[:, 0], a, ea, 'alpha')


def main(which):
    if which == 'oracle':
        run_oracle()
    elif which == 'emu':
        import emulib
        with emulib.emulated_ops() as dev:
            run_kernels(dev)
    else:
        import torch
        run_kernels(torch.device('cuda:0'))
    kernels = sorted({k for k, _ in G.WORST})
    print('\nworst |got - ref| / (u e), bar %g  [%s]' % (R.FACTOR, which))
    print('%-30s' % 'kernel' + ''.join('%8s' % c for c in 'ABCDE'))
    for k in kernels:
        print('%-30s' % k + ''.join('%8s' % ('%.3f' % G.WORST[k, c] if (k, c) in G.WORST else '-') for c in 'ABCDE'))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else 'gpu'))
