"""Test-set evaluation at the shape of the Blender test set: one 800 x 800 x 3 frame pair (tests/eval_cases.py's kind of pair: gt U(0,1)
with a flat white half, rgb = gt + 0.05 N(0,1)), MSE + PSNR + SSIM as ValidateHook measures them.

Rows, alternating window by window in one process, their outputs compared before they are timed:
  kernels          evaluate.frame_metrics on the device frame (csrc/xr_eval.hip: one tile launch, one fold)
  tensor ops       the module's own tensor-op path (evaluate._ssim_tensor_ops + img2mse's expression) on the device, in float64
  host             the frame copied to the host (the D2H copy is inside the window) and measured by the tensor-op path there -- the
                   shape of the reference's path, which calls skimage on the host
and the 8-bit side-by-side image: the kernel, against the copy of both fp32 frames it replaces.

  python tools/microbench_eval.py [--out profiles/eval_microbench.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fns, n_windows=5, n_calls=10, warmup=3):
    """fns: {name: (callable, calls per window)}; -> {name: (median ms per call, min, max)}, the callables alternating window by window;
    a host clock around work that ends in a device synchronise (the host row's work is on the host)"""
    for f, _ in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(n_windows):
        for k, (f, calls) in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0) / calls)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=800)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from xrnerf_amd import evaluate as EV
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    n = args.size
    rng = np.random.default_rng(0)
    gt = rng.uniform(0, 1, (n, n, 3)).astype(np.float32)
    gt[:, n // 2:] = 1.0
    rgb = (gt + 0.05 * rng.normal(0, 1, gt.shape)).astype(np.float32)
    x, y = torch.from_numpy(rgb).to(dev), torch.from_numpy(gt).to(dev)
    taps, cov = EV.window(7)
    R = EV.REFERENCE_SSIM_DATA_RANGE
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2

    def kernels():
        return EV.frame_metrics(x, y)

    def tensor_ops(a=x, b=y):
        mse = ((a - b).double() ** 2).mean()
        sums, _ = EV._ssim_tensor_ops(a[None], b[None], taps, cov, C1, C2)
        return torch.stack([mse, EV.mse2psnr(mse), sums[0] / a.numel()])

    def host():
        return tensor_ops(x.cpu(), y.cpu())
    k, t, h = kernels().cpu(), tensor_ops().cpu(), host()
    _, mk = EV.calculate_ssim(x, y, data_range=R, full=True)
    _, mt = EV._ssim_tensor_ops(x[None], y[None], taps, cov, C1, C2)
    pair = EV.ops.eval_to8b_pair(x, y)
    want = EV.to8b(np.hstack((rgb, gt)))
    lines = ['test-set evaluation on %s: one %d x %d x 3 frame pair, uniform 7 x 7 window, data_range %.1f' % (torch.cuda.get_device_name(0), n, n, R),
             'mse / psnr / ssim  kernels    %.12e %.9f %.15f' % tuple(k.tolist()),
             '                   tensor ops %.12e %.9f %.15f' % tuple(t.tolist()),
             '                   host       %.12e %.9f %.15f' % tuple(h.tolist()),
             'S map, kernels against tensor ops on the device: %d of %d values differ in their bits, max |difference| %.3e'
             % (int((mk.view(torch.int64) != mt[0].view(torch.int64)).sum()), mk.numel(), float((mk - mt[0]).abs().max())),
             '8-bit pair against numpy: %d of %d bytes differ' % (int((pair.cpu().numpy() != want).sum()), want.size), '',
             'median ms per frame (min .. max), 5 windows; a host clock around a synchronised window', '']
    assert abs(float(k[2] - t[2])) <= n * n * 3 * 2.0 ** -53 and abs(float(k[2] - h[2])) <= n * n * 3 * 2.0 ** -53, 'the three paths disagree on SSIM'
    assert abs(float(k[0] - t[0])) <= 2.0 ** -22 * float(t[0]) and int((pair.cpu().numpy() != want).sum()) == 0
    print('timing ...', flush=True)
    r = windows({'kernels': (kernels, 50), 'tensor ops': (tensor_ops, 5), 'host': (host, 2)})
    for name, calls in (('kernels', 50), ('tensor ops', 5), ('host', 2)):
        lines.append('%-44s %10.4f (%.4f .. %.4f)   %d calls per window' % (('mse + psnr + ssim, %s' % name,) + r[name] + (calls,)))
    lines.append('tensor ops on the device / kernels = %.0f x; host (with its D2H copy) / kernels = %.0f x' % (r['tensor ops'][0] / r['kernels'][0], r['host'][0] / r['kernels'][0]))
    p = windows({'to8b pair kernel + copy of the bytes': (lambda: EV.ops.eval_to8b_pair(x, y).cpu(), 20),
                 'copy of both fp32 frames + numpy to8b': (lambda: EV.to8b(np.hstack((x.cpu().numpy(), y.cpu().numpy()))), 5)})
    lines.append('')
    for name, v in p.items():
        lines.append('%-44s %10.4f (%.4f .. %.4f)' % ((name,) + v))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
