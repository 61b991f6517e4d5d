"""Animatable NeRF at the config's shape (configs/animatable_nerf/an_h36m_s9_train_pose.py: 1024 rays x 64 samples, 6890 vertices,
`train_pose`): train_step + backward + torch Adam through the kernel path (xrnerf_amd/csrc/xr_aninerf.hip) and through the module's own
tensor-op path (aninerf.tensor_op_path(True)) on the device, and each replaced stage on its own against the tensor-op composition it
replaces.  Median of 5 windows of 10 calls, the two paths alternating window by window in one process.

  python tools/microbench_aninerf.py            the step and the per-stage table
  python tools/microbench_aninerf.py --trace    5 kernel-path steps only (to be run under a kernel tracer, in a run of its own)

The tensor-op nearest-vertex query materialises [chunk, V, 3] differences: it runs in pieces of aninerf.CLOSEST_CHUNK = 4096 points
(339 MB per piece at V = 6890; 65 536 points at once would be 5.4 GB of differences plus the distance matrix)."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def windows(fns, n_windows=5, n_calls=10, warmup=3):
    """fns: {name: callable}; -> {name: median ms per call}, the callables alternating window by window"""
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(n_windows):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n_calls):
                f()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / n_calls)
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--samples', type=int, default=64)
    ap.add_argument('--verts', type=int, default=6890)
    args = ap.parse_args()
    import xrnerf_amd
    from xrnerf_amd import aninerf, ops
    import aninerf_restatement as RS
    dev = torch.device('cuda:0')
    cfg = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'aninerf_model_cfg.json')))['model']
    datas = aninerf.synthetic_body(args.verts, 5, args.rays, args.samples, device=dev)

    def make(seed=0):
        torch.manual_seed(seed)
        net = xrnerf_amd.build_network(copy.deepcopy(cfg)).to(dev)
        return net, torch.optim.Adam(net.get_params(), lr=5e-4)
    nets = {'kernels': make(), 'tensor ops': make()}

    def step(which):
        net, opt = nets[which]
        old = aninerf.tensor_op_path(which == 'tensor ops')
        try:
            out = net.train_step({k: v[None] for k, v in datas.items()}, opt)
            opt.zero_grad(set_to_none=True)
            out['loss'].backward()
            opt.step()
        finally:
            aninerf.tensor_op_path(old)
        return out

    if args.trace:
        for _ in range(5):
            step('kernels')
        torch.cuda.synchronize()
        return
    out = step('kernels')
    n_sel = int(out['ret']['deform']['sel'].numel())
    print('shape: %d rays x %d samples = %d queries, %d vertices, %d near the body (%.1f %%)' % (
        args.rays, args.samples, args.rays * args.samples, args.verts, n_sel, 100.0 * n_sel / (args.rays * args.samples)))
    t = windows({k: (lambda k=k: step(k)) for k in nets})
    print('train_step + backward + Adam: kernels %.3f ms, tensor ops %.3f ms (x%.2f)' % (t['kernels'], t['tensor ops'], t['tensor ops'] / t['kernels']))

    # ---- each replaced stage against the tensor ops it replaces, at this step's sizes
    pts = datas['pts'].reshape(-1, 3)
    R, T = datas['smpl_R'], datas['smpl_T'].reshape(3)
    q, idx, dist, flag = ops.ani_closest(pts, datas['smpl_verts'], 0.05, R, T)
    sel = aninerf.select(flag, dist)
    M = sel.numel()
    qs, idxs = q[sel].contiguous(), idx[sel].contiguous()
    logits = torch.randn(M, 24, device=dev)
    g24, g3, g3b = torch.randn(M, 24, device=dev), torch.randn(M, 3, device=dev), torch.randn(M, 3, device=dev)
    dirs = torch.nn.functional.normalize(torch.randn(M, 3, device=dev), dim=-1)
    bw = ops.ani_blend_forward(datas['smpl_bw'], idxs, logits)
    A, B = datas['A'], datas['big_A']
    rows = []

    def tensor(f):
        def run():
            old = aninerf.tensor_op_path(True)
            try:
                return f()
            finally:
                aninerf.tensor_op_path(old)
        return run

    def bench(name, kernel, torch_ops):
        r = windows({'k': kernel, 't': torch_ops})
        rows.append((name, r['k'], r['t']))

    bench('closest vertex (%d x %d)' % (pts.shape[0], args.verts), lambda: ops.ani_closest(pts, datas['smpl_verts'], 0.05, R, T),
          tensor(lambda: aninerf.closest(pts, datas['smpl_verts'], 0.05, R, T)))
    bench('selection (%d -> %d)' % (pts.shape[0], M), lambda: aninerf.select(flag, dist), tensor(lambda: aninerf.select(flag, dist)))
    bench('blend head forward (%d)' % M, lambda: ops.ani_blend_forward(datas['smpl_bw'], idxs, logits),
          lambda: RS.blend(datas['smpl_bw'], idxs, logits))
    lg = logits.clone().requires_grad_(True)

    def blend_both():
        lg.grad = None
        (RS.blend(datas['smpl_bw'], idxs, lg) * g24).sum().backward()
    bench('blend head forward + backward', lambda: ops.ani_blend_backward(ops.ani_blend_forward(datas['smpl_bw'], idxs, logits), g24), blend_both)
    bench('skinning forward, points + dirs', lambda: ops.ani_skin_forward(qs, dirs, bw, A, B), lambda: RS.skin(qs, dirs, bw, A, B))
    bwg = bw.clone().requires_grad_(True)

    def skin_both():
        bwg.grad = None
        p, d = RS.skin(qs, dirs, bwg, A, B)
        ((p * g3).sum() + (d * g3b).sum()).backward()
    bench('skinning forward + backward', lambda: (ops.ani_skin_forward(qs, dirs, bw, A, B), ops.ani_skin_backward(qs, dirs, bw, A, B, g3, g3b)),
          skin_both)
    ge = torch.randn(M, 64, device=dev)
    pg = qs.clone().requires_grad_(True)

    def enc_both():
        pg.grad = None
        (RS.embed(pg, 10) * ge[:, :63]).sum().backward()
    bench('encoding forward + input gradient (L = 10)', lambda: (ops.nerf_encode(qs, qs, 10, 0), ops.ani_encode_backward(qs, ge, 10)), enc_both)
    print('%-46s %12s %12s %8s' % ('stage', 'kernel ms', 'tensor ms', 'ratio'))
    for name, k, t_ in rows:
        print('%-46s %12.4f %12.4f %8.2f' % (name, k, t_, t_ / k))
    slower = [name for name, k, t_ in rows if k > t_]
    print('stages slower than the tensor ops they replace: %s' % (', '.join(slower) or 'none'))


if __name__ == '__main__':
    main()
