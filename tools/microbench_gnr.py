"""GNR's body-shape queries at SMPL-X scale: synthetic_mesh(5, 0) (10 242 vertices, 20 480 faces) with 262 144 queries (the sample
points of one make_nerf_input call), uniform in a box around the body sized so that about a fifth of them are inside.

Rows: set_mesh (grid build, with its two blocking reads), nearest_points, inside_mesh, and the embedding kernel against the tensor-op
composition it replaces (gnr.embedding_tensor_ops), the two alternating window by window in one process.  Device events around windows
of calls, median of 5 windows after warm-up; the embedding pair's outputs are compared at this size before they are timed.  The grid
build and the two searches have no tensor-op equivalent: their times are recorded and carry no bar.  The embedding kernel must not be
slower than the composition.

  python tools/microbench_gnr.py [--out profiles/gnr_microbench.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fns, n_windows=5, n_calls=10, warmup=3):
    """fns: {name: callable}; -> {name: (median ms per call, min, max)}, the callables alternating window by window"""
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
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--subdivisions', type=int, default=5)
    ap.add_argument('--queries', type=int, default=262144)
    ap.add_argument('--grow', type=float, default=0.0, help='the query box: the bounding box grown by this on every side')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from xrnerf_amd import gnr
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    mesh = {k: v.to(dev) for k, v in gnr.synthetic_mesh(args.subdivisions, 0).items()}
    V, F = mesh['verts'].shape[0], mesh['faces'].shape[0]
    lo, hi = mesh['verts'].min(0)[0] - args.grow, mesh['verts'].max(0)[0] + args.grow
    g = torch.Generator(device='cpu').manual_seed(0)
    pts = (torch.rand((args.queries, 3), generator=g).to(dev) * (hi - lo) + lo).contiguous()
    param = {'center': ((hi + lo) / 2), 'spatial_freq': 180.0}
    width = 512
    s = gnr.MeshGridSearcher(mesh['verts'], mesh['faces'])
    near_pts, near_faces = s.nearest_points(pts)
    signs = s.inside_mesh(pts)
    inside = float((signs > 0).float().mean())
    k_out, k_alpha = gnr.embed(pts, near_pts, near_faces, signs, mesh, param, width)
    t_out, t_alpha = gnr.embedding_tensor_ops(pts, near_pts, near_faces, signs, mesh, param, width, True, True, True)
    worst = float((k_out - t_out).abs().max())
    assert torch.equal(k_alpha, t_alpha) and worst < 1e-5, worst
    lines = ['GNR body-shape queries on %s: synthetic_mesh(%d, 0) = %d vertices, %d faces; grid %s = %d cells, %d slots; %d queries, %.1f %% inside'
             % (torch.cuda.get_device_name(0), args.subdivisions, V, F, s.num[:3].tolist(), int(s.num[3]), s.tri_idx.numel(), args.queries, 100 * inside),
             'embedding kernel against the tensor-op composition at this size: max |difference| %.3e, alpha_smpl equal' % worst,
             'median ms per call of 5 windows (min .. max); set_mesh: windows of 5 calls, the rest: windows of 10', '']
    r = windows({'set_mesh': lambda: s.set_mesh(mesh['verts'], mesh['faces'])}, n_calls=5)
    r.update(windows({'nearest_points': lambda: s.nearest_points(pts), 'inside_mesh': lambda: s.inside_mesh(pts)}))
    r.update(windows({'embedding kernel': lambda: gnr.embed(pts, near_pts, near_faces, signs, mesh, param, width),
                      'embedding tensor ops': lambda: gnr.embedding_tensor_ops(pts, near_pts, near_faces, signs, mesh, param, width, True, True, True)}))
    for k, (med, mn, mx) in r.items():
        lines.append('%-22s %9.4f   (%.4f .. %.4f)' % (k, med, mn, mx))
    ratio = r['embedding tensor ops'][0] / r['embedding kernel'][0]
    lines += ['', 'embedding: tensor ops / kernel = %.2f x (condition: >= 1)' % ratio]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    assert ratio >= 1.0, 'the embedding kernel is slower than the composition it replaces'


if __name__ == '__main__':
    main()
