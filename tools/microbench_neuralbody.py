"""NeuralBody at the config's shape (configs/neuralbody/nb_zjumocap_313.py: 6890 vertices, 5 mm voxels, 1024 rays x 64 samples):
train_step + backward + torch Adam through the kernel path (xrnerf_amd/csrc/xr_neuralbody.hip) and through the module's own tensor-op
path (neuralbody.tensor_op_path(True)) on the device, each replaced stage on its own against the tensor-op composition it replaces,
and a frame of chunks with and without the per-frame reuse of the sparse network's levels.  Median of 5 windows of 10 calls (the frame:
3 windows of 1), the two paths alternating window by window in one process.

  python tools/microbench_neuralbody.py [--stage step|structure|net|sample|frame|all]

Each stage can be run as a command of its own (under a time limit of its own)."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument('--stage', default='all', choices=('step', 'structure', 'net', 'sample', 'frame', 'all'))
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--samples', type=int, default=64)
    ap.add_argument('--verts', type=int, default=6890)
    ap.add_argument('--voxel', type=float, default=0.005)
    ap.add_argument('--frame-rays', type=int, default=16384, help='rays of the frame of chunks (chunk = the config\'s 4096)')
    args = ap.parse_args()
    import xrnerf_amd
    from xrnerf_amd import neuralbody as NB
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    cfg = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'neuralbody_model_cfg.json')))['model']
    cfg['cfg']['smpl_embedder']['voxel_size'] = [args.voxel] * 3
    datas = NB.synthetic_frame(args.verts, 5, args.rays, args.samples, device=dev)
    want = lambda s: args.stage in (s, 'all')

    def make(seed=0):
        torch.manual_seed(seed)
        net = xrnerf_amd.build_network(copy.deepcopy(cfg)).to(dev)
        return net, torch.optim.Adam(net.parameters(), lr=5e-4)
    nets = {'kernels': make(), 'tensor ops': make()}

    def on(which, f):
        def run():
            old = NB.tensor_op_path(which == 'tensor ops')
            try:
                return f()
            finally:
                NB.tensor_op_path(old)
        return run

    def step(which):
        net, opt = nets[which]
        return NB.train_step(net, {k: v[None] for k, v in datas.items()}, opt)

    emb = nets['kernels'][0].smpl_conv
    coord, out_sh, min_xyz = emb.prepare(datas)
    frame = NB.build_frame(coord, out_sh)
    print('shape: %d vertices, voxel %g, out_sh %r (%d cells), rows per level %r, %d rays x %d samples' % (
        args.verts, args.voxel, list(out_sh), out_sh[0] * out_sh[1] * out_sh[2], frame.n, args.rays, args.samples))
    rows = []

    def bench(name, f, **kw):
        r = windows({k: on(k, lambda k=k: f(k)) for k in ('kernels', 'tensor ops')}, **kw)
        rows.append((name, r['kernels'], r['tensor ops']))

    if want('step'):
        bench('train_step + backward + Adam', step)
    if want('structure'):
        bench('frame structure (5 levels, 13 tables)', lambda k: NB.build_frame(coord, out_sh))
    if want('net') or want('sample'):
        frames = {'kernels': frame, 'tensor ops': on('tensor ops', lambda: NB.build_frame(coord, out_sh))()}
        code = torch.randn(frame.n[0], 16, device=dev)
    if want('net'):
        def net_fwd(k):
            with torch.no_grad():
                return nets[k][0].smpl_conv.xyzc_net(code, frames[k])

        def net_both(k):
            net = nets[k][0].smpl_conv.xyzc_net
            net.zero_grad(set_to_none=True)
            sum(f.sum() for f in net(code, frames[k])).backward()
        bench('sparse network forward (17 convolutions)', net_fwd)
        bench('sparse network forward + backward', net_both)
    if want('sample'):
        feats = {k: [torch.randn(frames[k].n[l + 1], c, device=dev, requires_grad=True) for l, c in enumerate(NB.LEVEL_CHANNELS)]
                 for k in frames}
        g = torch.randn(args.rays * args.samples, 352, device=dev)
        R, T = datas['smpl_R'], datas['smpl_T']

        def samp_fwd(k):
            with torch.no_grad():
                return NB.sample_features(feats[k], frames[k], datas['pts'], R, T, min_xyz, args.voxel)

        def samp_both(k):
            for f in feats[k]:
                f.grad = None
            (NB.sample_features(feats[k], frames[k], datas['pts'], R, T, min_xyz, args.voxel) * g).sum().backward()
        bench('feature sampling forward (%d points)' % g.shape[0], samp_fwd)
        bench('feature sampling forward + row gradients', samp_both)
    if want('frame'):
        fd = NB.synthetic_frame(args.verts, 5, args.frame_rays, args.samples, device=dev)

        def per_chunk(net):
            """the reference's val_step: the whole forward, sparse network included, for every chunk"""
            N = fd['rays_o'].shape[0]
            with torch.no_grad():
                for i in range(0, N, net.chunk):
                    net.forward({k: (v[i:i + net.chunk] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == N and k in NB._RAY_KEYS else v)
                                 for k, v in fd.items()}, True)
        r = windows({'reuse': lambda: nets['kernels'][0].render_frame(fd), 'per chunk': lambda: per_chunk(nets['kernels'][0]),
                     'tensor ops per chunk': on('tensor ops', lambda: per_chunk(nets['tensor ops'][0]))}, n_windows=3, n_calls=1, warmup=1)
        print('frame of %d rays in chunks of %d: levels reused %.3f ms, sparse network per chunk %.3f ms, tensor ops per chunk %.3f ms' % (
            args.frame_rays, nets['kernels'][0].chunk, r['reuse'], r['per chunk'], r['tensor ops per chunk']))
    if rows:
        print('%-46s %12s %12s %8s' % ('stage', 'kernel ms', 'tensor ms', 'ratio'))
        for name, k, t_ in rows:
            print('%-46s %12.4f %12.4f %8.2f' % (name, k, t_, t_ / k))
        slower = [name for name, k, t_ in rows if k > t_]
        print('stages slower than the tensor ops they replace: %s' % (', '.join(slower) or 'none'))


if __name__ == '__main__':
    main()
