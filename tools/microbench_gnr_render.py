"""GNR's renderer stages at the shape of configs/gnr/gnr_genebody.py: 1024 rays x 256 samples = 262 144 points, 4 source views, feature
maps [4, 256, 128, 128], images and masks 512 x 512, synthetic_mesh(5, 0) as the body (gnr_render.synthetic_scene at that size).

Rows: the visual hull with its compaction, the pixel-aligned gather forward and forward + backward (the gradient in the feature maps),
the blend compositor forward and forward + backward, and the three chained -- each kernel path against the tensor-op composition it
replaces (the host path's lines of xrnerf_amd/gnr_render.py run on device tensors), the two alternating window by window in one
process.  Device events around windows of calls, median of 5 windows after warm-up; every pair's outputs are compared at this size
before they are timed.  The survivors' share is recorded: it sets what the nearest-point query (profiles/gnr_microbench.txt) costs per
step once it is handed the survivors only.  The last row is render_rays as a whole: one training call with its backward, the three stages as kernels against the three stages as
tensor ops; the mesh queries and the network are the same on both sides.

  python tools/microbench_gnr_render.py [--out profiles/gnr_render_microbench.txt]"""
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
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--map', type=int, default=128)
    ap.add_argument('--subdivisions', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from xrnerf_amd import gnr_render as GR
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    R, S, V = args.rays, args.samples, 4
    sc = GR.synthetic_scene(0, R, S, V, args.size, args.channels, args.map, args.map, args.subdivisions)
    t_vals = (torch.linspace(0., 1., S)[None].repeat(R, 1) + (sc['t_rand'] - 0.5) / (S - 1)).to(dev)
    hull_in = dict(rays=sc['rays'].to(dev), t_vals=t_vals, calibs=sc['calibs'].to(dev), persps=sc['persps'].to(dev), masks=sc['masks'].to(dev),
                   width=args.size, height=args.size, depth=sc['smpl']['depth'].to(dev), rot=sc['smpl']['rot'][0].to(dev))
    feats, images = sc['feats'].to(dev), sc['images'].to(dev)
    feats_last = GR.channel_last(feats)
    noise = sc['noise'].to(dev)
    zz = (float(sc['q_persps'][-2]), float(sc['q_persps'][-1]))

    # the pairs' outputs at this size
    hk, ht = GR.visual_hull(**hull_in), GR.hull_tensor_ops(**hull_in)
    M = hk['M']
    same = hk['M'] == ht['M'] and torch.equal(hk['idx'], ht['idx'])
    differ = int(hk['M'] != ht['M']) if same else int(torch.ne(torch.zeros(R * S, dtype=torch.bool, device=dev).index_fill(0, hk['idx'].long(), True),
                                                             torch.zeros(R * S, dtype=torch.bool, device=dev).index_fill(0, ht['idx'].long(), True)).sum())
    lines = ['GNR renderer stages on %s: %d rays x %d samples = %d points, %d views, features [%d, %d, %d, %d], images %d x %d'
             % (torch.cuda.get_device_name(0), R, S, R * S, V, V, args.channels, args.map, args.map, args.size, args.size),
             'survivors of the visual hull: %d of %d points (%.1f %%), %d of %d rays cross it; %d flags differ between kernel and tensor ops'
             % (M, R * S, 100.0 * M / (R * S), int((hk['table'][:, 0] > 0).sum()), R, differ)]
    xy, idx, table = hk['xy'], hk['idx'], hk['table']
    rows_k, src_k = GR.pixel_gather(xy, feats_last, images)
    lat_t, src_t = GR.gather_tensor_ops(xy, feats, images)
    C = args.channels
    lines.append('gather at this size: max |kernel - tensor ops| %.3e' % float((rows_k[:, :, :C + 3] - lat_t).abs().max()))
    g = torch.Generator(device='cpu').manual_seed(1)
    up = torch.randn((M, V, C + 3), generator=g).to(dev)
    up_rows = torch.cat([up, up.new_zeros((M, V, rows_k.shape[2] - C - 3))], -1)

    def gather_grad(kernel):
        """forward and the gradient in the feature maps (train_encoder), channel-last for the kernel, channel-first for the tensor ops"""
        if kernel:
            f = feats_last.detach().requires_grad_()
            GR.pixel_gather(xy, f, images)[0].backward(up_rows)
            return f.grad.permute(0, 3, 1, 2)
        f = feats.detach().requires_grad_()
        GR.gather_tensor_ops(xy, f, images)[0].backward(up)
        return f.grad
    gk_, gt2 = gather_grad(True), gather_grad(False)
    lines.append('gather backward at this size: max |kernel - tensor ops| %.3e (largest %.3e)' % (float((gk_ - gt2).abs().max()), float(gt2.abs().max())))
    net = torch.randn((M, 4 + V + 1 + V), generator=g).to(dev)
    net[:, 4:4 + V + 1] = torch.softmax(net[:, 4:4 + V + 1], -1)
    gt = sc['rgb_gt'].to(dev)

    def comp(fn, grad):
        n = net.clone().requires_grad_(grad)
        out = fn(n)
        if grad:
            (((out[0][:, :3] - gt) ** 2).mean() + ((out[0][:, 3:] - gt) ** 2).mean()).backward()
            return out, n.grad
        return out, None
    kern = lambda n: GR.composite(n, src_k, idx, table, t_vals, noise, zz, False)
    tens = lambda n: GR.composite_tensor_ops(n, src_k, idx, R, S, t_vals, noise, zz, False)
    (ok, gk), (ot, gt_) = comp(kern, True), comp(tens, True)
    lines.append('compositor at this size: max |kernel - tensor ops| rgb_map %.3e, depth %.3e, weights %.3e, gradient %.3e (largest %.3e)'
                 % (float((ok[0] - ot[0]).detach().abs().max()), float((ok[1] - ot[1]).detach().abs().max()), float((ok[3] - ot[3]).detach().abs().max()),
                    float((gk - gt_).abs().max()), float(gt_.abs().max())))
    lines += ['median ms per call of 5 windows of 10 calls (min .. max)', '']

    def chain(hull, gather, composite):
        h = hull(**hull_in)
        rows, src = gather(h['xy'])
        n = net[:h['M']].clone().requires_grad_()
        out = composite(n, src, h)
        (((out[0][:, :3] - gt) ** 2).mean() + ((out[0][:, 3:] - gt) ** 2).mean()).backward()
    pairs = (
        ('hull + compaction', lambda: GR.visual_hull(**hull_in), lambda: GR.hull_tensor_ops(**hull_in)),
        ('gather forward', lambda: GR.pixel_gather(xy, feats_last, images), lambda: GR.gather_tensor_ops(xy, feats, images)),
        ('gather forward + backward', lambda: gather_grad(True), lambda: gather_grad(False)),
        ('compositor forward', lambda: comp(kern, False), lambda: comp(tens, False)),
        ('compositor forward + backward', lambda: comp(kern, True), lambda: comp(tens, True)),
        ('stages chained', lambda: chain(GR.visual_hull, lambda q: GR.pixel_gather(q, feats_last, images),
                                         lambda n, s, h: GR.composite(n, s, h['idx'], h['table'], t_vals, noise, zz, False)),
         lambda: chain(GR.hull_tensor_ops, lambda q: GR.gather_tensor_ops(q, feats, images),
                       lambda n, s, h: GR.composite_tensor_ops(n, s, h['idx'], R, S, t_vals, noise, zz, False))),
    )
    # render_rays as a whole: one training call, forward and backward, the config's GNRMLP (W = 256) and renderer options.  The
    # composition runs the three stages as tensor ops (gnr_render.TENSOR_OPS_STAGES); the mesh queries (no tensor-op form exists) and
    # the network are the same code on both sides, and both sides query the survivors only
    import json
    from xrnerf_amd import builder, gnr
    with open(os.path.join(ROOT, 'tests', 'golden', 'gnr_render_cfg.json')) as f:
        cfg = json.load(f)
    mlp = builder.build_mlp(dict(type='GNRMLP', opt=dict(cfg['nerf'], input_ch_feat=C))).to(dev)
    ren = builder.build_render(dict(type='GnrRenderer', opt=dict(cfg['nerf_renderer'], model=None, N_samples=S, loadSize=args.size, N_rand=R)))
    ren.nerf = mlp
    smpl = {k: v.to(dev) for k, v in sc['smpl'].items()}
    param = {'center': sc['mesh_param']['center'].to(dev), 'spatial_freq': sc['mesh_param']['spatial_freq']}
    t_rand = sc['t_rand'].to(dev)

    def step(tensor_ops):
        GR.TENSOR_OPS_STAGES = tensor_ops
        try:
            rgb, _ = ren.render_rays(hull_in['rays'], feats, images, hull_in['masks'], hull_in['calibs'], smpl, param, persps=hull_in['persps'],
                                     q_persps=sc['q_persps'], is_train=True, t_rand=t_rand, noise=noise)
            mlp.zero_grad(set_to_none=True)
            ren.cal_loss(rgb, gt).backward()
            return rgb.detach()
        finally:
            GR.TENSOR_OPS_STAGES = False
    lines.insert(-2, 'render_rays at this size: max |kernel - tensor-op stages| rgb_map %.3e' % float((step(False) - step(True)).abs().max()))
    searcher = gnr.MeshGridSearcher(smpl['verts'], smpl['faces'])
    all_pts = GR.sample_points(hull_in['rays'], t_vals).contiguous()
    q = windows({'all points': lambda: searcher.nearest_points(all_pts), 'survivors': lambda: searcher.nearest_points(hk['pts'])}, n_windows=3, n_calls=2, warmup=1)
    cl = windows({'channel_last': lambda: GR.channel_last(feats)})
    pairs = pairs + (('render_rays, training call + backward', lambda: step(False), lambda: step(True)),)
    losers = []
    for name, k, t in pairs:
        r = windows({'kernel': k, 'tensor ops': t})
        ratio = r['tensor ops'][0] / r['kernel'][0]
        lines.append('%-30s kernel %9.4f (%.4f .. %.4f)   tensor ops %9.4f (%.4f .. %.4f)   tensor ops / kernel = %.2f x'
                     % ((name,) + r['kernel'] + r['tensor ops'] + (ratio,)))
        if ratio < 1.0:
            losers.append(name)
    lines += ['', 'nearest-point query (both sides of the render_rays row hand it the survivors): all %d points %.3f ms, the %d survivors %.3f ms'
              % (R * S, q['all points'][0], M, q['survivors'][0]),
              'channel-last conversion of the feature maps, once per frame, counted in no row above except render_rays (cached there): %.4f ms' % cl['channel_last'][0]]
    lines += ['', 'condition: no replaced stage slower than its composition -- %s' % ('met' if not losers else 'NOT met by: ' + ', '.join(losers))]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
