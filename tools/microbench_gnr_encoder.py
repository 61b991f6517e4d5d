"""GNR's image encoder at the shape of configs/gnr/gnr_genebody.py: HGFilter (group norm, 4 stacks, hourglass depth 2, ave_pool) on
[4, 3, 512, 512] images, generated weights (tests/gnr_encoder_restatement.make_state_dict).

Rows: the stem (7x7 stride-2 convolution, group norm, relu), one ConvBlock(256, 256) at 128 x 128, 64 x 64 and 32 x 32, one hourglass,
one stack (hourglass, top_m, conv_last, bn_end, l, bl, al), the whole filter, and render_rays (one training call with its backward,
tools/microbench_gnr_render.py's last row) with the encoder in front -- each kernel path (csrc/xr_gnr_encoder.hip, channel-last)
against the tensor-op path it replaces (the same modules' host path run on device tensors, NCHW, the vendor convolution library), the
two alternating window by window in one process.  Device events around windows of calls, median of 5 windows after warm-up; the
outputs are compared at this size before anything is timed.  Every line is written as it is measured.

  python tools/microbench_gnr_encoder.py [--out profiles/gnr_encoder_microbench.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def windows(fns, n_windows=5, n_calls=10, warmup=2):
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
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--calls', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import gnr_encoder_restatement as RS
    from xrnerf_amd import builder, gnr_encoder as E, gnr_render as GR, ops
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    V, size = args.views, args.size
    out = open(args.out, 'w') if args.out else None

    def say(line=''):
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    with open(os.path.join(ROOT, 'tests', 'golden', 'gnr_encoder_cfg.json')) as f:
        filt = builder.build_embedder(json.load(f)['image_filter'])
    filt.load_state_dict(RS.make_state_dict({k: tuple(v.shape) for k, v in filt.state_dict().items()}), strict=True)
    filt = filt.eval().to(dev)
    for p in filt.parameters():
        p.requires_grad = False
    g = torch.Generator().manual_seed(0)
    images = (torch.rand((V, 3, size, size), generator=g) * 2 - 1).to(dev)
    m = filt._modules

    def tensor_ops(fn):
        def run():
            E.TENSOR_OPS = True
            try:
                with torch.no_grad():
                    return fn()
            finally:
                E.TENSOR_OPS = False
        return run

    def kernels(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    say('GNR image encoder on %s: HGFilter %s on images [%d, 3, %d, %d]' % (torch.cuda.get_device_name(0), json.dumps(RS.CONFIG_OPT, sort_keys=True), V, size, size))
    yk, yt = kernels(lambda: filt(images))(), tensor_ops(lambda: filt(images))()
    torch.cuda.synchronize()
    say('whole filter at this size: max |kernel - tensor ops| %.3e (largest %.3e, std %.3f); the kernels\' output is the channel-last buffer: %s'
        % (float((yk - yt).abs().max()), float(yt.abs().max()), float(yt.std()), GR.channel_last(yk).data_ptr() == yk.data_ptr()))
    say('median ms per call of 5 windows of %d calls (min .. max)' % args.calls)
    say()

    def maps(C, s):
        x = torch.randn((V, C, s, s), generator=g).to(dev)
        return x, x.permute(0, 2, 3, 1).contiguous()

    def stem_k():
        x = E._conv_k(filt.conv1, E._last(images))
        return ops.hg_gn_relu(x, *E._gn(ops.hg_gn_stats(x), filt.bn1), out=x)

    def stack_k(prev):
        prev = prev.clone()
        ll = E._conv_k(m['conv_last0'], m['top_m_0'].forward_last(m['m0'].forward_last(prev)))
        end = E._gn(ops.hg_gn_stats(ll), m['bn_end0'])
        tmp = E._conv_k(m['l0'], ll, end)
        E._conv_k(m['bl0'], ll, end, out=prev, accumulate=True)
        E._conv_k(m['al0'], tmp, out=prev, accumulate=True)
        return prev

    def stack_t(prev):
        ll = F.relu(m['bn_end0'](m['conv_last0'](m['top_m_0'](m['m0'](prev)))))
        tmp = m['l0'](ll)
        return prev + m['bl0'](ll) + m['al0'](tmp)
    q = size // 4
    blk = m['top_m_0']
    rows = [('stem 7x7 s2 + norm + relu', kernels(stem_k), tensor_ops(lambda: F.relu(filt.bn1(filt.conv1(images)))))]
    for s in (q, q // 2, q // 4):
        x, xl = maps(256, s)
        rows.append(('ConvBlock(256, 256) at %d x %d' % (s, s), kernels(lambda xl=xl: blk.forward_last(xl)), tensor_ops(lambda x=x: blk(x))))
    x, xl = maps(256, q)
    rows.append(('one hourglass (depth 2)', kernels(lambda: m['m0'].forward_last(xl)), tensor_ops(lambda: m['m0'](x))))
    rows.append(('one stack', kernels(lambda: stack_k(xl)), tensor_ops(lambda: stack_t(x))))
    rows.append(('whole filter', kernels(lambda: filt(images)), tensor_ops(lambda: filt(images))))
    results = {}
    for name, k, t in rows:
        r = windows({'kernel': k, 'tensor ops': t}, n_calls=args.calls)
        results[name] = r
        say('%-32s kernel %9.4f (%.4f .. %.4f)   tensor ops %9.4f (%.4f .. %.4f)   tensor ops / kernel = %.2f x'
            % ((name,) + r['kernel'] + r['tensor ops'] + (r['tensor ops'][0] / r['kernel'][0],)))

    # render_rays with the encoder in front: one training call with its backward at the configuration's size (tools/microbench_gnr_render.py's
    # last row), the frozen encoder on the kernels against the frozen encoder on tensor ops; the renderer's stages are kernels on both sides
    R, S = args.rays, args.samples
    sc = GR.synthetic_scene(0, R, S, V, size, 256, q, q, 5)
    with open(os.path.join(ROOT, 'tests', 'golden', 'gnr_render_cfg.json')) as f:
        cfg = json.load(f)
    mlp = builder.build_mlp(dict(type='GNRMLP', opt=dict(cfg['nerf'], input_ch_feat=256))).to(dev)
    ren = builder.build_render(dict(type='GnrRenderer', opt=dict(cfg['nerf_renderer'], model=None, N_samples=S, loadSize=size, N_rand=R)))
    ren.nerf = mlp
    d = lambda t: t.to(dev)
    smpl = {k: d(v) for k, v in sc['smpl'].items()}
    param = {'center': d(sc['mesh_param']['center']), 'spatial_freq': sc['mesh_param']['spatial_freq']}
    src = d(sc['images']) * 2 - 1
    rays, masks, calibs, persps, t_rand, noise, gt = (d(sc[k]) for k in ('rays', 'masks', 'calibs', 'persps', 't_rand', 'noise', 'rgb_gt'))

    def step(tensor):
        E.TENSOR_OPS = tensor
        try:
            with torch.no_grad():
                feats = filt(src)
        finally:
            E.TENSOR_OPS = False
        rgb, _ = ren.render_rays(rays, feats, d(sc['images']), masks, calibs, smpl, param, persps=persps, q_persps=sc['q_persps'], is_train=True,
                                 t_rand=t_rand, noise=noise)
        mlp.zero_grad(set_to_none=True)
        ren.cal_loss(rgb, gt).backward()
        return rgb.detach()
    say()
    say('render_rays at this size: max |encoder kernels - encoder tensor ops| rgb_map %.3e' % float((step(False) - step(True)).abs().max()))
    r = windows({'kernel': lambda: step(False), 'tensor ops': lambda: step(True)}, n_calls=args.calls)
    say('%-32s kernel %9.4f (%.4f .. %.4f)   tensor ops %9.4f (%.4f .. %.4f)   tensor ops / kernel = %.2f x'
        % (('encoder + render_rays + backward',) + r['kernel'] + r['tensor ops'] + (r['tensor ops'][0] / r['kernel'][0],)))
    w = results['whole filter']
    say()
    say('condition: the whole filter is not slower than the tensor-op path it replaces -- %s' % ('met' if w['kernel'][0] <= w['tensor ops'][0] else 'NOT met'))
    losers = [n for n, r in results.items() if r['kernel'][0] > r['tensor ops'][0]]
    say('rows that lose: %s' % (', '.join(losers) if losers else 'none'))


if __name__ == '__main__':
    main()
