"""GNR's renderer stages on the MI355X (xrnerf_amd/csrc/xr_gnr_render.hip behind xrnerf_amd/gnr_render.py): visual hull and compaction,
pixel-aligned gather, blend compositor forward and backward.  The check_* bodies take the device, so tests/test_emu_gnr_render.py runs
them on the kernels' host build and tests/test_gnr_render_host.py on the tensor-op path.

Reference: tests/golden/ref_gnr_render.npz -- the reference's own GnrRenderer.render_rays and GNRMLP on a generated scene
(tests/golden/make_golden_gnr_render.py), a float32 run and a float64 run that is handed the float32 run's decisions.  For shapes the
fixture does not hold: tests/gnr_render_restatement.py in float64 (and in float32 for the bar), itself held to the fixture.

Bars (the convention of DESIGN.md sections 13 / 14): max |got - ref64| <= 4 max |ref32 - ref64| per tensor (per column where columns
differ in scale), floored at 2^-22 of the tensor's largest float64 magnitude.  Decisions (hull flags, smpl_vis) are compared wherever
the stored float64 distance from a deciding rounding boundary exceeds 1e-3 pixel (1e-4 for the depth comparison); at most 1 % of the
points may be left out that way.  Every check prints its worst figure next to the bar."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')

FLOOR = 2.0 ** -22
HULL_CASES = tuple((R, V) for R in (1, 3, 48) for V in (2, 4))
GATHER_CASES = tuple((N, C) for N in (1, 63, 65, 1000) for C in (16, 256))
GATHER_BWD_CASES = ((1, 16), (65, 16), (1000, 256))
COMPOSITE_CASES = ((4, False, 16), (2, True, 16), (4, False, 200))          # S = 200: more than one 64-lane chunk per ray
MODES = ('inf', 'trn')
RATIOS = {}                                     # what -> worst figure / bar, for profiles/gnr_render_gpu_tests.txt


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_gnr_render.npz'))


_scene = []


def scene():
    if not _scene:
        from xrnerf_amd.gnr_render import synthetic_scene
        _scene.append(synthetic_scene())
    return _scene[0]


def held(got, r32, r64, what, columns=False, floor_abs=0.0):
    got, r32, r64 = (np.asarray(a, np.float64) for a in (got, r32, r64))
    assert got.shape == r64.shape and np.isfinite(got).all(), what
    if got.size == 0:
        return
    ax = tuple(range(got.ndim - 1)) if columns else None
    scale = np.abs(r64).max(ax)
    bar = np.maximum(np.maximum(4.0 * np.abs(r32 - r64).max(ax), FLOOR * scale), floor_abs)
    worst = np.abs(got - r64).max(ax)
    ratio = float(np.max(worst / np.maximum(bar, 1e-300)))
    RATIOS[what] = max(RATIOS.get(what, 0.0), ratio)
    print('%s: worst %.3e, bar %.3e, ratio %.3f (max|ref| %.3e)' % (what, float(np.max(worst)), float(np.max(bar)), ratio, float(np.max(scale))))
    assert (worst <= bar).all(), (what, np.asarray(worst).tolist(), np.asarray(bar).tolist())


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


_targets = {}


def target(R):
    """ground-truth colours of R rays: the scene's for its 48, generated otherwise"""
    if R not in _targets:
        _targets[R] = scene()['rgb_gt'] if R == 48 else torch.from_numpy(np.random.default_rng(R).uniform(0, 1, (R, 3)).astype(np.float32))
    return _targets[R]


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.int32)


def hull_inputs(dev, gold, mode, R, V, tile=1):
    """the scene's first R rays, repeated `tile` times (the scan of the rays' counts takes 256 per sweep: 6 x 48 rays reach its second)"""
    sc = scene()
    return dict(rays=sc['rays'][:R].repeat(tile, 1).to(dev), t_vals=torch.from_numpy(gold[mode + '.t_vals'][:R]).repeat(tile, 1).to(dev),
                calibs=sc['calibs'][:V].to(dev),
                persps=sc['persps'][:V].to(dev), masks=sc['masks'][:V].to(dev), width=sc['width'], height=sc['width'],
                depth=sc['smpl']['depth'][:V].to(dev), rot=sc['smpl']['rot'][0].to(dev))


def hull64(inp):
    import gnr_render_restatement as RS
    d = lambda t: t.detach().cpu().double() if torch.is_tensor(t) else t
    return RS.hull(**{k: d(v) for k, v in inp.items()})


def hull32(inp):
    import gnr_render_restatement as RS
    d = lambda t: t.detach().cpu() if torch.is_tensor(t) else t
    return RS.hull(**{k: d(v) for k, v in inp.items()})


# ------------------------------------------------------------------------------------------ hull
def check_hull(dev, gold, R, V, mode='inf', tile=1):
    from xrnerf_amd import gnr_render as GR
    inp = hull_inputs(dev, gold, mode, R, V, tile)
    R *= tile
    S = inp['t_vals'].shape[1]
    got = GR.visual_hull(**inp)
    sync()
    r64 = hull64(inp)
    if V == 4:                                                     # the reference's own run
        want, boundary = gold[mode + '.inside'][:R * S], gold[mode + '.boundary'][:R * S]
    else:
        want, boundary = r64['inside'].numpy(), r64['boundary'].numpy()
    idx = got['idx'].cpu().numpy().astype(np.int64)
    flags = np.zeros(R * S, bool)
    flags[idx] = True
    compared = boundary > 1e-3
    print('hull %s R=%d V=%d: %d inside (fixture %d), %d flags differ among %d compared (bar 0), %d left out (bar %.2f)' % (
        mode, R, V, int(flags.sum()), int(want.sum()), int((flags != want)[compared].sum()), int(compared.sum()), int((~compared).sum()),
        0.01 * R * S))
    assert (~compared).sum() <= 0.01 * R * S
    assert np.array_equal(flags[compared], want[compared])
    assert got['M'] == idx.size and np.array_equal(idx, np.nonzero(flags)[0]), 'survivors in the order of torch.nonzero'
    table = got['table'].cpu().numpy()
    count = flags.reshape(R, S).sum(1)
    assert np.array_equal(table[:, 0], count) and np.array_equal(table[:, 1], np.cumsum(count) - count)
    # the compacted rows, on the survivors every run has
    keys = ('pts', 'xy', 'z', 'attdirs')
    if V == 4 and R == 48:
        widx = np.nonzero(want)[0]
        common = np.intersect1d(idx, widx)
        gi, wi = np.searchsorted(idx, common), np.searchsorted(widx, common)
        ref32 = {k: gold['%s.%s' % (mode, k)][wi] for k in keys}
        ref64 = {k: gold['%s.%s64' % (mode, k)][wi] for k in keys}
        vis_want, margin = gold[mode + '.smpl_vis'][wi], gold[mode + '.vis_margin'][wi]
    else:
        r32 = hull32(inp)
        assert np.array_equal(r32['inside'].numpy()[compared], want[compared])
        w32, w64 = np.nonzero(r32['inside'].numpy())[0], np.nonzero(r64['inside'].numpy())[0]
        common = np.intersect1d(np.intersect1d(idx, w32), w64)
        gi, i32, i64 = np.searchsorted(idx, common), np.searchsorted(w32, common), np.searchsorted(w64, common)
        ref32 = {k: r32[k].numpy()[i32] for k in keys}
        ref64 = {k: r64[k].numpy()[i64] for k in keys}
        vis_want, margin = r64['vis'].numpy()[i64], r64['vis_margin'].numpy()[i64]
    for k in keys:
        held(got[k].cpu().numpy()[gi], ref32[k], ref64[k], 'hull %s' % k, columns=(k == 'attdirs'))
    vis = got['vis'].cpu().numpy()[gi]
    sure = margin > 1e-4
    print('  smpl_vis: %d differ among %d compared (bar 0), %d left out (bar %.2f), true for %.2f' % (
        int((vis != vis_want)[sure].sum()), int(sure.sum()), int((~sure).sum()), 0.01 * sure.size, float(vis.mean()) if vis.size else 0.0))
    if R >= 48:                                                    # (the smaller cases are prefixes of this one)
        assert (~sure).sum() <= 0.01 * sure.size
    assert np.array_equal(vis[sure], vis_want[sure])
    again = GR.visual_hull(**inp)
    for k in ('table', 'idx'):
        assert torch.equal(again[k], got[k])
    for k in ('pts', 'xy', 'z', 'attdirs'):
        assert np.array_equal(bits(again[k]), bits(got[k])), 'a second run must repeat the bits of %s' % k
    assert torch.equal(again['vis'], got['vis'])


def check_hull_edges(dev, gold):
    """a NaN origin contributes no survivor; a camera behind the points puts them outside; R = 0 and no survivor launch nothing more"""
    from xrnerf_amd import gnr_render as GR
    inp = hull_inputs(dev, gold, 'inf', 48, 4)
    S = inp['t_vals'].shape[1]
    base = GR.visual_hull(**inp)
    rays = inp['rays'].clone()
    hit = int(torch.nonzero(base['table'][:, 0] > 0)[0])
    rays[hit, 1] = float('nan')
    got = GR.visual_hull(**dict(inp, rays=rays))
    assert int(got['table'][hit, 0]) == 0 and got['M'] == base['M'] - int(base['table'][hit, 0])
    keep = torch.cat([base['table'][:hit, 0], base['table'][hit + 1:, 0]])
    assert torch.equal(torch.cat([got['table'][:hit, 0], got['table'][hit + 1:, 0]]), keep)
    assert bool(torch.isfinite(got['pts']).all())
    behind = inp['calibs'].clone()
    behind[1, 2, :] = -behind[1, 2, :]                            # view 1 looks the other way: z <= 1e-9 for every point
    got = GR.visual_hull(**dict(inp, calibs=behind))
    assert got['M'] == 0 and int(got['table'].abs().sum()) == 0
    for k, shape in (('pts', (0, 3)), ('idx', (0,)), ('xy', (0, 4, 2)), ('z', (0, 4)), ('vis', (0, 4)), ('attdirs', (0, 5, 3))):
        assert tuple(got[k].shape) == shape
    empty = GR.visual_hull(**dict(inp, rays=inp['rays'][:0], t_vals=inp['t_vals'][:0]))
    assert empty['M'] == 0 and tuple(empty['table'].shape) == (0, 2)
    # the compositor on nothing: the reference's defaults
    sc = scene()
    for white, fill in ((False, 0.0), (True, 1.0)):
        rgb, depth, acc, w = GR.composite(torch.zeros((0, 9), device=dev), torch.zeros((0, 4, 3), device=dev), got['idx'], got['table'],
                                          inp['t_vals'], None, (float(sc['q_persps'][-2]), float(sc['q_persps'][-1])), white)
        assert tuple(rgb.shape) == (48, 6) and bool((rgb == fill).all()) and bool((depth == 0).all()) and bool((w == 0).all())
        assert tuple(w.shape) == (48, S) and bool((acc == 0).all())


# ------------------------------------------------------------------------------------------ gather
def gather_coordinates(N, V, seed):
    rng = np.random.default_rng([seed, N])
    xy = rng.uniform(-1.3, 1.3, (N, V, 2))
    special = np.array([[-1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.0, 0.3], [-1.6, 0.1], [1.7, -0.2], [0.2, -1.5], [0.1, 1.9]])
    n = min(N, len(special))
    for v in range(V):
        xy[:n, v] = np.roll(special, v, 0)[:n]
    return torch.from_numpy(xy.astype(np.float32))


def check_gather(dev, gold, N, C):
    import gnr_render_restatement as RS
    from xrnerf_amd import gnr_render as GR
    V, fh, fw, size = 4, 12, 20, 64
    rng = np.random.default_rng([C, 3])
    feats = torch.from_numpy(rng.normal(0, 1, (V, C, fh, fw)).astype(np.float32))
    images = torch.from_numpy(rng.uniform(0, 1, (V, 3, size, size)).astype(np.float32))
    xy = gather_coordinates(N, V, 11)
    col0, ld = 10, (10 + C + 3 + 3) // 4 * 4 + 4                   # 10 embedding columns in front, at least 4 padding columns behind
    out = torch.full((N, V, ld), 7.0, device=dev)
    rows, rgb = GR.pixel_gather(xy.to(dev), GR.channel_last(feats.to(dev)), images.to(dev), out, col0)
    sync()
    assert rows.data_ptr() == out.data_ptr() and tuple(rgb.shape) == (N, V, 3)
    rows = rows.cpu()
    assert bool((rows[:, :, :col0] == 7.0).all()), 'columns in front of col0 are left alone'
    assert bool((rows[:, :, col0 + C + 3:] == 0.0).all()) and rows[:, :, col0 + C + 3:].shape[-1] >= 4, 'padding is exact zeros'
    r64 = RS.gather(xy.double(), feats.double(), images.double()).numpy()
    r32 = RS.gather(xy, feats, images).numpy()
    held(rows[:, :, col0:col0 + C + 3].numpy(), r32, r64, 'gather N=%d C=%d' % (N, C))
    assert np.array_equal(bits(rgb), bits(rows[:, :, col0 + C:col0 + C + 3])), 'source_rgb is the row\'s colour'
    rows2, rgb2 = GR.pixel_gather(xy.to(dev), GR.channel_last(feats.to(dev)), images.to(dev))
    assert np.array_equal(bits(rows2[:, :, :C + 3]), bits(rows[:, :, col0:col0 + C + 3])) and rows2.shape[-1] % 4 == 0
    assert bool((rows2[:, :, C + 3:] == 0).all())


def check_gather_fixture(dev, gold, mode):
    from xrnerf_amd import gnr_render as GR
    sc = scene()
    xy = torch.from_numpy(gold[mode + '.xy']).to(dev)
    rows, rgb = GR.pixel_gather(xy, GR.channel_last(sc['feats'].to(dev)), sc['images'].to(dev))
    sync()
    C = sc['feats'].shape[1]
    ni = gold[mode + '.nerf_input']
    held(rows[:, :, :C + 3].cpu().numpy(), ni[..., ni.shape[-1] - C - 3:], gold[mode + '.gathered64'], 'gather fixture nerf_input', columns=True)
    held(rgb.cpu().numpy(), gold[mode + '.source_rgb'], gold[mode + '.source_rgb64'], 'gather fixture source_rgb')


def check_gather_backward(dev, gold, N, C, nan=True):
    """the gradient in the feature maps against float64 autograd of F.grid_sample; two runs repeat the bits; a NaN entry of the
    upstream gradient contributes nothing (kernel tiers: on the host path autograd carries it through)"""
    import gnr_render_restatement as RS
    from xrnerf_amd import gnr_render as GR
    V, fh, fw, size = 4, 12, 20, 64
    rng = np.random.default_rng([C, N, 9])
    feats = torch.from_numpy(rng.normal(0, 1, (V, C, fh, fw)).astype(np.float32))
    images = torch.from_numpy(rng.uniform(0, 1, (V, 3, size, size)).astype(np.float32))
    xy = gather_coordinates(N, V, 13)
    col0, ld = 10, (10 + C + 3 + 3) // 4 * 4
    g = torch.from_numpy(rng.normal(0, 1, (N, V, ld)).astype(np.float32))

    def run(grad):
        fl = GR.channel_last(feats.to(dev)).requires_grad_()
        rows, rgb = GR.pixel_gather(xy.to(dev), fl, images.to(dev), torch.zeros((N, V, ld), device=dev), col0)
        assert not rgb.requires_grad
        rows.backward(grad.to(dev))
        sync()
        return fl.grad.permute(0, 3, 1, 2).contiguous()

    def ref(dtype, grad):
        f = feats.detach().clone().to(dtype).requires_grad_()
        RS.gather(xy.to(dtype), f, images.to(dtype)).backward(grad[:, :, col0:col0 + C + 3].to(dtype))
        return f.grad.numpy()
    got = run(g)
    held(got.cpu().numpy(), ref(torch.float32, g), ref(torch.float64, g), 'gather backward N=%d C=%d' % (N, C))
    assert np.array_equal(bits(run(g)), bits(got)), 'a second run must repeat the bits'
    if nan:
        bad, zeroed = g.clone(), g.clone()
        bad[0, 1, col0 + 2], bad[N - 1, 0, col0 + C - 1] = float('nan'), float('inf')
        zeroed[0, 1, col0 + 2], zeroed[N - 1, 0, col0 + C - 1] = 0.0, 0.0
        held(run(bad).cpu().numpy(), ref(torch.float32, zeroed), ref(torch.float64, zeroed), 'gather backward with a NaN and an infinite entry')


# ------------------------------------------------------------------------------------------ compositor
def composite_inputs(dev, gold, mode):
    sc = scene()
    inside = gold[mode + '.inside']
    R, S = gold[mode + '.t_vals'].shape
    count = inside.reshape(R, S).sum(1)
    table = np.stack([count, np.cumsum(count) - count], 1).astype(np.int32)
    return dict(net=torch.from_numpy(gold[mode + '.net']).to(dev), source_rgb=torch.from_numpy(gold[mode + '.source_rgb']).to(dev),
                idx=torch.from_numpy(np.nonzero(inside)[0].astype(np.int32)).to(dev), table=torch.from_numpy(table).to(dev),
                t_vals=torch.from_numpy(gold[mode + '.t_vals']).to(dev), noise=sc['noise'].to(dev) if mode == 'trn' else None,
                z_near_far=(float(sc['q_persps'][-2]), float(sc['q_persps'][-1])), white=False)


def dense(inp, dtype, R_S=None):
    """the restatement's dense formulation on the same inputs -> (rgb_map, depth, acc, weights, d_net) for the fixture's loss"""
    import gnr_render_restatement as RS
    c = lambda t: t.detach().cpu().to(dtype)
    R, S = inp['t_vals'].shape
    inside = torch.zeros(R * S, dtype=torch.bool)
    inside[inp['idx'].cpu().long()] = True
    net = c(inp['net'])[:, :4 + inp['source_rgb'].shape[1] + 1].clone().requires_grad_()
    rgb_map, depth, acc, weights = RS.composite_dense(net, c(inp['source_rgb']), inside, c(inp['t_vals']),
                                                      c(inp['noise']) if inp['noise'] is not None else None, inp['z_near_far'], inp['white'])
    RS.loss(rgb_map, target(R).to(dtype)).backward()
    return [t.detach().numpy() for t in (rgb_map, depth, acc, weights)] + [net.grad.numpy()]


def run_composite(inp, dev):
    import gnr_render_restatement as RS
    from xrnerf_amd import gnr_render as GR
    net = inp['net'].clone().requires_grad_()
    rgb_map, depth, acc, weights = GR.composite(**dict(inp, net=net))
    loss = RS.loss(rgb_map, target(inp['t_vals'].shape[0]).to(dev))
    loss.backward()
    sync()
    V = inp['source_rgb'].shape[1]
    assert bool((net.grad[:, 4 + V + 1:] == 0).all())
    return rgb_map.detach(), depth.detach(), acc.detach(), weights.detach(), net.grad[:, :4 + V + 1].contiguous(), loss.detach()


def check_composite_fixture(dev, gold, mode):
    inp = composite_inputs(dev, gold, mode)
    rgb_map, depth, acc, weights, d_net, loss = run_composite(inp, dev)
    g = lambda k: (gold['%s.%s' % (mode, k)], gold['%s.%s64' % (mode, k)])
    held(rgb_map.cpu().numpy(), *g('rgb_map'), 'composite %s rgb_map' % mode, columns=True)
    held(depth.cpu().numpy(), *g('depth'), 'composite %s depth' % mode)
    held(weights.cpu().numpy(), *g('weights'), 'composite %s weights' % mode)
    held(acc.cpu().numpy(), gold[mode + '.weights'].sum(1), gold[mode + '.weights64'].sum(1), 'composite %s acc' % mode)
    held(float(loss), *g('loss'), 'composite %s loss' % mode)
    held(d_net.cpu().numpy(), *g('d_net'), 'composite %s d_net' % mode, columns=True)
    # the dense formulation, scattered to [R, S] with -1e4
    d64 = dense(inp, torch.float64)
    for name, got, a32, a64 in (('rgb_map', rgb_map, *g('rgb_map')), ('depth', depth, *g('depth')), ('weights', weights, *g('weights')),
                                ('d_net', d_net, *g('d_net'))):
        want = d64[{'rgb_map': 0, 'depth': 1, 'weights': 3, 'd_net': 4}[name]]
        held(got.cpu().numpy(), want + (a32 - a64), want, 'composite %s %s against the dense formulation' % (mode, name), columns=(name in ('rgb_map', 'd_net')))
    again = run_composite(inp, dev)
    for a, b in zip(again, (rgb_map, depth, acc, weights, d_net, loss)):
        assert np.array_equal(bits(a), bits(b)), 'a second run must repeat the bits'
    # the network's full output (occlusion columns behind the attention): a row stride, no copy
    wide = torch.cat([inp['net'], torch.full((inp['net'].shape[0], 4), 3.0, device=dev)], 1)
    other = run_composite(dict(inp, net=wide), dev)
    for a, b in zip(other, (rgb_map, depth, acc, weights, d_net, loss)):
        assert np.array_equal(bits(a), bits(b)), 'further columns are ignored'


def check_composite_cases(dev, gold, V, white, S=16):
    """generated ray tables: a ray without survivors, a ray with all 16 samples inside, single survivors first / last, more than one
    workgroup of rays; against the restatement's dense formulation (float32 run for the bar); with S = 200 a ray's survivors
    fill more than one 64-lane chunk (the fully inside rays four), so the carried product and the backward's chunk hand-over run"""
    R = 70
    rng = np.random.default_rng([V, int(white), 5] + ([S] if S != 16 else []))
    inside = rng.uniform(0, 1, (R, S)) < 0.4
    inside[0], inside[1], inside[2], inside[3], inside[R - 1] = False, True, False, False, True
    inside[2, 0], inside[3, S - 1] = True, True
    M = int(inside.sum())
    count = inside.sum(1)
    net = rng.normal(0, 1.5, (M, 4 + V + 1)).astype(np.float32)
    att = rng.uniform(0, 1, (M, V + 1))
    net[:, 4:] = (att / att.sum(1, keepdims=True)).astype(np.float32)
    net[rng.uniform(0, 1, M) < 0.1, 3] = 30.0                    # opaque samples: alpha rounds to 1, the factor to 1e-10
    t = np.linspace(0, 1, S, dtype=np.float32)[None] + ((rng.uniform(0, 1, (R, S)) - 0.5) / (S - 1)).astype(np.float32)
    inp = dict(net=torch.from_numpy(net).to(dev), source_rgb=torch.from_numpy(rng.uniform(0, 1, (M, V, 3)).astype(np.float32)).to(dev),
               idx=torch.from_numpy(np.nonzero(inside.reshape(-1))[0].astype(np.int32)).to(dev),
               table=torch.from_numpy(np.stack([count, np.cumsum(count) - count], 1).astype(np.int32)).to(dev),
               t_vals=torch.from_numpy(t).to(dev), noise=torch.from_numpy(rng.normal(0, 1, (R, S)).astype(np.float32)).to(dev),
               z_near_far=None if white else (1.8, 4.2), white=white)
    rgb_map, depth, acc, weights, d_net, _ = run_composite(inp, dev)
    d32, d64 = dense(inp, torch.float32), dense(inp, torch.float64)
    what = 'composite cases V=%d white=%d %s' % (V, white, '' if S == 16 else 'S=%d ' % S)
    for i, (name, got) in enumerate((('rgb_map', rgb_map), ('depth', depth), ('acc', acc), ('weights', weights), ('d_net', d_net))):
        held(got.cpu().numpy(), d32[i], d64[i], what + name, columns=(name in ('rgb_map', 'd_net')))
    fill = 1.0 if white else 0.0
    assert bool((rgb_map[0] == fill).all()) and float(depth[0]) == 0.0 and float(acc[0]) == 0.0 and bool((weights[0] == 0).all())
    assert bool((weights.cpu()[~torch.from_numpy(inside)] == 0).all()), 'no weight outside the hull'
    again = run_composite(inp, dev)
    for a, b in zip(again, (rgb_map, depth, acc, weights, d_net)):
        assert np.array_equal(bits(a), bits(b)), 'a second run must repeat the bits'


def check_end_to_end_stages(dev, gold, mode):
    """hull -> gather -> (the fixture's network output on the survivors) -> compositor: the stages chained on the fixture's inputs;
    rgb_map, depth and the loss on every ray none of whose samples was left out by the boundary rule"""
    import gnr_render_restatement as RS
    from xrnerf_amd import gnr_render as GR
    sc = scene()
    inp = hull_inputs(dev, gold, mode, 48, 4)
    h = GR.visual_hull(**inp)
    R, S = inp['t_vals'].shape
    want, boundary = gold[mode + '.inside'], gold[mode + '.boundary']
    rays_out = (boundary.reshape(R, S) <= 1e-3).any(1)
    assert rays_out.sum() <= 0.05 * R
    rows, src = GR.pixel_gather(h['xy'], GR.channel_last(sc['feats'].to(dev)), sc['images'].to(dev))
    # the network is not part of this library yet: the fixture's output, row by flat index
    widx = np.nonzero(want)[0]
    pos = np.searchsorted(widx, h['idx'].cpu().numpy())
    known = (pos < widx.size) & (widx[np.minimum(pos, widx.size - 1)] == h['idx'].cpu().numpy())
    net = np.zeros((h['M'], gold[mode + '.net'].shape[1]), np.float32)
    net[:, :4] = -1e4
    net[known] = gold[mode + '.net'][pos[known]]
    rgb_map, depth, acc, weights = GR.composite(torch.from_numpy(net).to(dev), src, h['idx'], h['table'], inp['t_vals'],
                                                sc['noise'].to(dev) if mode == 'trn' else None,
                                                (float(sc['q_persps'][-2]), float(sc['q_persps'][-1])), False)
    sync()
    keep = ~rays_out
    held(rgb_map.cpu().numpy()[keep], gold[mode + '.rgb_map'][keep], gold[mode + '.rgb_map64'][keep], 'stages %s rgb_map' % mode, columns=True)
    held(depth.cpu().numpy()[keep], gold[mode + '.depth'][keep], gold[mode + '.depth64'][keep], 'stages %s depth' % mode)
    held(kept_loss(rgb_map.cpu().numpy(), keep), kept_loss(gold[mode + '.rgb_map'], keep), kept_loss(gold[mode + '.rgb_map64'], keep),
         'stages %s loss' % mode)


# ------------------------------------------------------------------------------------------ GNRMLP, GnrRenderer
def load_params():
    return np.load(os.path.join(G, 'ref_gnr_render_params.npz'))


def config():
    import json
    with open(os.path.join(G, 'gnr_render_cfg.json')) as f:
        return json.load(f)


def built(dev, params, V=4):
    """(GNRMLP, GnrRenderer) built through the registry from the stored option dicts, the fixture's weights loaded strictly"""
    from xrnerf_amd import builder, gnr_render  # noqa: F401
    cfg = config()
    mlp = builder.build_mlp(dict(type='GNRMLP', opt=dict(cfg['nerf'], num_views=V), W=cfg['nerf_W']))
    if V == 4:
        mlp.load_state_dict({k[2:]: torch.from_numpy(params[k]) for k in params.files if k.startswith('w.')}, strict=True)
    mlp = mlp.to(dev)
    ren = builder.build_render(dict(type='GnrRenderer', opt=dict(cfg['nerf_renderer'], model=None, num_views=V)))
    ren.nerf = mlp
    return mlp, ren


ZERO_GRADIENT = 'value_linears.2.bias'


def held_param_grads(mlp, params, what):
    """per parameter tensor, the issue's bar.  One tensor has another floor: value_linears.2.bias shifts every attention logit alike,
    which the softmax ignores, so its true gradient is 0 (1e-19 in the float64 run) and every float32 run leaves rounding noise there
    whose scale is that of the sums it is made of, not of its own value.  Its floor is 2^-22 of the largest float64 gradient of its
    layer (the layer's weight gradient sums the same upstream rows)."""
    f64 = lambda n: params['trn.g.' + n].astype(np.float64) + params['trn.gd.' + n]
    for name, p in mlp.named_parameters():
        floor = FLOOR * float(np.abs(f64('value_linears.2.weight')).max()) if name == ZERO_GRADIENT else 0.0
        held(p.grad.cpu().numpy(), params['trn.g.' + name].astype(np.float64), f64(name), '%s gradient of %s' % (what, name), floor_abs=floor)


def check_mlp(dev, gold, params):
    """strict load; the output on the fixture's nerf_input / attention directions, alpha_only, and (training case, the fixture's
    upstream gradient) the parameter gradients"""
    mlp, _ = built(dev, params)
    ref_keys = sorted(k[2:] for k in params.files if k.startswith('w.'))
    assert sorted(mlp.state_dict().keys()) == ref_keys
    t = lambda k: torch.from_numpy(gold[k]).to(dev)
    for mode in MODES:
        x, att, vis = t(mode + '.nerf_input'), t(mode + '.attdirs'), t(mode + '.smpl_vis')
        out = mlp(x, att, smpl_vis=vis)
        sync()
        V = x.shape[1]
        assert tuple(out.shape) == (x.shape[0], 4 + V + 1 + V)
        held(out.detach().cpu().numpy()[:, :4 + V + 1], gold[mode + '.net'], gold[mode + '.net64'], 'GNRMLP %s output' % mode, columns=True)
        alpha = mlp(x, att, alpha_only=True)
        held(alpha.detach().cpu().numpy()[:, 0], gold[mode + '.net'][:, 3], gold[mode + '.net64'][:, 3], 'GNRMLP %s alpha_only' % mode)
    mlp.zero_grad()
    up = torch.cat([t('trn.d_net'), torch.zeros((out.shape[0], V), device=dev)], 1)
    out.backward(up)
    sync()
    held_param_grads(mlp, params, 'GNRMLP')


def check_mlp_two_views(dev, gold, params):
    """V = 2 (own weights) against the float64 restatement of the reference's forward"""
    import gnr_render_restatement as RS
    torch.manual_seed(3)
    mlp, _ = built(dev, params, V=2)
    with torch.no_grad():
        for name, p in mlp.named_parameters():
            if name.endswith('weight'):
                p.mul_(3.0)
    x = torch.from_numpy(gold['inf.nerf_input'][:65, :2].copy())
    att = torch.from_numpy(gold['inf.attdirs'][:65, :3].copy())
    out = mlp(x.to(dev), att.to(dev))
    sync()
    sd = {k: v.detach().cpu() for k, v in mlp.state_dict().items()}
    r32 = RS.gnr_mlp(sd, x, att).numpy()
    r64 = RS.gnr_mlp({k: v.double() for k, v in sd.items()}, x.double(), att.double()).numpy()
    held(out.detach().cpu().numpy(), r32, r64, 'GNRMLP V=2 output', columns=True)


def kept_loss(rgb_map, keep):
    import gnr_render_restatement as RS
    gt = scene()['rgb_gt'].double()[torch.from_numpy(keep)]
    return float(RS.loss(torch.as_tensor(np.asarray(rgb_map, np.float64))[torch.from_numpy(keep)], gt))


def check_render_rays(dev, gold, params, mode):
    """GnrRenderer.render_rays on the fixture's inputs: rgb_map, depth and the loss on every ray none of whose samples the boundary
    rule leaves out (at most 5 % of the rays); with the training draws, one step's parameter gradients"""
    mlp, ren = built(dev, params)
    sc = scene()
    d = lambda t: t.to(dev)
    smpl = {k: d(v) for k, v in sc['smpl'].items()}
    param = {'center': d(sc['mesh_param']['center']), 'spatial_freq': sc['mesh_param']['spatial_freq']}
    train = mode == 'trn'
    rgb_map, depth = ren.render_rays(d(sc['rays']), d(sc['feats']), d(sc['images']), d(sc['masks']), d(sc['calibs']), smpl, param,
                                     persps=d(sc['persps']), q_persps=sc['q_persps'], is_train=train, t_rand=d(sc['t_rand']), noise=d(sc['noise']))
    loss = ren.cal_loss(rgb_map, d(sc['rgb_gt']))
    R, S = sc['t_rand'].shape
    keep = ~(gold[mode + '.boundary'].reshape(R, S) <= 1e-3).any(1)
    assert (~keep).sum() <= 0.05 * R
    assert tuple(rgb_map.shape) == (R, 6) and tuple(depth.shape) == (R,)
    got = rgb_map.detach().cpu().numpy()
    held(got[keep], gold[mode + '.rgb_map'][keep], gold[mode + '.rgb_map64'][keep], 'render_rays %s rgb_map' % mode, columns=True)
    held(depth.detach().cpu().numpy()[keep], gold[mode + '.depth'][keep], gold[mode + '.depth64'][keep], 'render_rays %s depth' % mode)
    held(kept_loss(got, keep), kept_loss(gold[mode + '.rgb_map'], keep), kept_loss(gold[mode + '.rgb_map64'], keep), 'render_rays %s loss' % mode)
    if keep.all():
        held(float(loss.detach()), gold[mode + '.loss'], gold[mode + '.loss64'], 'render_rays %s cal_loss' % mode)
    if train:
        assert keep.all(), 'the training case leaves no ray out, so the whole step is comparable'
        mlp.zero_grad()
        loss.backward()
        sync()
        held_param_grads(mlp, params, 'render_rays')


def check_renderer_contract(dev, gold, params):
    """the config's dicts build through the registry; refused options raise what DESIGN says; no survivor and R = 0 give the defaults"""
    from xrnerf_amd import builder
    from xrnerf_amd.gnr_render import GNRMLP, GnrRenderer
    cfg = config()
    mlp, ren = built(dev, params)
    assert isinstance(mlp, GNRMLP) and isinstance(ren, GnrRenderer)
    full = builder.build_mlp(dict(type='GNRMLP', opt=dict(cfg['nerf'], input_ch_feat=256)))        # the config's own size
    assert full.alpha_linears[0].in_features == 63 + 7 + 259 and full.W == 256
    for key, exc in (('use_vh_free', NotImplementedError), ('debug', NotImplementedError), ('regularization', NotImplementedError),
                     ('angle_diff', NotImplementedError)):
        with pytest.raises(exc, match=key):
            builder.build_render(dict(type='GnrRenderer', opt=dict(cfg['nerf_renderer'], model=None, **{key: True})))
    with pytest.raises(NotImplementedError, match='projection'):
        builder.build_render(dict(type='GnrRenderer', opt=dict(cfg['nerf_renderer'], model=None), projection='orthogonal'))
    with pytest.raises(ValueError, match='activation'):
        builder.build_mlp(dict(type='GNRMLP', opt=cfg['nerf'], activation='swish'))
    with pytest.raises(ValueError, match='weighted_pool'):
        builder.build_mlp(dict(type='GNRMLP', opt=dict(cfg['nerf'], weighted_pool=False)))
    with pytest.raises(NotImplementedError):
        ren.reconstruct(None, None, None, None, None, None)
    sc = scene()
    d = lambda t: t.to(dev)
    smpl = {k: d(v) for k, v in sc['smpl'].items()}
    param = {'center': d(sc['mesh_param']['center']), 'spatial_freq': sc['mesh_param']['spatial_freq']}
    args = (d(sc['feats']), d(sc['images']), d(sc['masks']) * 0, d(sc['calibs']), smpl, param)      # empty masks: no survivor
    for rays in (d(sc['rays']), d(sc['rays'])[:0]):
        rgb, depth = ren.render_rays(rays, *args, persps=d(sc['persps']), q_persps=sc['q_persps'], is_train=False)
        assert tuple(rgb.shape) == (rays.shape[0], 6) and tuple(depth.shape) == (rays.shape[0],)
        assert bool((rgb == 0).all()) and bool((depth == 0).all())
    # the other methods keep the reference's signatures and agree with the stages
    rs, re_ = ren.get_rays_perspective([8, 12, 20, 26], d(sc['q_calib']), d(sc['q_persps']))
    assert tuple(rs.shape) == (4, 6, 3) and tuple(re_.shape) == (4, 6, 3)
    pts = torch.from_numpy(gold['inf.pts']).to(dev)
    inside, vis, scan_vis = ren.inside_pts_vh(pts, d(sc['masks']), smpl, d(sc['calibs']), d(sc['persps']))
    sure = gold['inf.boundary'][gold['inf.inside']] > 1e-3
    assert bool(inside.cpu()[torch.from_numpy(sure)].all()) and scan_vis is None and vis.shape[1] == 4


def check_tables_in_step():
    """the header, the ctypes table and the library's exported symbols name the same renderer entry points"""
    import re
    from xrnerf_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_gnr.h')).read()
    declared = set(re.findall(r'^(?:int|size_t) (xr_gnr_\w+)\(', header, re.M))
    assert declared == set(_lib.GNR_SIGNATURES) | set(_lib.GNR_RENDER_SIGNATURES)
    for name, (res, args) in _lib.GNR_RENDER_SIGNATURES.items():
        text = header[header.index(' %s(' % name):]
        text = text[:text.index(');')]
        assert text.count(',') + 1 == len(args), name
        assert hasattr(_lib.load(), name), name


def write_ratios(tier):
    path = os.environ.get('XR_GNR_RENDER_RATIOS')
    if path:
        with open(path, 'w') as f:
            f.write('# worst |got - ref64| / bar of every bar of tests/test_gpu_gnr_render.py on the %s (1.0 = at the bar)\n' % tier)
            for k in sorted(RATIOS):
                f.write('%-70s %.4f\n' % (k, RATIOS[k]))


# ------------------------------------------------------------------------------------------ the MI355X
@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from xrnerf_amd import ops
    assert ops.gnr_render_kernels_available(), 'the library has no xr_gnr_render entry points'
    yield torch.device('cuda')
    write_ratios('MI355X')


@pytest.mark.gpu
@pytest.mark.parametrize('R,V', HULL_CASES)
def test_hull_flags_order_and_rows(dev, gold, R, V):
    from xrnerf_amd import ops
    assert ops.gnr_render_kernels_available()
    check_hull(dev, gold, R, V)


@pytest.mark.gpu
def test_hull_with_the_training_draws(dev, gold):
    check_hull(dev, gold, 48, 4, 'trn')


@pytest.mark.gpu
def test_hull_of_288_rays_scans_the_counts_in_two_sweeps(dev, gold):
    check_hull(dev, gold, 48, 2, tile=6)


@pytest.mark.gpu
def test_hull_nan_ray_camera_behind_and_nothing_to_do(dev, gold):
    check_hull_edges(dev, gold)


@pytest.mark.gpu
@pytest.mark.parametrize('N,C', GATHER_CASES)
def test_gather_against_float64_grid_sample(dev, gold, N, C):
    check_gather(dev, gold, N, C)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
def test_gather_holds_the_fixture(dev, gold, mode):
    check_gather_fixture(dev, gold, mode)


@pytest.mark.gpu
@pytest.mark.parametrize('N,C', GATHER_BWD_CASES)
def test_gather_backward_to_the_feature_maps(dev, gold, N, C):
    check_gather_backward(dev, gold, N, C)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
def test_compositor_holds_the_fixture_forward_and_backward(dev, gold, mode):
    check_composite_fixture(dev, gold, mode)


@pytest.mark.gpu
@pytest.mark.parametrize('V,white,S', COMPOSITE_CASES)
def test_compositor_empty_full_and_opaque_rays(dev, gold, V, white, S):
    check_composite_cases(dev, gold, V, white, S)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
def test_stages_chained_on_the_fixture(dev, gold, mode):
    check_end_to_end_stages(dev, gold, mode)


@pytest.fixture(scope='module')
def params():
    return load_params()


@pytest.mark.gpu
def test_gnrmlp_strict_load_output_alpha_only_and_parameter_gradients(dev, gold, params):
    check_mlp(dev, gold, params)


@pytest.mark.gpu
def test_gnrmlp_with_two_views_against_the_restatement(dev, gold, params):
    check_mlp_two_views(dev, gold, params)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
def test_render_rays_on_the_fixture(dev, gold, params, mode):
    check_render_rays(dev, gold, params, mode)


@pytest.mark.gpu
def test_config_builds_refusals_and_empty_hull(dev, gold, params):
    check_renderer_contract(dev, gold, params)


@pytest.mark.gpu
def test_header_table_and_library_name_the_same_entry_points(dev):
    check_tables_in_step()
