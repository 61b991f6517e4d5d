"""The bodies of the float64 checks of the KiloNeRF tiny-MLP kernels (xrnerf_amd/csrc/xr_kilo.hip: k_kilo_mlp, k_kilo_mlp_bwd<1|2>,
k_kilo_student_step<1|2>, k_kilo_student_fwd<1|2>), shared by the GPU tier (tests/test_gpu_kilo_f64.py) and the host emulation of the same
source (tests/test_kilo_f64_host.py).  Everything runs through the public wrappers (ops.kilo_mlp_forward / kilo_mlp_backward,
kilo.MultiNetwork.packed / unpack_like, kilo_distill.student_step / student_forward) against tests/ref64_kilo.py, network by network and
entry by entry: every number is held to ITS OWN propagated rounding bound, so a one-sample network is judged at its own scale.

Scene: 24 networks on a 2 x 3 x 4 grid, explicit sample positions [R, 7, 3] (7 samples per ray: rays straddle networks), per-ray unit view
directions.  The number of samples per network is CHOSEN (COUNTS: every size at which the 128-sample tile / 32-sample wave code changes
path); networks 0, 23 and the adjacent pair 11, 12 are empty, the networks left over hold 2 or 3 samples, about 150 samples lie outside
the domain, and the samples are shuffled over the rays.  Every sample keeps 2e-3 from every face of its cell, of its occupancy voxel and of
the global box (more than the 1e-3 of a cell edge and the 2e-3 of the global faces that float32 and float64 need to agree on the cell).
Weights: uniform +-sqrt(6 / fan_in), biases likewise, one seed per network.

Kink-free points: a sample with a unit closer to its relu kink than twice that unit's forward bound e_z is redrawn (deterministic, at
most 16 rounds), and fewer than 10 % of a case's points may need that (a cap on a margin mis-scaled upwards).  Measured on the host with
8 000 points per architecture: 0.09 % (1, 0, 1), 0.6 % (5, 3, 2), 0.9 % (10, 4, 2), 1.7 % (11, 5, 3), 8.2 % (16, 16, 8).  For the students
the share is taken over all batches of an architecture together: a batch of one example has no share of its own."""
import functools
import json
import os

import numpy as np
import torch

import ref64_kilo as R64

GMIN, GMAX, FIXED = (-0.67, -1.2, -0.37), (0.67, 1.2, 1.03), (2, 3, 4)
OCC_RES = (4, 6, 8)
N_NETS, S_PER_RAY = 24, 7
EMPTY = (0, 11, 12, 23)
COUNTS = (1, 31, 32, 33, 64, 95, 96, 97, 127, 128, 129, 160, 161, 256, 257, 385, 1500)
COUNTS_HOST = (1, 33, 129)
ARCH_FWD = ((10, 4, 2), (1, 0, 1), (5, 3, 2), (4, 1, 1), (0, 0, 1), (11, 5, 3), (16, 16, 8))
ARCH_BWD = ARCH_FWD[:5]
ARCH_REFUSED = ((11, 4, 2), (10, 5, 2), (10, 4, 3))
BATCHES = (1, 31, 32, 33, 127, 128, 129, 257, 416)
BATCHES_HOST = (33, 129)
MARGIN = 2e-3
MIN_KINK_MARGIN = 2.0
STRIDE_PAD = 8
U = R64.U


def log(rec):
    """KILO_F64_LOG=<file>: append what each check measured (worst error / bound per tensor, redrawn share, the ulp constants)"""
    path = os.environ.get('KILO_F64_LOG')
    if path:
        rec = dict(rec, s_trig=R64.S_TRIG, s_exp=R64.S_EXP)
        with open(path, 'a') as f:
            f.write(json.dumps(rec) + '\n')


def ratio(got, ref, bound):
    """worst |got - ref| / bound; where the bound is zero the entry must equal the reference exactly (inf otherwise)"""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


# ------------------------------------------------------------------------------------------ networks
def dims(arch):
    pf, df, nh = arch
    return 3 * (2 * pf + 1), 3 * (2 * df + 1)


def make_network(arch, n_nets, seed):
    """kilo.MultiNetwork on the host with uniform +-sqrt(6 / fan_in) weights and biases, a different seed per network"""
    from xrnerf_amd import kilo
    P, D = dims(arch)
    mn = kilo.MultiNetwork(n_nets, P, D, num_hidden_layers=arch[2])
    ps = mn.ordered_parameters()
    with torch.no_grad():
        for n in range(n_nets):
            rng = np.random.default_rng(100000 * seed + n)
            for k in range(0, len(ps), 2):
                w, b = ps[k], ps[k + 1]
                bound = np.sqrt(6.0 / w.shape[1])
                w[n] = torch.from_numpy(rng.uniform(-bound, bound, tuple(w.shape[1:])).astype(np.float32))
                b[n] = torch.from_numpy(rng.uniform(-bound, bound, tuple(b.shape[1:])).astype(np.float32))
    return mn


def ref_nets(mn):
    ts = [p.detach().numpy() for p in mn.ordered_parameters()]
    return [R64.Net(ts, n) for n in range(mn.num_networks)]


def padded_blocks(mn, dev, seed=5):
    """the packed blocks with STRIDE_PAD floats of stride padding per network (a known non-zero filler the kernels must never read into a result)"""
    packed = mn.packed()
    g = torch.Generator().manual_seed(seed)
    fill = torch.randn((packed.shape[0], STRIDE_PAD), generator=g) + 3.0
    return torch.cat([packed, fill], 1).contiguous().to(dev)


def pad_mask(arch, stride):
    """True at the floats of a block that hold no parameter: 3 after b_alpha, the rgb head's 4th column and 4th bias, the stride padding"""
    P, D = dims(arch)
    nh = arch[2]
    m = np.zeros(stride, bool)
    o_alpha = P * 32 + 32 + (nh - 1) * (32 * 32 + 32)
    m[o_alpha + 33:o_alpha + 36] = True
    o_rgb = o_alpha + 36 + (32 * 32 + 32) + ((32 + D) * 32 + 32)
    m[o_rgb + 3:o_rgb + 128:4] = True
    m[o_rgb + 131] = True
    assert o_rgb + 132 == stride - STRIDE_PAD
    m[o_rgb + 132:] = True
    return m


def domains():
    from xrnerf_amd import kilo_distill
    lo, hi = kilo_distill.fixed_resolution_domains(GMIN, GMAX, FIXED)
    return lo.numpy(), hi.numpy()


# ------------------------------------------------------------------------------------------ the scene
def _draw_in_cells(rng, nets, lo, hi):
    """one point per entry of `nets` inside that network's cell: a random octant (= occupancy voxel of the 4 x 6 x 8 grid), MARGIN away
    from the octant's faces -> float32 positions, flat occupancy index"""
    nets = np.asarray(nets)
    clo, chi = lo[nets].astype(np.float64), hi[nets].astype(np.float64)
    half = (chi - clo) / 2
    octant = rng.integers(0, 2, (len(nets), 3))
    a = clo + octant * half + MARGIN
    p = a + rng.uniform(0, 1, (len(nets), 3)) * (half - 2 * MARGIN)
    cell = np.stack(np.unravel_index(nets, FIXED), 1)
    oi = 2 * cell + octant
    return p.astype(np.float32), np.ravel_multi_index((oi[:, 0], oi[:, 1], oi[:, 2]), OCC_RES)


def layout(counts):
    """designed number of samples per network: the chosen counts on the non-empty networks in a fixed shuffled order, 2 or 3 on the rest"""
    per = np.zeros(N_NETS, np.int64)
    free = [n for n in range(N_NETS) if n not in EMPTY]
    order = np.random.default_rng(len(counts)).permutation(len(free))
    for k, j in enumerate(order):
        per[free[j]] = counts[k] if k < len(counts) else 2 + (k % 2)
    return per


@functools.lru_cache(maxsize=None)
def case(arch, counts, seed=1):
    """the scene for one architecture (the kink-free redraw depends on the weights).  Cached: the tests share it and leave it unchanged."""
    per = layout(counts)
    lo, hi = domains()
    mn = make_network(arch, N_NETS, seed)
    nets = ref_nets(mn)
    rng = np.random.default_rng(seed)
    net_of = np.repeat(np.arange(N_NETS), per)
    n_in = len(net_of)
    n_out = 150 if len(counts) > 4 else 10
    n_out += (-(n_in + n_out)) % S_PER_RAY
    n_rays = (n_in + n_out) // S_PER_RAY
    pts, occ_idx = _draw_in_cells(rng, net_of, lo, hi)
    # outside the domain: beyond one face by 0.01 .. 0.5 on a random axis, anywhere on the others
    g0, g1 = np.array(GMIN), np.array(GMAX)
    out = g0 + rng.uniform(-0.2, 1.2, (n_out, 3)) * (g1 - g0)
    ax, side, far = rng.integers(0, 3, n_out), rng.integers(0, 2, n_out), rng.uniform(0.01, 0.5, n_out)
    out[np.arange(n_out), ax] = np.where(side == 0, g0[ax] - far, g1[ax] + far)
    perm = rng.permutation(n_in + n_out)                                  # slot of each sample on the [R, 7] lattice
    dirs = rng.normal(0, 1, (n_rays, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)
    v_of = dirs[perm[:n_in] // S_PER_RAY]
    # kink-free points
    redrawn, near_plain = np.zeros(n_in, bool), np.zeros(n_in, bool)
    todo = np.arange(n_in)
    for rnd in range(16):
        bad = []
        for n in np.unique(net_of[todo]):
            idx = todo[net_of[todo] == n]
            f = R64.forward(nets[n], R64.local_x(pts[idx], lo[n], hi[n]), v_of[idx])
            bad.append(idx[f['margin'] < MIN_KINK_MARGIN])
            if rnd == 0:
                near_plain[idx] = f['plain_margin'] < 1024.0
        todo = np.concatenate(bad) if bad else np.zeros(0, np.int64)
        if len(todo) == 0:
            break
        redrawn[todo] = True
        pts[todo], occ_idx[todo] = _draw_in_cells(rng, net_of[todo], lo, hi)
    assert len(todo) == 0, 'points next to a kink left after 16 rounds'
    share = float(redrawn.mean())
    assert share < 0.10, share
    allp = np.zeros((n_in + n_out, 3), np.float32)
    allp[perm[:n_in]] = pts
    allp[perm[n_in:]] = out.astype(np.float32)
    return dict(arch=arch, mn=mn, nets=nets, per=per, lo=lo, hi=hi, slot=perm[:n_in], net_of=net_of, occ_idx=occ_idx, n_rays=n_rays,
                pts=allp.reshape(n_rays, S_PER_RAY, 3), viewdirs=dirs, redrawn_share=share, share_within_1024u=float(near_plain.mean()), memo={})


def _active(c, occupancy):
    """samples (indices into c['slot']) a network evaluates, the occupancy grid [4, 6, 8] (or None), the voxel switched off"""
    if not occupancy:
        return np.ones(len(c['slot']), bool), None
    big = int(np.argmax(c['per'] == 129))
    vox = np.bincount(c['occ_idx'][c['net_of'] == big], minlength=int(np.prod(OCC_RES))).argmax()
    occ = np.ones(int(np.prod(OCC_RES)), bool)
    occ[vox] = False
    keep = c['occ_idx'] != vox
    assert 0 < (~keep).sum() < 129
    return keep, occ


def reference(c, occupancy=False, drop_sample=False, drop_feature=None, drop_bias=None):
    """float64 forward of every network over its samples -> per network (sample slots, forward dict); cached per variant"""
    key = (occupancy, drop_sample, drop_feature, drop_bias)
    if key not in c['memo']:
        keep, _ = _active(c, occupancy)
        if drop_sample:                                              # mutation: the 129-sample network loses its last sample
            keep = keep.copy()
            keep[np.flatnonzero(c['net_of'] == int(np.argmax(c['per'] == 129)))[-1]] = False
        out = {}
        for n in range(N_NETS):
            idx = np.flatnonzero((c['net_of'] == n) & keep)
            slots = c['slot'][idx]
            p = c['pts'].reshape(-1, 3)[slots]
            f = R64.forward(c['nets'][n], R64.local_x(p, c['lo'][n], c['hi'][n]), c['viewdirs'][slots // S_PER_RAY], drop=drop_feature,
                            drop_bias=drop_bias)
            out[n] = (slots, f)
        c['memo'][key] = out
    return c['memo'][key]


def _scene_args(c, dev, occupancy):
    _, occ = _active(c, occupancy)
    occ_t = None if occ is None else torch.from_numpy(occ).to(dev)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(viewdirs=T(c['viewdirs']), gmin=GMIN, gmax=GMAX, fixed_res=FIXED, occ_res=OCC_RES if occ is not None else None,
                occupancy=occ_t, domain_mins=T(c['lo']), domain_maxs=T(c['hi'])), T(c['pts'])


# ------------------------------------------------------------------------------------------ forward
def check_forward(dev, arch, counts=COUNTS, occupancy=False):
    """-> raw, the reference, and a function giving the worst ratio of this raw against another (mutated) reference"""
    from xrnerf_amd import ops
    c = case(arch, counts)
    ref = reference(c, occupancy)
    a, pts = _scene_args(c, dev, occupancy)
    params = padded_blocks(c['mn'], dev)
    raw, cnt = ops.kilo_mlp_forward(a['viewdirs'], a['gmin'], a['gmax'], a['fixed_res'], a['occ_res'], a['occupancy'], a['domain_mins'],
                                    a['domain_maxs'], params, *arch, pts=pts, want_counts=True)
    raw = raw.reshape(-1, 4).cpu().numpy()
    designed = np.array([len(ref[n][0]) for n in range(N_NETS)])
    assert np.array_equal(cnt.cpu().numpy().astype(np.int64), designed), (cnt.cpu().numpy(), designed)
    if not occupancy:
        assert np.array_equal(designed, c['per']) and all(designed[n] == 0 for n in EMPTY)
    active = np.zeros(raw.shape[0], bool)

    def against(r):
        w = np.zeros(4)
        for n in range(N_NETS):
            slots, f = r[n]
            active[slots] = True
            for k in range(4):
                w[k] = max(w[k], ratio(raw[slots, k], f['raw'][:, k], f['e_raw'][:, k]))
        return w
    worst = against(ref)
    inactive = raw[~active]
    assert inactive.shape[0] >= 10 and np.array_equal(inactive.view(np.uint32), np.zeros_like(inactive, np.uint32))   # exactly +0
    log(dict(case='forward', arch=list(arch), occupancy=occupancy, samples=int(active.sum()), redrawn_share=c['redrawn_share'], share_within_1024u=c['share_within_1024u'],
             worst_ratio=dict(zip(('r', 'g', 'b', 'alpha'), worst.tolist()))))
    assert worst.max() <= 1.0, worst
    return raw, ref, against


# ------------------------------------------------------------------------------------------ backward
def ref_gradients(c, draw, occupancy=False, drop_sample=False, drop_feature=None, swap_rows=False):
    """float64 gradients and bounds of every parameter tensor, [N, ...] each, in ordered_parameters() order"""
    ref = reference(c, occupancy, drop_sample, drop_feature)
    ps = c['mn'].ordered_parameters()
    G = [np.zeros(tuple(p.shape)) for p in ps]
    E = [np.zeros(tuple(p.shape)) for p in ps]
    for n in range(N_NETS):
        slots, f = ref[n]
        if len(slots) == 0:
            continue
        g, e = R64.backward(c['nets'][n], f, draw[slots].astype(np.float64))
        for k in range(len(ps)):
            G[k][n], E[k][n] = g[k].reshape(G[k][n].shape), e[k].reshape(E[k][n].shape)
    if swap_rows:                                                     # mutation: two rows of one network's direction-layer gradient
        n = int(np.argmax(c['per'] == 33))
        G[-4][n][[3, 4]] = G[-4][n][[4, 3]]
    return G, E


def _compare_blocks(c, blocks, G, E, base=None):
    """worst ratio per parameter tensor of the gradient blocks against (G, E); base: the pattern the buffer held before (float64 blocks)"""
    from xrnerf_amd import kilo
    mn = c['mn']
    ps = mn.ordered_parameters()
    n_floats = mn.packed().shape[1]
    got = kilo.MultiNetwork.unpack_like(blocks[:, :n_floats].cpu(), ps)
    pat = None if base is None else kilo.MultiNetwork.unpack_like(base[:, :n_floats], ps)
    worst = {}
    for k, (name, _) in enumerate(mn.named_parameters()):
        g = got[k].numpy().astype(np.float64)
        if pat is None:
            worst[name] = ratio(g, G[k], E[k])
        else:
            p = pat[k].numpy().astype(np.float64)
            worst[name] = ratio(g, G[k] + p, E[k] + U * np.abs(p))
    return worst


def check_backward(dev, arch, counts=COUNTS):
    """Gradients of every entry of every tensor of every network within its own bound: into a zero-filled buffer, accumulated onto a known
    pattern (within bound + U |pattern|; the pattern is of magnitude 2^-12, below the gradient sums of the networks that take more than one
    atomic addition per entry, so that every rounding of the accumulation happens at the gradient's scale, which the bound covers),
    and through reuse_generation after a forward on the same samples.  dL/draw is standard normal on the active rows and NaN on the rows
    the documentation says are ignored; the padding floats keep their bits in every run."""
    from xrnerf_amd import ops
    c = case(arch, counts)
    ref = reference(c)
    a, pts = _scene_args(c, dev, False)
    params = padded_blocks(c['mn'], dev)
    n_samples = c['n_rays'] * S_PER_RAY
    draw = np.full((n_samples, 4), np.nan, np.float32)
    rng = np.random.default_rng(77)
    for n in range(N_NETS):
        draw[ref[n][0]] = rng.normal(0, 1, (len(ref[n][0]), 4)).astype(np.float32)
    G, E = ref_gradients(c, draw)
    draw_t = torch.from_numpy(draw.reshape(c['n_rays'], S_PER_RAY, 4)).to(dev)
    call = lambda **kw: ops.kilo_mlp_backward(draw_t, a['viewdirs'], a['gmin'], a['gmax'], a['fixed_res'], None, None, a['domain_mins'],
                                              a['domain_maxs'], params, *arch, pts=pts, **kw)
    pads = pad_mask(arch, params.shape[1])
    bits = lambda t: t.cpu().numpy().view(np.uint32)
    # 1. zero-filled buffer
    g0 = call()
    torch.cuda.synchronize()
    w0 = _compare_blocks(c, g0, G, E)
    assert not bits(g0)[:, pads].any()
    # 2. onto a known pattern (pads included)
    gen = torch.Generator().manual_seed(9)
    pattern = (torch.randn(tuple(params.shape), generator=gen) * 2.0 ** -12)
    buf = pattern.clone().to(dev)
    g1 = call(grad=buf)
    assert g1.data_ptr() == buf.data_ptr()
    w1 = _compare_blocks(c, g1, G, E, base=pattern.double())
    assert np.array_equal(bits(g1)[:, pads], bits(pattern)[:, pads])
    # 3. the forward's assignment reused
    ops.kilo_mlp_forward(a['viewdirs'], a['gmin'], a['gmax'], a['fixed_res'], None, None, a['domain_mins'], a['domain_maxs'], params, *arch, pts=pts)
    g2 = call(reuse_generation=ops.kilo_ws_generation())
    w2 = _compare_blocks(c, g2, G, E)
    assert not bits(g2)[:, pads].any()
    log(dict(case='backward', arch=list(arch), redrawn_share=c['redrawn_share'], share_within_1024u=c['share_within_1024u'], worst_ratio_zero_buffer=w0, worst_ratio_onto_pattern=w1,
             worst_ratio_reused_assignment=w2))
    for w in (w0, w1, w2):
        assert max(w.values()) <= 1.0, w
    return g0, draw, (G, E)


def check_refusals(dev):
    """architectures beyond the gradient kernels' register layout are refused by kilo_mlp_backward and student_step; nothing is written"""
    from xrnerf_amd import _lib, kilo_distill, ops
    import pytest
    lo, hi = domains()
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for arch in ARCH_REFUSED:
        mn = make_network(arch, N_NETS, 3)
        params = mn.packed().to(dev)
        rng = np.random.default_rng(4)
        pts, _ = _draw_in_cells(rng, np.repeat(np.arange(1, 8), 2), lo, hi)
        pts = T(pts.reshape(2, 7, 3))
        vd = T(np.float32([[0, 0, 1], [1, 0, 0]]))
        grad = torch.full_like(params, 7.0)
        with pytest.raises(_lib.XrError):
            ops.kilo_mlp_backward(torch.ones((2, 7, 4), device=dev), vd, GMIN, GMAX, FIXED, None, None, T(lo), T(hi), params, *arch, pts=pts, grad=grad)
        ex = torch.zeros((N_NETS, 4, 6), device=dev)
        loss, sgrad = torch.full((N_NETS,), 7.0, device=dev), torch.full_like(params, 7.0)
        before = params.clone()
        with pytest.raises(_lib.XrError):
            kilo_distill.student_step(ex, torch.zeros((N_NETS, 4, 4), device=dev), T(lo), T(hi), params, *arch, 0.05, loss=loss, grad=sgrad)
        torch.cuda.synchronize()
        assert bool((grad == 7.0).all()) and bool((sgrad == 7.0).all()) and bool((loss == 7.0).all()) and torch.equal(params, before)


# ------------------------------------------------------------------------------------------ students
ALPHA_DISTANCE = 0.0625


@functools.lru_cache(maxsize=None)
def student_case(arch, n_nets, batch, ex_stride, seed=2):
    """examples [N, B, ex_stride] inside boxes of the scene's grid (columns past 5: a filler the kernels skip), teacher raw [N, B, 4];
    examples next to a relu kink or to the alpha pre-activation's leaky_relu kink are redrawn like the scene's points"""
    lo, hi = domains()
    boxes = np.array([5, 14, 22][:n_nets] if n_nets > 1 else [9])
    mn = make_network(arch, n_nets, seed + 10)
    nets = ref_nets(mn)
    rng = np.random.default_rng(1000 * seed + batch)
    ex = rng.normal(0, 1, (n_nets, batch, ex_stride)).astype(np.float32) + 5.0
    redrawn, near_plain = np.zeros((n_nets, batch), bool), np.zeros((n_nets, batch), bool)

    def draw(n, k):
        p, _ = _draw_in_cells(rng, np.full(k, boxes[n]), lo, hi)
        d = rng.normal(0, 1, (k, 3))
        return p, (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    fwd = []
    for n in range(n_nets):
        ex[n, :, 0:3], ex[n, :, 3:6] = draw(n, batch)
        for rnd in range(16):
            f = R64.forward(nets[n], R64.local_x(ex[n, :, 0:3], lo[boxes[n]], hi[boxes[n]]), ex[n, :, 3:6])
            if rnd == 0:
                near_plain[n] = f['plain_margin'] < 1024.0
            bad = np.flatnonzero(np.minimum(f['margin'], f['alpha_margin']) < MIN_KINK_MARGIN)
            if len(bad) == 0:
                break
            redrawn[n, bad] = True
            ex[n, bad, 0:3], ex[n, bad, 3:6] = draw(n, len(bad))
        assert len(bad) == 0
        fwd.append(f)
    share = float(redrawn.mean())
    teacher = rng.normal(0, 1, (n_nets, batch, 4)).astype(np.float32)
    return dict(arch=arch, mn=mn, nets=nets, ex=ex, teacher=teacher, lo=lo[boxes], hi=hi[boxes], fwd=fwd, redrawn_share=share, redrawn=int(redrawn.sum()), near_plain=int(near_plain.sum()), points=int(redrawn.size))


def _student_reference(s, batch_for_scale=None, without_examples=None):
    """per network: loss with bound, gradient blocks (float64 tensors per parameter [N, ...]) with bounds"""
    ps = s['mn'].ordered_parameters()
    G = [np.zeros(tuple(p.shape)) for p in ps]
    E = [np.zeros(tuple(p.shape)) for p in ps]
    loss, e_loss = np.zeros(len(s['nets'])), np.zeros(len(s['nets']))
    for n, net in enumerate(s['nets']):
        L = R64.student_loss(s['fwd'][n], s['teacher'][n], ALPHA_DISTANCE, batch_for_scale)
        loss[n], e_loss[n] = L['loss'], L['e_loss']
        if without_examples is not None:                               # mutation: these examples contribute no gradient
            L['draw'][without_examples] = 0.0
        g, e = R64.backward(net, s['fwd'][n], L['draw'], L['e_draw'])
        for k in range(len(ps)):
            G[k][n], E[k][n] = g[k].reshape(G[k][n].shape), e[k].reshape(E[k][n].shape)
    return loss, e_loss, G, E


def _blocks_worst(mn, blocks, G, E):
    from xrnerf_amd import kilo
    ps = mn.ordered_parameters()
    got = kilo.MultiNetwork.unpack_like(blocks[:, :mn.packed().shape[1]].cpu(), ps)
    return {name: ratio(got[k].numpy(), G[k], E[k]) for k, (name, _) in enumerate(mn.named_parameters())}


def _tensor_floats(mn, k):
    """mask over a block's floats: those of parameter tensor k"""
    from xrnerf_amd import kilo
    which = kilo.MultiNetwork.pack([torch.full_like(p, float(j + 1)) for j, p in enumerate(mn.ordered_parameters())]).numpy().astype(np.int64)
    return which[0] == k + 1


def _pack64(mn, tensors):
    """float64 per-parameter arrays -> float64 blocks in the packed layout (pads zero)"""
    from xrnerf_amd import kilo
    ps = mn.ordered_parameters()
    n_floats = mn.packed().shape[1]
    idx = kilo.MultiNetwork.pack([torch.arange(1, p[0].numel() + 1, dtype=torch.float32).reshape(p[0].shape).expand_as(p) for p in ps])
    assert idx.shape[1] == n_floats
    out = np.zeros((ps[0].shape[0], n_floats))
    # entry j of the block <- element (index - 1) of the tensor the offset falls into, found by packing per-tensor markers
    which = kilo.MultiNetwork.pack([torch.full_like(p, float(k + 1)) for k, p in enumerate(ps)]).numpy().astype(np.int64)
    for k, t in enumerate(tensors):
        m = which[0] == k + 1
        flat = np.asarray(t).reshape(t.shape[0], -1)
        out[:, m] = flat[:, idx[0].numpy().astype(np.int64)[m] - 1]
    return out


def check_student(dev, arch, batch, n_nets, ex_stride):
    """loss and every gradient entry of k_kilo_student_step, raw and rendered output of k_kilo_student_fwd (with and without domains), and
    the fused Adam update (step 1 from zero moments, step 7 from given moments) against float64 Adam on the float64 gradient"""
    from xrnerf_amd import kilo_distill as KD
    s = student_case(arch, n_nets, batch, ex_stride)
    mn = s['mn']
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ex, teacher, lo, hi = T(s['ex']), T(s['teacher']), T(s['lo']), T(s['hi'])
    params = padded_blocks(mn, dev)
    params0 = params.clone()
    pads = pad_mask(arch, params.shape[1])
    bits = lambda t: t.cpu().numpy().view(np.uint32)
    loss_ref, e_loss, G, E = _student_reference(s)
    rec = dict(case='student', arch=list(arch), batch=batch, n_nets=n_nets, ex_stride=ex_stride, redrawn_share=s['redrawn_share'])
    # ---- forward: raw and rendered, global positions with domains, local positions without
    raw_ref = np.stack([f['raw'] for f in s['fwd']])
    e_raw = np.stack([f['e_raw'] for f in s['fwd']])
    ren = [R64.student_render(f['raw'], f['e_raw'], ALPHA_DISTANCE) for f in s['fwd']]
    local = s['ex'].copy()
    for n in range(n_nets):
        local[n, :, 0:3] = R64.local_x(s['ex'][n, :, 0:3], s['lo'][n], s['hi'][n])
    for tag, e_in, kw in (('domains', ex, dict(domain_mins=lo, domain_maxs=hi)), ('local', T(local), {})):
        raw = KD.student_forward(e_in, params, *arch, **kw).cpu().numpy()
        rgba = KD.student_forward(e_in, params, *arch, render=True, alpha_distance=ALPHA_DISTANCE, **kw).cpu().numpy()
        rec['fwd_raw_' + tag] = ratio(raw, raw_ref, e_raw)
        rec['fwd_rendered_' + tag] = ratio(rgba, np.stack([r[0] for r in ren]), np.stack([r[1] for r in ren]))
    # ---- the step without Adam: loss and gradient
    grad = torch.full_like(params, 7.0)
    loss, g = KD.student_step(ex, teacher, lo, hi, params, *arch, ALPHA_DISTANCE, grad=grad)
    torch.cuda.synchronize()
    assert torch.equal(params, params0)
    rec['loss'] = ratio(loss.cpu().numpy(), loss_ref, e_loss)
    rec['grad'] = _blocks_worst(mn, g, G, E)
    n_floats = mn.packed().shape[1]
    assert bool((g[:, n_floats:] == 7.0).all())                       # the stride padding is never written
    g_bits = bits(g)[:, :n_floats].copy()
    # ---- Adam: step 1 from zero moments, step 7 from given moments; grad=None at batch <= 128, passed beyond
    G64, E64 = _pack64(mn, G), _pack64(mn, E)
    live = ~pads[:n_floats]
    hyper = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8)
    gen = torch.Generator().manual_seed(batch)
    for step in (1, 7):
        p = params0.clone()
        if step == 1:
            m, v = torch.zeros_like(p), torch.zeros_like(p)
        else:
            m = (torch.randn(tuple(p.shape), generator=gen) * 1e-2).to(dev)
            v = (torch.rand(tuple(p.shape), generator=gen) * 1e-3 + 1e-6).to(dev)
            keep = torch.from_numpy(~pads).to(dev)                     # the moments of a float without a parameter never left zero
            keep[n_floats:] = True                                     # (the stride padding may hold anything: it is not touched)
            m, v = (m * keep).contiguous(), (v * keep).contiguous()
        m0, v0 = m.clone(), v.clone()
        gout = None if batch <= 128 else torch.full_like(p, 7.0)
        loss2, g2 = KD.student_step(ex, teacher, lo, hi, p, *arch, ALPHA_DISTANCE, grad=gout, adam=dict(m=m, v=v, step=step, **hyper))
        torch.cuda.synchronize()
        assert np.array_equal(bits(loss2), bits(loss))
        if gout is not None:
            assert np.array_equal(bits(g2)[:, :n_floats], g_bits)        # the gradient written beside the update: the no-Adam call's bits
        else:
            assert g2 is None
        f64 = lambda t: t.cpu().numpy().astype(np.float64)[:, :n_floats]
        (pr, e_p), (mr, e_m), (vr, e_v) = R64.adam(f64(params0), f64(m0), f64(v0), G64, E64, step, hyper['lr'], *hyper['betas'], hyper['eps'])
        if step == 1:
            adam1 = dict(p=f64(p), p0=f64(params0), e_p=e_p)
        rec['adam_step%d' % step] = dict(p=ratio(f64(p)[:, live], pr[:, live], e_p[:, live]), m=ratio(f64(m)[:, live], mr[:, live], e_m[:, live]),
                                         v=ratio(f64(v)[:, live], vr[:, live], e_v[:, live]))
        # floats that hold no parameter: the stride padding is untouched, the pads inside the block see a zero gradient
        for new, old in ((p, params0), (m, m0), (v, v0)):
            assert np.array_equal(bits(new)[:, n_floats:], bits(old)[:, n_floats:])
        assert np.array_equal(bits(p)[:, pads], bits(params0)[:, pads])
    log(rec)
    flat = [rec['loss']] + list(rec['grad'].values()) + [rec[k] for k in rec if k.startswith('fwd_')]
    flat += [x for st in (1, 7) for x in rec['adam_step%d' % st].values()]
    assert max(flat) <= 1.0, rec
    return g, (G, E), adam1


def check_student_arch(dev, arch, batches=BATCHES, combos=((1, 6), (3, 10), (1, 10), (3, 6))):
    """every batch size at every (network count, example stride); the redrawn share is taken over the architecture's examples together (a
    batch of one has no share of its own)"""
    redrawn = near = points = 0
    for batch in batches:
        for n_nets, ex_stride in combos:
            check_student(dev, arch, batch, n_nets, ex_stride)
            s = student_case(arch, n_nets, batch, ex_stride)
            redrawn, near, points = redrawn + s['redrawn'], near + s['near_plain'], points + s['points']
    log(dict(case='student_redrawn', arch=list(arch), redrawn_share=redrawn / points, share_within_1024u=near / points, points=points))
    assert redrawn / points < 0.10, (redrawn, points)


# ------------------------------------------------------------------------------------------ the bars bite
def check_mutations(dev, counts=COUNTS, batch=129, batch2=257, fwd_archs=((11, 5, 3), (16, 16, 8))):
    """Mutations of the REFERENCE side only: the kernel's (correct) output must then lie outside the bar."""
    from xrnerf_amd import kilo
    arch = (5, 3, 2)
    c = case(arch, counts)
    g0, draw, (G, E) = check_backward(dev, arch, counts)
    names = [n for n, _ in c['mn'].named_parameters()]
    out = {}
    # one sample removed from the 129-sample network
    Gm, Em = ref_gradients(c, draw, drop_sample=True)
    out['sample_removed'] = max(_compare_blocks(c, g0, Gm, Em).values())
    # the top position frequency's sine row dropped (every channel)
    Gm, Em = ref_gradients(c, draw, drop_feature=(None, 'sin', arch[0] - 1))
    out['sine_row_dropped'] = max(_compare_blocks(c, g0, Gm, Em).values())
    # two rows of one network's direction-layer gradient swapped
    Gm, Em = ref_gradients(c, draw, swap_rows=True)
    w = _compare_blocks(c, g0, Gm, Em)
    out['rows_swapped'] = w['direction_layer.weight']
    assert all(v <= 1.0 for k, v in w.items() if k != 'direction_layer.weight')
    # ---- the students, per tensor group
    g, (G, E), _ = check_student(dev, arch, batch, 1, 6)
    s = student_case(arch, 1, batch, 6)
    # dscale taken with batch + 1: every tensor's gradient is off by 1 / (batch + 1)
    _, _, Gm, Em = _student_reference(s, batch_for_scale=batch + 1)
    w = _blocks_worst(s['mn'], g, Gm, Em)
    out['dscale_batch_plus_1'] = w
    # the second round's contribution removed (batch > 128: examples 128 .. 255 reach the gradient only through `grad`)
    big = batch2
    g2, _, adam1 = check_student(dev, arch, big, 1, 6)
    s2 = student_case(arch, 1, big, 6)
    _, _, Gm, _ = _student_reference(s2, without_examples=slice(128, 256))
    _, _, _, E2 = _student_reference(s2)
    w2 = _blocks_worst(s2['mn'], g2, Gm, E2)
    out['second_round_removed'] = w2
    # Adam not applied to one hidden-layer tensor: the reference keeps the old parameters there
    k = names.index('pts_linears.1.weight')
    fl = _tensor_floats(s2['mn'], k)
    out['adam_skipped_on_pts_linears.1.weight'] = ratio(adam1['p'][:, fl], adam1['p0'][:, fl], adam1['e_p'][:, fl])
    # ---- the forward at the deep architectures: the bias of hidden layer 1 dropped in the reference
    for fa in fwd_archs:
        _, _, against = check_forward(dev, fa, counts)
        out['forward_bias_dropped_%d_%d_%d' % fa] = float(against(reference(case(fa, counts), drop_bias=1)).max())
    log(dict(case='mutations', arch=list(arch), worst_ratio_against_mutated_reference=out))
    # (the second round may hold a single example whose alpha gradient is next to nothing: that mutation is asserted on the hidden layers)
    flat = [x for key, v in out.items() for n, x in (v.items() if isinstance(v, dict) else [('', v)])
            if key != 'second_round_removed' or n.startswith('pts_linears.')]
    assert all(x > 1.0 for x in flat), out
