"""NeuralBody on the MI355X (xrnerf_amd/csrc/xr_neuralbody.hip behind xrnerf_amd/neuralbody.py).  The check_* bodies take the device, so
tests/test_emu_neuralbody.py runs the same bodies on the kernels' host build.

References: the float64 dense restatement (tests/neuralbody_restatement.py) and its autograd; the fixture step of the reference's own
modules (tests/golden/ref_neuralbody.npz, expected values = its float64 run).

Bars.  Convolution and sampling: 4 x the deviation of the float32 restatement from the float64 restatement on the same case, computed
here, with a floor of 2^-22 max|ref| -- the kernels' exact-product fp32 arithmetic differs from torch's only in summation order, so
torch's own float32 error is the scale.  Structure: exact.  Fixture step: every quantity 4 x the float32-against-float64 deviation
the generator recorded for it (`dev.*`); `raw` is held to grad_bars.RAW_BAR as long as the reference's own float32 run meets it (its
recorded deviation is 2.3e-6 of max|raw|, under RAW_BAR = 4e-6), and to the 4 x rule only if it did not.  The features' bars carry
2^-24 max|ref| more, because the fixture stores the float64 features rounded to float32.  A gradient's 2-norm is held to 4 x the
relative 2-norm of the reference's whole float32 difference: an upper bound on the norms' difference, so that check catches gross
errors only (a wrong scale, a missing term) and the sampled entries carry the weight.  Every check prints its worst figure next to
its bar."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')

STRUCT_V = (1, 63, 65, 257)
STRUCT_SH = ((32, 32, 32), (32, 64, 32), (64, 32, 96))
# 1 179 648 cells = 288 count workgroups: the scan of their counts takes 256 per sweep, so the far-corner voxel's workgroup gets a carry
STRUCT_TWO_SWEEPS = (257, (96, 128, 96))
# every (Cin, Cout, strided) of the network
CONV_LAYERS = ((16, 16, False), (32, 32, False), (64, 64, False), (128, 128, False), (16, 32, True), (32, 64, True), (64, 128, True),
               (128, 128, True))
CONV_N = (1, 63, 65, 300)
CONV_DIMS = (12, 10, 14)          # the tables come from the restatement here, so the volume may be small: the float64 dense conv3d stays quick
SAMPLE_N = (1, 63, 65, 1000)
SAMPLE_SH = (32, 64, 32)
FLOOR = 2.0 ** -22


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_neuralbody.npz'))


def model_cfg():
    return json.load(open(os.path.join(G, 'neuralbody_model_cfg.json')))['model']


def bar_of(q32, q64):
    q64 = np.asarray(q64, np.float64)
    scale = float(np.abs(q64).max()) if q64.size else 0.0
    dev = float(np.abs(np.asarray(q32, np.float64) - q64).max()) if q64.size else 0.0
    return max(4.0 * dev, FLOOR * scale), scale


def held(got, q32, q64, what):
    """max |got - float64| within 4 x the float32 restatement's own deviation (floor 2^-22 max|ref|)"""
    got = np.asarray(got, np.float64)
    q64 = np.asarray(q64, np.float64)
    assert got.shape == q64.shape and np.isfinite(got).all(), what
    bar, scale = bar_of(q32, q64)
    worst = float(np.abs(got - q64).max()) if q64.size else 0.0
    print('%s: worst %.3e, bar %.3e (of max|ref| %.3e: %.2e, %.2e)' % (what, worst, bar, scale, worst / max(scale, 1e-300), bar / max(scale, 1e-300)))
    assert worst <= bar, (what, worst, bar)
    return worst


# ------------------------------------------------------------------------------------------ structure
def structure_coords(V, out_sh, seed=0):
    """V voxel coordinates (z, y, x): the far corner (dim - 1 on every axis), cell 0, duplicates of both, then a cluster (odd and even
    coordinates, duplicates by themselves); V = 1 is the single far-corner voxel"""
    rng = np.random.default_rng([V, seed] + list(out_sh))
    sh = np.array(out_sh)
    c = np.clip(np.rint(sh / 2 + rng.normal(0, 3.0, (V, 3))), 0, sh - 1).astype(np.int32)
    fixed = [sh - 1, np.zeros(3), sh - 1, np.zeros(3), sh - 2, np.ones(3)]
    for i, f in enumerate(fixed[:V]):
        c[i] = f
    return c


def check_structure(dev, V, out_sh):
    import neuralbody_restatement as RS
    from xrnerf_amd import neuralbody as NB
    coord = structure_coords(V, out_sh)
    frame = NB.build_frame(torch.as_tensor(coord).to(dev), out_sh)
    assert frame.kernels, 'the structure did not come from the kernels'
    rows, vert_row = RS.all_rows(coord, out_sh)
    assert frame.n == [int(r.shape[0]) for r in rows], (frame.n, [int(r.shape[0]) for r in rows])
    assert len(np.unique(coord, axis=0)) < V or V < 3
    assert np.array_equal(frame.vert_row.cpu().numpy(), vert_row.numpy())
    for l in range(RS.LEVELS):
        dims = RS.dims_of(out_sh, l)
        assert np.array_equal(frame.rows[l].cpu().numpy(), rows[l].numpy()), ('rows', l)
        assert np.array_equal(frame.vols[l].cpu().numpy(), RS.index_volume(rows[l], dims).numpy()), ('index volume', l)
        assert np.array_equal(frame.subm[l].cpu().numpy(), RS.subm_table(rows[l], dims).numpy()), ('subm table', l)
        if l + 1 < RS.LEVELS:
            o, i = RS.down_tables(rows[l], dims, rows[l + 1])
            assert np.array_equal(frame.down_out[l].cpu().numpy(), o.numpy()), ('output-stationary table', l)
            assert np.array_equal(frame.down_in[l].cpu().numpy(), i.numpy()), ('input-stationary table', l)
    # the tensor-op rulebook agrees too
    old = NB.tensor_op_path(True)
    try:
        ft = NB.build_frame(torch.as_tensor(coord).to(dev), out_sh)
    finally:
        NB.tensor_op_path(old)
    assert not ft.kernels
    for l in range(RS.LEVELS):
        assert np.array_equal(ft.rows[l].cpu().numpy(), rows[l].numpy()) and np.array_equal(ft.subm[l].cpu().numpy(), frame.subm[l].cpu().numpy())
    for l in range(RS.LEVELS - 1):
        assert np.array_equal(ft.down_out[l].cpu().numpy(), frame.down_out[l].cpu().numpy())
        assert np.array_equal(ft.down_in[l].cpu().numpy(), frame.down_in[l].cpu().numpy())


def check_structure_errors(dev):
    """a bad out_sh and a volume over the cap come back as XR_E* and launch nothing (the sentinel counts stay)"""
    import ctypes as C
    from xrnerf_amd import _lib, ops
    lib = _lib.load()
    coord = torch.zeros((4, 3), dtype=torch.int32, device=dev)
    vol = torch.full((64,), 7, dtype=torch.int32, device=dev)
    rows = torch.full((64,), 7, dtype=torch.int32, device=dev)
    vert_row = torch.full((4,), 7, dtype=torch.int32, device=dev)
    counts = torch.full((5,), 7, dtype=torch.int32, device=dev)
    ws = torch.zeros((1 << 16,), dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    for sh in ((33, 32, 32), (32, 48, 32), (0, 32, 32), (1024, 1024, 128)):
        rc = lib.xr_nb_build_rows(p(coord), 4, sh[0], sh[1], sh[2], p(vol), p(rows), p(vert_row), p(counts), p(ws), ws.numel(), ops._stream())
        assert rc < 0, (sh, rc)
        assert int(lib.xr_nb_build_rows_workspace_bytes(*sh)) == 0
        with pytest.raises(_lib.XrError):
            ops.nb_layout(4, sh)
        with pytest.raises((_lib.XrError, ValueError)):
            from xrnerf_amd import neuralbody as NB
            NB.build_frame(coord, sh)
    torch.cuda.synchronize()
    for t in (vol, rows, vert_row, counts):
        assert bool((t == 7).all())
    assert ops.NB_MAX_CELLS >= 6 * 128 * 224 * 384


def check_no_vertices(dev):
    """V = 0: five empty levels -- cleared index volumes, zero counts, empty tables -- not uninitialised memory"""
    from xrnerf_amd import ops
    out_sh = (32, 64, 32)
    vols, rows, vert_row, n = ops.nb_build_rows(torch.zeros((0, 3), dtype=torch.int32, device=dev), out_sh)
    assert n == [0] * 5 and vert_row.numel() == 0 and all(r.numel() == 0 for r in rows)
    assert sum(v.numel() for v in vols) == sum((32 * 64 * 32) >> (3 * l) for l in range(5))
    assert all(bool((v == -1).all()) for v in vols)
    assert tuple(ops.nb_subm_table(vols[0], rows[0], out_sh).shape) == (0, 27)


# ------------------------------------------------------------------------------------------ convolution
def conv_rows(N, dims, seed=0):
    """N distinct active cells of a level with `dims`: N = 1 is a lone voxel (only the centre tap contributes); otherwise a full
    3 x 3 x 3 block (all 27 taps), the volume's eight corners, and a cluster"""
    D, H, W = dims
    rng = np.random.default_rng([N, seed])
    if N == 1:
        return torch.tensor([((D // 2 + 1) * H + H // 2) * W + W // 2 + 1])
    cells = set()
    for z in range(3):
        for y in range(3):
            for x in range(3):
                cells.add(((z + 2) * H + y + 3) * W + x + 4)
    for z in (0, D - 1):
        for y in (0, H - 1):
            for x in (0, W - 1):
                cells.add((z * H + y) * W + x)
    while len(cells) < N:
        z, y, x = (int(v) for v in np.clip(np.rint(np.array(dims) / 2 + rng.normal(0, 2.5, 3)), 0, np.array(dims) - 1))
        cells.add((z * H + y) * W + x)
    return torch.tensor(sorted(cells)[:N] if len(cells) > N else sorted(cells))


def check_conv(dev, cin, cout, strided, N):
    import neuralbody_restatement as RS
    from xrnerf_amd import ops
    dims = CONV_DIMS
    rows = conv_rows(N, dims)
    rng = np.random.default_rng([cin, cout, int(strided), N])
    x = rng.normal(0, 1, (rows.shape[0], cin)).astype(np.float32)
    w = (rng.normal(0, 1, (cout, 3, 3, 3, cin)) * np.sqrt(2.0 / (27 * cin))).astype(np.float32)
    if strided:
        rows_out = RS.down_rows(rows, dims)
        tab, back = RS.down_tables(rows, dims, rows_out)
    else:
        rows_out = rows
        tab = back = RS.subm_table(rows, dims)
    g = rng.normal(0, 1, (rows_out.shape[0], cout)).astype(np.float32)
    if N == 1 and not strided:
        assert int((tab >= 0).sum()) == 1 and int(tab[0, 13]) == 0            # the lone voxel: only the centre tap
    if N > 1:
        assert bool((RS.subm_table(rows, dims) >= 0).all(1).any())            # the block's centre has all 27 taps

    def restated(dtype):
        xs = torch.as_tensor(x).to(dtype).requires_grad_(True)
        ws = torch.as_tensor(w).to(dtype).requires_grad_(True)
        y = RS.strided_conv(xs, rows, dims, ws)[0] if strided else RS.subm_conv(xs, rows, dims, ws)
        (y * torch.as_tensor(g).to(dtype)).sum().backward()
        return y.detach().numpy(), xs.grad.numpy(), ws.grad.numpy()
    y64, dx64, dw64 = restated(torch.float64)
    y32, dx32, dw32 = restated(torch.float32)
    t = lambda a: torch.as_tensor(a).to(dev)
    xd, wd, gd = t(x), t(w), t(g)
    tabd, backd = t(tab.int().numpy()), t(back.int().numpy())
    y = ops.nb_conv(xd, tabd, wd)
    dx = ops.nb_conv(gd, backd, wd, transposed=True, flip=not strided)
    dw = ops.nb_conv_weight_grad(xd, tabd, gd)
    torch.cuda.synchronize()
    tag = '%d->%d %s N=%d' % (cin, cout, 'strided' if strided else 'subm', N)
    held(y.cpu().numpy(), y32, y64, 'conv forward ' + tag)
    held(dx.cpu().numpy(), dx32, dx64, 'conv input gradient ' + tag)
    held(dw.cpu().numpy(), dw32, dw64, 'conv weight gradient ' + tag)
    assert torch.equal(ops.nb_conv(xd, tabd, wd), y) and torch.equal(ops.nb_conv_weight_grad(xd, tabd, gd), dw)


# ------------------------------------------------------------------------------------------ sampling
def sample_levels(out_sh, seed=0):
    """random active sets and rows for the four sampled levels: a blob around the centre, the half z < D / 3 left empty"""
    import neuralbody_restatement as RS
    rng = np.random.default_rng([seed] + list(out_sh))
    rows, feats = [], []
    for l in range(1, RS.LEVELS):
        D, H, W = RS.dims_of(out_sh, l)
        z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
        keep = (rng.uniform(0, 1, (D, H, W)) < 0.4) & (z >= D // 3)
        keep[D - 1, H - 1, W - 1] = True
        keep[D - 1, 0, 0] = True
        r = torch.as_tensor(np.flatnonzero(keep.reshape(-1)))
        rows.append(r)
        feats.append(rng.normal(0, 1, (r.shape[0], RS.CHANNELS[l - 1])).astype(np.float32))
    return rows, feats


def _sample_case(dev, pts, R, T, mn, voxel, out_sh, strided_out, what):
    import neuralbody_restatement as RS
    from xrnerf_amd import ops
    rows, feats = sample_levels(out_sh)
    N = pts.shape[0]
    rng = np.random.default_rng([N, 17])
    gout = rng.normal(0, 1, (N, 352)).astype(np.float32)

    def restated(dtype):
        fs = [torch.as_tensor(f).to(dtype).requires_grad_(True) for f in feats]
        c = lambda a: torch.as_tensor(a).to(dtype)
        out = RS.sample(fs, rows, out_sh, RS.grid(c(pts), c(R), c(T), c(mn), voxel, out_sh))
        (out * c(gout)).sum().backward()
        return out.detach().numpy(), [f.grad.numpy() for f in fs]
    o64, g64 = restated(torch.float64)
    o32, g32 = restated(torch.float32)
    dead = []
    for l in range(4):
        dims = RS.dims_of(out_sh, l + 1)
        grown = torch.nn.functional.max_pool3d(RS.mask_of(rows[l], dims)[None, None].double(), 3, 1, 1)
        c64 = lambda a: torch.as_tensor(a).double()
        g = RS.grid(c64(pts), c64(R), c64(T), c64(mn), voxel, out_sh)
        near = torch.nn.functional.grid_sample(grown, g[None, None, None], padding_mode='zeros', align_corners=True)[0, 0, 0, 0]
        dead.append((near == 0).numpy())
    assert N < 60 or any(d.any() for d in dead)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    vols = [t(RS.index_volume(rows[l], RS.dims_of(out_sh, l + 1)).int().numpy()) for l in range(4)]
    fd = [t(f) for f in feats]
    args = (t(pts), t(R), t(T), t(mn), voxel, out_sh, vols)
    if strided_out:
        buf = torch.full((N, 364), 5.0, dtype=torch.float32, device=dev)
        out = ops.nb_sample_forward(*args, fd, out=buf)[:, :352]
        assert bool((buf[:, 352:] == 5.0).all())
        gbuf = torch.zeros((N, 360), dtype=torch.float32, device=dev)
        gbuf[:, :352] = t(gout)
        grad = gbuf[:, :352]
    else:
        out = ops.nb_sample_forward(*args, fd)
        grad = t(gout)
    n_rows = [int(r.shape[0]) for r in rows]
    gs = ops.nb_sample_backward(*args, n_rows, grad)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    c0 = 0
    for l, ch in enumerate(RS.CHANNELS):
        s = slice(c0, c0 + ch)
        held(got[:, s], o32[:, s], o64[:, s], '%s forward level %d' % (what, l + 1))
        # a point with no active corner at a level: exact zeros.  (Decided on the active set grown by one cell, so that a point within
        # rounding of a cell boundary, whose fp32 corners may be the neighbouring cells, is not asked for more than its tolerance)
        assert not got[:, s][dead[l]].any(), (what, 'rows without an active corner must be exact zeros', l + 1)
        assert not o64[:, s][dead[l]].any()
        held(gs[l].cpu().numpy(), g32[l], g64[l], '%s row gradient level %d' % (what, l + 1))
        c0 += ch
    # a second launch repeats the bits
    out2 = ops.nb_sample_forward(*args, fd)
    gs2 = ops.nb_sample_backward(*args, n_rows, grad)
    assert torch.equal(out2, out.contiguous()) and all(torch.equal(a, b) for a, b in zip(gs, gs2))
    return o64


def check_sampling(dev, N, strided_out):
    """random points in a posed frame, a fifth of them outside the volume on one side or another"""
    out_sh = SAMPLE_SH
    rng = np.random.default_rng([N, int(strided_out)])
    voxel = 0.05
    from xrnerf_amd.aninerf import _rot
    R = _rot(rng.normal(0, 1, 3), 0.7).astype(np.float32)
    T = rng.normal(0, 0.3, 3).astype(np.float32)
    mn = rng.normal(0, 0.2, 3).astype(np.float32)
    ext = np.array([out_sh[2], out_sh[1], out_sh[0]]) * voxel
    q = mn + rng.uniform(-0.15, 1.15, (N, 3)) * ext
    pts = (q @ R.T.astype(np.float64) + T).astype(np.float32)
    _sample_case(dev, pts, R, T, mn, voxel, out_sh, strided_out, 'sampling N=%d%s' % (N, ' strided' if strided_out else ''))


def check_sampling_edges(dev):
    """identity pose, voxel 1, min_xyz 0, so that the normalised coordinate is exact: points exactly at -1 and +1, on the cell
    boundaries of every level, outside on each side, and inside the empty part of the volume (all eight corners empty)"""
    out_sh = SAMPLE_SH
    W, H, D = out_sh[2], out_sh[1], out_sh[0]
    sh = np.array([W, H, D], np.float64)
    pts = [[0, 0, 0], [W, H, D], [0, H, 0], [W, 0, D], [W / 2, H / 2, D / 2]]
    for side in range(3):
        for v in (-0.5, -3.0, 1.01, 1.5):
            p = [W / 2, H / 2, D * 0.8]
            p[side] = v * sh[side]
            pts.append(p)
    for l in range(1, 5):                                   # f = c' (size_l - 1) an integer: cell boundaries of level l
        for i in (0, 1, 2, 5):
            pts.append([min(i, (W >> l) - 1) / ((W >> l) - 1) * W, min(i + 1, (H >> l) - 1) / ((H >> l) - 1) * H, D * 0.9])
    rng = np.random.default_rng(3)
    for _ in range(12):                                     # the empty low-z part of the volume
        pts.append([rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0, D * 0.1)])
    pts = np.array(pts, np.float32)
    R, T, mn = np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    o64 = _sample_case(dev, pts, R, T, mn, 1.0, out_sh, False, 'sampling edges')
    assert (o64[-12:, :96] == 0).all() and (o64[:5] != 0).any()          # (levels 1 and 2: the coarser ones reach an active plane)


# ------------------------------------------------------------------------------------------ fixture step
def network(dev, gold, dtype=torch.float32):
    import neuralbody_restatement as RS
    import xrnerf_amd
    cfg = copy.deepcopy(model_cfg())
    cfg['cfg']['smpl_embedder']['voxel_size'] = [float(gold['voxel'])] * 3
    net = xrnerf_amd.build_network(cfg)
    keys = [str(k) for k in gold['sd_keys']]
    shapes = [tuple(json.loads(str(s))) for s in gold['sd_shapes']]
    net.load_state_dict(RS.formula_state_dict(keys, shapes, int(gold['seed'])), strict=True)
    return net.to(dev).to(dtype)


def batch(dev, gold, batched=False):
    """the fixture's `datas`; batched: with the data loader's leading batch axis of 1, which train_step / val_step unfold"""
    d = {k[3:]: torch.as_tensor(gold[k]).to(dev) for k in gold.files if k.startswith('in.')}
    return {k: v[None] for k, v in d.items()} if batched else d


def fixture_bar(gold, name, scale, floor=0.0):
    return max(4.0 * float(gold['dev.' + name]), floor) * scale


def one_step(dev, gold):
    net = network(dev, gold)
    net.zero_grad()
    out = net.train_step(batch(dev, gold, True), None)
    out['loss'].backward()
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    return net, out


def check_fixture_step(dev, gold, repeat=True, expect_kernels=True, first=None):
    """first: the (net, out) of a step already made (the emulated tier counts the launches of the same step)"""
    import grad_bars
    import neuralbody_restatement as RS
    from xrnerf_amd import neuralbody as NB
    net, out = one_step(dev, gold) if first is None else first
    datas = batch(dev, gold)
    coord, out_sh, _ = net.smpl_conv.prepare(datas)
    assert list(out_sh) == [int(v) for v in gold['out_sh']]
    frame = NB.build_frame(coord, out_sh)
    assert frame.kernels == expect_kernels
    for l in range(RS.LEVELS):
        assert np.array_equal(frame.rows[l].cpu().numpy(), gold['rows.%d' % l]), ('rows of level', l)
    ret = out['ret']
    feats, ref = ret['xyzc_features'].detach().cpu().numpy().astype(np.float64), gold['features'].astype(np.float64)
    c0, worst = 0, {}
    for l, ch in enumerate(RS.CHANNELS):
        s = slice(c0, c0 + ch)
        scale = np.abs(ref[:, s]).max()
        # (the stored features are the float64 run's rounded to float32: 2^-24 of each value on top of the bar)
        bar = fixture_bar(gold, 'features.%d' % (l + 1), scale) + 2.0 ** -24 * scale
        worst['features.%d' % (l + 1)] = w = np.abs(feats[:, s] - ref[:, s]).max()
        print('features level %d: worst %.3e of max|ref|, bar %.3e' % (l + 1, w / scale, bar / scale))
        assert w <= bar, ('features', l + 1, w / scale, bar / scale)
        c0 += ch
    raw, raw_ref = ret['raw'].detach().cpu().numpy().astype(np.float64), gold['raw']
    scale = np.abs(raw_ref).max()
    # RAW_BAR as long as the reference's own float32 run meets it; the 4 x rule only if that run itself is over RAW_BAR
    recorded = float(gold['dev.raw'])
    raw_bar = grad_bars.RAW_BAR if recorded <= grad_bars.RAW_BAR else 4.0 * recorded
    w = np.abs(raw - raw_ref).max() / scale
    print('raw: worst %.3e of max|raw|, bar %.3e (RAW_BAR %.1e, recorded %.3e)' % (w, raw_bar, grad_bars.RAW_BAR, recorded))
    assert w <= raw_bar, ('raw', w, raw_bar)
    rgb, rgb_ref = ret['rgb'].detach().cpu().numpy().astype(np.float64), gold['rgb']
    w = np.abs(rgb - rgb_ref).max() / np.abs(rgb_ref).max()
    print('rgb: worst %.3e of max|rgb|, bar %.3e' % (w, 4 * float(gold['dev.rgb'])))
    assert w <= 4 * float(gold['dev.rgb']), ('rgb', w)
    w = abs(float(out['loss'].item()) - float(gold['loss'])) / float(gold['loss'])
    print('loss: %.3e relative, bar %.3e' % (w, 4 * float(gold['dev.loss'])))
    assert w <= 4 * float(gold['dev.loss']), ('loss', w)
    worst_g, worst_n = ('', 0.0), ('', 0.0)
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        g = p.grad.detach().cpu().numpy().reshape(-1).astype(np.float64)
        pos = RS.sample_positions(k, g.size)
        gmax, gnorm = float(gold['gmax.' + k]), float(gold['gnorm.' + k])
        if gmax == 0.0:
            assert not g.any(), k
            continue
        e = np.abs(g[pos] - gold['gsample.' + k]).max() / gmax
        n = abs(np.linalg.norm(g) - gnorm) / gnorm
        be, bn = 4 * float(gold['dev.gsample.' + k]), 4 * float(gold['dev.gnorm.' + k])
        if e / max(be, 1e-300) > worst_g[1]:
            worst_g = (k, e / max(be, 1e-300))
        if n / max(bn, 1e-300) > worst_n[1]:
            worst_n = (k, n / max(bn, 1e-300))
        assert e <= be, ('gradient entries', k, e, be)
        # (bn is 4 x the relative 2-norm of the reference's whole float32 difference, which only BOUNDS the difference of the norms --
        # the signed difference itself is one draw of a cancelling quantity, 3.7e-8 on the latent codes.  This line therefore catches
        # gross errors only; the entries above are the real check)
        assert n <= bn, ('gradient norm', k, n, bn)
    print('gradients: worst entry deviation %.2f of its bar (%s), worst norm deviation %.2f of its bar (%s)' % (
        worst_g[1], worst_g[0], worst_n[1], worst_n[0]))
    sd = net.state_dict()
    worst_s = 0.0
    for k in gold.files:
        if k.startswith('stat.'):
            ref_s = gold[k]
            scale = np.abs(ref_s).max()
            e = np.abs(sd[k[5:]].cpu().numpy().astype(np.float64) - ref_s).max() / scale
            b = 4 * float(gold['dev.' + k])
            worst_s = max(worst_s, e / max(b, 1e-300))
            assert e <= b, ('running statistics', k, e, b)
    print('running statistics: worst %.2f of its bar' % worst_s)
    if repeat:
        net2, out2 = one_step(dev, gold)
        assert torch.equal(out2['loss'], out['loss']) and torch.equal(out2['ret']['raw'], ret['raw'])
        for (k, a), (_, b) in zip(net.named_parameters(), net2.named_parameters()):
            assert torch.equal(a.grad, b.grad), ('the second step differs in', k)


LAUNCH_NAMES = ('nb_build_rows', 'nb_subm_table', 'nb_down_tables', 'nb_conv', 'nb_conv_weight_grad', 'nb_sample_forward', 'nb_sample_backward')


def counted_step(dev, gold):
    """one training step with the new ops counted -> (net, out, calls of the forward, calls of the backward)"""
    from xrnerf_amd import ops
    saved = {n: getattr(ops, n) for n in LAUNCH_NAMES}
    calls = []

    def wrap(n):
        def f(*a, **k):
            calls.append(n)
            return saved[n](*a, **k)
        return f
    net = network(dev, gold)
    net.zero_grad()
    try:
        for n in LAUNCH_NAMES:
            setattr(ops, n, wrap(n))
        out = net.train_step(batch(dev, gold, True), None)
        fwd = list(calls)
        out['loss'].backward()
    finally:
        for n in LAUNCH_NAMES:
            setattr(ops, n, saved[n])
    return net, out, fwd, calls[len(fwd):]


def assert_launch_counts(fwd, bwd):
    """a training step builds the structure once and issues one convolution launch per layer and direction"""
    count = lambda lst: {n: lst.count(n) for n in LAUNCH_NAMES if lst.count(n)}
    assert count(fwd) == {'nb_build_rows': 1, 'nb_subm_table': 5, 'nb_down_tables': 4, 'nb_conv': 17, 'nb_sample_forward': 1}, count(fwd)
    assert count(bwd) == {'nb_conv': 17, 'nb_conv_weight_grad': 17, 'nb_sample_backward': 1}, count(bwd)


def check_launch_counts(dev, gold):
    _, _, fwd, bwd = counted_step(dev, gold)
    assert_launch_counts(fwd, bwd)


def check_render_frame(dev, gold):
    """three chunks of a frame share one structure build and one run of the sparse network, and give the whole frame's pixels"""
    from xrnerf_amd import neuralbody as NB
    net = network(dev, gold)
    datas = batch(dev, gold)
    net.chunk = 12
    NB.CALLS['structure'] = NB.CALLS['sparse_net'] = 0
    ret = NB.render_frame(net, datas)
    assert NB.CALLS == {'structure': 1, 'sparse_net': 1}, NB.CALLS
    assert ret['rgb'].shape == (32, 3)
    net2 = network(dev, gold)
    with torch.no_grad():
        whole = net2.forward(batch(dev, gold), True)
    assert NB.CALLS == {'structure': 2, 'sparse_net': 2}
    assert float((ret['rgb'] - whole['rgb']).abs().max()) <= 1e-5
    for (k, a), (_, b) in zip(net.state_dict().items(), net2.state_dict().items()):
        if k.endswith('running_mean') or k.endswith('num_batches_tracked'):
            assert torch.equal(a, b), ('running statistics move once per frame', k)


def check_state_dict_and_registry(gold):
    import xrnerf_amd
    from xrnerf_amd import neuralbody as NB
    net = xrnerf_amd.build_network(copy.deepcopy(model_cfg()))
    assert isinstance(net, NB.NeuralBodyNetwork) and isinstance(net.smpl_conv, NB.SmplEmbedder) and isinstance(net.nerf_mlp, NB.NB_NeRFMLP)
    assert type(net.render).__name__ == 'NerfRender' and net.smpl_conv.voxel_size == [0.005] * 3
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold['sd_keys']]
    assert [list(v.shape) for v in sd.values()] == [json.loads(str(s)) for s in gold['sd_shapes']]


# ------------------------------------------------------------------------------------------ the GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize('out_sh', STRUCT_SH)
@pytest.mark.parametrize('V', STRUCT_V)
def test_structure_matches_the_restatement_exactly(dev, V, out_sh):
    check_structure(dev, V, out_sh)


@pytest.mark.gpu
def test_structure_with_two_scan_sweeps_matches_the_restatement_exactly(dev):
    check_structure(dev, *STRUCT_TWO_SWEEPS)


@pytest.mark.gpu
def test_bad_out_sh_and_volume_over_the_cap_launch_nothing(dev):
    check_structure_errors(dev)


@pytest.mark.gpu
def test_no_vertices_give_empty_levels(dev):
    check_no_vertices(dev)


@pytest.mark.gpu
@pytest.mark.parametrize('N', CONV_N)
@pytest.mark.parametrize('cin,cout,strided', CONV_LAYERS)
def test_convolution_forward_and_gradients_against_float64(dev, cin, cout, strided, N):
    check_conv(dev, cin, cout, strided, N)


@pytest.mark.gpu
@pytest.mark.parametrize('strided_out', [False, True])
@pytest.mark.parametrize('N', SAMPLE_N)
def test_sampling_forward_and_row_gradients_against_float64(dev, N, strided_out):
    check_sampling(dev, N, strided_out)


@pytest.mark.gpu
def test_sampling_edges_and_exact_zeros(dev):
    check_sampling_edges(dev)


@pytest.mark.gpu
def test_fixture_step_against_the_reference(dev, gold):
    check_fixture_step(dev, gold)


@pytest.mark.gpu
def test_step_launch_counts(dev, gold):
    check_launch_counts(dev, gold)


@pytest.mark.gpu
def test_render_frame_runs_the_sparse_network_once(dev, gold):
    check_render_frame(dev, gold)
