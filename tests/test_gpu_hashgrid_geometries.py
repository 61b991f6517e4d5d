"""The hash-grid lookup (xr_encode.hip) and scatter (xr_scatter.hip, the atomic kernel of xr_encode.hip) at level geometries other
than the default one: the block-to-level maps, the partition layouts, the overflow lists and the helper-stream fork are planned
from the geometry at every launch (tests/hashgrid_geometries.py says what each geometry reaches).  One test per geometry, against
the numpy float64 restatement tests/hashgrid_ref64.py: the forward at the bar of test_hashgrid_fwd_bwd, every table-gradient entry
against its own bound (grad_bars.scatter_close with the level kinds mirrored from s3_layout).  The bodies take the device."""
import numpy as np
import pytest
import torch

import grad_bars as B
import hashgrid_geometries as HG
import hashgrid_ref64 as H64

pytestmark = pytest.mark.gpu

FWD_BAR = 2e-6                          # the bar of test_hashgrid_fwd_bwd, table in [-1, 1]
SIZES = (1, 257, 1000, 16384, 20001)    # below min_n (atomic), at it, and more than four binning workgroups' worth of rows
N_FULL = 20001                          # the row count of the variants


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, copy=True)      # (a copy on the host build too)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def feature_major(g, dev):
    """[n, 2L] fp32 -> the scatter's [2L, ld] layout"""
    n = g.shape[0]
    dt = torch.zeros((g.shape[1], (n + 63) // 64 * 64), dtype=torch.float32)
    dt[:, :n] = torch.from_numpy(g).t()
    return dt.contiguous().to(dev)


def level_slices(meta, kinds, want_atomic):
    return [slice(2 * int(meta.offset[lv]), 2 * int(meta.offset[lv + 1])) for lv, k in enumerate(kinds) if (k == 'atomic') == want_atomic]


def lookup_and_scatter(dev, meta, table, n, layout, tag):
    """forward, strided forward, scatter into zeros (+ a second launch), overwrite; -> what the variants reuse"""
    from xrnerf_amd import ops
    rng = np.random.default_rng(n + (layout == 'rays'))
    x = HG.positions(n, rng, layout)
    what = '%s %s n=%d' % (tag, layout, n)
    tx, tt = T(x, dev), T(table, dev)
    enc_t = ops.hashgrid_fwd(tt, tx, meta)
    err = float(np.abs(enc_t[:, :n].t().cpu().numpy() - H64.encode64(table, x, meta)).max())
    B._log(dict(check='hashgrid_fwd', what=what, n=n, err=err))
    assert err <= FWD_BAR, (what, 'forward', err)
    rows7 = np.full((n, 7), 7.0, np.float32)
    rows7[:, :3] = x
    assert same_bits(ops.hashgrid_fwd(tt, T(rows7, dev)[:, :3], meta)[:, :n], enc_t[:, :n]), (what, 'strided positions')
    g = rng.normal(0, 1, (n, 2 * meta.n_levels)).astype(np.float32)
    g[5:9] = 0
    dt = feature_major(g, dev)
    t = H64.table_grad64(x, g, meta)
    kinds = B.level_kinds(meta, n)
    out = torch.zeros(meta.n_params, dtype=torch.float32, device=dev)
    ops.hashgrid_bwd(tx, dt, meta, out)
    B.scatter_close(out.cpu().numpy(), t, meta, g, n, what=what)
    again = torch.zeros(meta.n_params, dtype=torch.float32, device=dev)
    ops.hashgrid_bwd(tx, dt, meta, again)
    ow = torch.full((meta.n_params,), 7.0, dtype=torch.float32, device=dev)
    ops.hashgrid_bwd(tx, dt, meta, ow, overwrite=True)
    for s in level_slices(meta, kinds, want_atomic=False):        # fixed-point sums: the same bits every launch, written or added to zeros
        assert same_bits(again[s], out[s]), (what, 'a second launch differs', s)
        assert same_bits(ow[s], out[s]), (what, 'overwrite differs from accumulate into zeros', s)
    if 'atomic' in kinds:           # (fp32 atomics arrive in any order: the overwriting launch, which clears those slices itself, against float64)
        B.scatter_close(ow.cpu().numpy(), t, meta, g, n, what=what + ' overwrite')
    return x, tx, g, dt, t


def variants(dev, meta, n, tag, x, tx, g, dt, t):
    """level ranges, live rows, device-side count, no workspace at n rows (t: table_grad64 of (x, g))"""
    from xrnerf_amd import ops
    what = '%s n=%d' % (tag, n)
    kinds = B.level_kinds(meta, n)
    L = meta.n_levels
    rng = np.random.default_rng(n + 2)
    # level ranges: (0, L/2) then (L/2, L) into a non-zero table equals the whole launch into it
    init = rng.normal(0, 1e-2, meta.n_params).astype(np.float32)
    t_init = H64.table_grad64(x, g, meta, init=init)
    whole = T(init, dev)
    ops.hashgrid_bwd(tx, dt, meta, whole)
    B.scatter_close(whole.cpu().numpy(), t_init, meta, g, n, what=what + ' accumulate')
    if L >= 2:
        h = L // 2
        parts = T(init, dev)
        ops.hashgrid_bwd(tx, dt, meta, parts, levels=(0, h))
        a = 2 * int(meta.offset[h])
        assert same_bits(parts[a:], T(init, dev)[a:]), (what, 'levels (0, %d) touched entries of later levels' % h)
        for s in level_slices(meta, kinds[:h], want_atomic=False):
            assert same_bits(parts[s], whole[s]), (what, 'levels (0, %d) differ from the whole launch' % h, s)
        before = parts.clone()
        ops.hashgrid_bwd(tx, dt, meta, parts, levels=(h, L))
        assert same_bits(parts[:a], before[:a]), (what, 'levels (%d, %d) touched entries of earlier levels' % (h, L))
        for s in level_slices(meta, kinds, want_atomic=False):
            assert same_bits(parts[s], whole[s]), (what, 'the two ranges differ from the whole launch', s)
        B.scatter_close(parts.cpu().numpy(), t_init, meta, g, n, what=what + ' two level ranges')
    # live-row list: NaN in the rows outside it
    live = np.flatnonzero(rng.uniform(size=n) < 0.5).astype(np.int32)
    g_live = np.zeros_like(g)
    g_live[live] = g[live]
    rows = torch.zeros(n, dtype=torch.int32)
    rows[:len(live)] = torch.from_numpy(live)
    dtp = dt.clone()
    dtp[:, np.setdiff1d(np.arange(n), live)] = float('nan')
    live_t = (rows.to(dev), torch.tensor([len(live), 0, 0, 0], dtype=torch.int32, device=dev))
    out = torch.full((meta.n_params,), 5.0, dtype=torch.float32, device=dev)
    ops.hashgrid_bwd(tx, dtp, meta, out, live=live_t, overwrite=True)
    B.scatter_close(out.cpu().numpy(), H64.table_grad64(x, g_live, meta), meta, g_live, n, what=what + ' live rows')
    # device-side count
    nd = n // 3
    g_nd = g.copy()
    g_nd[nd:] = 0
    out = torch.zeros(meta.n_params, dtype=torch.float32, device=dev)
    ops.hashgrid_bwd(tx, dt, meta, out, n_dev=torch.tensor([nd], dtype=torch.int32, device=dev))
    B.scatter_close(out.cpu().numpy(), H64.table_grad64(x, g_nd, meta), meta, g_nd, n, what=what + ' device-side count')
    # no workspace: every level through the atomic kernel, within the atomic bound
    out = torch.zeros(meta.n_params, dtype=torch.float32, device=dev)
    ops.hashgrid_bwd(tx, dt, meta, out, use_workspace=False)
    bound = (B.CONTRIB + (t['count'] + 1) * B.U) * t['budget'] + 2.0 ** -23 * np.abs(t['ref'])
    bad = np.flatnonzero(np.abs(out.cpu().numpy().astype(np.float64) - t['ref']) > bound)
    assert not bad.size, (what, 'no workspace: entries over the atomic bound', bad.size, int(bad[0]))
    return dtp, live_t


def fused_adam(dev, meta, n, tag, tx, dtp, live_t):
    """two steps of the scatter with the optimiser's update inside against scatter (overwrite) + adam_step_multi, bit for bit;
    where a level has no non-atomic path the entry point refuses and changes nothing"""
    from xrnerf_amd import _lib, ops
    what = '%s n=%d' % (tag, n)
    rng = np.random.default_rng(n + 3)
    p0 = rng.uniform(-1e-4, 1e-4, meta.n_params).astype(np.float32)
    P = [T(p0, dev), T(p0, dev)]
    M, V = ([torch.zeros(meta.n_params, dtype=torch.float32, device=dev) for _ in range(2)] for _ in range(2))
    E = [P[0].clone(), P[1].clone()]
    supported = ops.hashgrid_bwd_adam_supported(n, meta)
    assert supported == ('atomic' not in B.level_kinds(meta, n)), (what, B.level_kinds(meta, n))
    if not supported:
        M[1].fill_(0.25), V[1].fill_(0.5)
        keep = [a[1].clone() for a in (P, M, V, E)]
        with pytest.raises(_lib.XrError):
            ops.hashgrid_bwd_adam(tx, dtp, meta, ops.adam_fuse(P[1], M[1], V[1], E[1], 1, 1e-2, 0.9, 0.99, 1e-15, 1e-6, 0.01), live=live_t)
        torch.cuda.synchronize()
        assert all(same_bits(a[1], k) for a, k in zip((P, M, V, E), keep)), (what, 'a refused fused update changed the optimiser state')
        return
    for step in (1, 2):
        mom = min(0.05, step / (100.0 + step - 1))
        g = torch.full((meta.n_params,), 5.0, dtype=torch.float32, device=dev)
        ops.hashgrid_bwd(tx, dtp, meta, g, live=live_t, overwrite=True)
        ops.adam_step_multi([P[0]], [g], [M[0]], [V[0]], step, 1e-2, 0.9, 0.99, 1e-15, 1e-6, [E[0]], mom)
        ops.hashgrid_bwd_adam(tx, dtp, meta, ops.adam_fuse(P[1], M[1], V[1], E[1], step, 1e-2, 0.9, 0.99, 1e-15, 1e-6, mom), live=live_t)
        for name, a in zip('p m v ema'.split(), (P, M, V, E)):
            assert same_bits(a[0], a[1]), (what, 'fused update differs from scatter + optimiser launch', name, 'step', step)
    assert float((P[0] - T(p0, dev)).abs().max()) > 0, (what, 'the update moved nothing')


def geometry_case(dev, gid, sizes=SIZES, n_full=N_FULL):
    from xrnerf_amd import ops
    meta = ops.GridMeta(*HG.GEOMETRIES[gid])
    sc = B.sc_test()
    if sc['rl']:
        assert HG.paths(meta, max(n_full, sc['min_n'])) == HG.PATHS[gid], (gid, HG.paths(meta, max(n_full, sc['min_n'])))
    table = np.random.default_rng(len(gid) + ord(gid[0])).uniform(-1, 1, meta.n_params).astype(np.float32)
    kept = None
    for n in sizes:
        r = lookup_and_scatter(dev, meta, table, n, 'faces', gid)
        if n == n_full:
            kept = r
    lookup_and_scatter(dev, meta, table, n_full, 'rays', gid)
    x, tx, g, dt, t = kept
    dtp, live_t = variants(dev, meta, n_full, gid, x, tx, g, dt, t)
    fused_adam(dev, meta, n_full, gid, tx, dtp, live_t)
    small = [n for n in sizes if 9 < n < sc['min_n']]
    if small:                       # below min_n rows every level is atomic: the fused update refuses
        n = small[-1]
        every = (torch.arange(n, dtype=torch.int32, device=dev), torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev))
        fused_adam(dev, meta, n, gid, tx[:n].contiguous(), dt[:, :(n + 63) // 64 * 64].contiguous(), every)


@pytest.mark.parametrize('gid', list(HG.GEOMETRIES))
def test_lookup_and_scatter_at_geometry(dev, gid):
    geometry_case(dev, gid)


ENCODINGS = {
    'A': dict(otype='HashGrid', n_levels=8, n_features_per_level=2, log2_hashmap_size=14, base_resolution=4, per_level_scale=1.5),
    # per_level_scale left out: Encoding's own default, 2.0, is what runs (res 16 ... 524 288)
    'J': dict(otype='HashGrid', n_levels=16, n_features_per_level=2, log2_hashmap_size=15, base_resolution=16),
    'K': dict(otype='HashGrid', n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16),
}


def encoding_case(dev, gid, sizes=(257, N_FULL)):
    from xrnerf_amd import ops, tcnn
    enc = tcnn.Encoding(3, ENCODINGS[gid])
    meta, ref_meta = enc.meta, ops.GridMeta(*HG.GEOMETRIES[gid])
    assert enc.n_output_dims == 2 * ref_meta.n_levels
    for a, b in ((meta.scale, ref_meta.scale), (meta.resolution, ref_meta.resolution), (meta.offset, ref_meta.offset)):
        assert np.array_equal(a, b), gid
    if gid in 'JK':
        assert int(meta.resolution[-1]) == 524288
    table = np.random.default_rng(11).uniform(-1, 1, meta.n_params).astype(np.float32)
    with torch.no_grad():
        enc.params.copy_(torch.from_numpy(table))
    enc = enc.to(dev)
    for n in sizes:
        what = 'Encoding %s n=%d' % (gid, n)
        rng = np.random.default_rng(n + 5)
        x = HG.positions(n, rng)
        tx = T(x, dev)
        enc.params.grad = None
        y = enc(tx)
        assert y.shape == (n, enc.n_output_dims)
        assert same_bits(y.detach().contiguous(), ops.hashgrid_fwd(enc.params.detach(), tx, meta)[:, :n].t().contiguous()), (what, 'forward')
        err = float(np.abs(y.detach().cpu().numpy() - H64.encode64(table, x, meta)).max())
        B._log(dict(check='hashgrid_fwd', what=what, n=n, err=err))
        assert err <= FWD_BAR, (what, 'forward', err)
        g = rng.normal(0, 1, (n, enc.n_output_dims)).astype(np.float32)
        y.backward(T(g, dev))
        t = H64.table_grad64(x, g, meta)
        B.scatter_close(enc.params.grad.cpu().numpy(), t, meta, g, n, what=what + ' backward')
        direct = torch.zeros(meta.n_params, dtype=torch.float32, device=dev)
        ops.hashgrid_bwd(tx, feature_major(g, dev), meta, direct)
        B.scatter_close(direct.cpu().numpy(), t, meta, g, n, what=what + ' hashgrid_bwd')
        for s in level_slices(meta, B.level_kinds(meta, n), want_atomic=False):
            assert same_bits(enc.params.grad[s], direct[s]), (what, 'backward differs from ops.hashgrid_bwd', s)


@pytest.mark.parametrize('gid', list(ENCODINGS))
def test_tcnn_encoding_at_geometry(dev, gid):
    encoding_case(dev, gid)
