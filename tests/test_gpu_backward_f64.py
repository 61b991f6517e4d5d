"""The training backward against float64: the fused MLP backward (xr_mlp.hip: k_nerf_mlp_bwd_1_2 in every XR_MLP_BWD_DW arithmetic,
k_nerf_mlp_bwd_deep, the layer-by-layer path) and the third-generation table scatter (xr_scatter.hip: binned, run-length, overflow
lists, atomic below 16384 rows), against tests/ref64_ngp.py at the bars of tests/grad_bars.py.  The bodies take the device; the
emulator runs them at small sizes (tests/test_emu_backward_f64.py)."""
import numpy as np
import pytest
import torch

import grad_bars as B
import ref64_ngp as R

pytestmark = pytest.mark.gpu

MODES = ('f32', 'b2', 'b2x', 'b2f', 'h2f')
SENTINEL = 7.0


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def mlp_inputs(n, nhd, nhc, seed):
    from xrnerf_amd import synthetic as S
    rng = np.random.default_rng(seed)
    enc = rng.normal(0, 0.5, (n, 32)).astype(np.float32)
    dirs = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    draw = rng.normal(0, 1, (n, 4)).astype(np.float32)
    return enc, dirs, draw, S.mlp_weights(32, 64, nhd, 16, 4), S.mlp_weights(32, 64, nhc, 16, 5)


def mlp_case(dev, n, arith, nhd=1, nhc=2, n_valid=None, dead=None, live=False, row0=0, count=None, seed=0, check_raw=True):
    """one backward call against float64.  n_valid: device-side count (rows behind it hold NaN); dead: bool [n] rows with an exactly
    zero dL/d(raw); live: hand the backward the list of the other rows (ops.live_rows); row0 / count: the launch covers rows
    [row0, row0 + count).  Rows the launch must not write hold SENTINEL in dL/d(encoding) beforehand."""
    from xrnerf_amd import ops
    enc, dirs, draw, wd, wc = mlp_inputs(n, nhd, nhc, seed)
    lo, hi = row0, n if count is None else row0 + count
    hi = hi if n_valid is None else min(hi, n_valid)
    sel = slice(lo, hi)
    fwd = R.mlp64(enc[sel], dirs[sel], wd, wc, nhd, nhc, None)
    risk = np.zeros(n, bool)
    risk[sel] = B.at_risk(fwd['margin'], arith)
    draw[risk] = 0.0
    if dead is not None:
        draw[dead] = 0.0
    ref = R.mlp64(enc[sel], dirs[sel], wd, wc, nhd, nhc, draw[sel])
    enc_g, draw_g = enc.copy(), draw.copy()
    if n_valid is not None:
        enc_g[n_valid:] = np.nan
        draw_g[n_valid:] = np.nan
    enc_t = T(np.ascontiguousarray(enc_g.T), dev)
    n_dev = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device=dev)
    if check_raw and row0 == 0 and count is None:
        raw = ops.nerf_mlp_fwd(enc_t, T(dirs, dev), n, T(wd, dev), T(wc, dev), nhd, nhc, n_dev=n_dev).cpu().numpy()
        B.raw_close(raw[sel], ref['raw'], 'raw n=%d (%d, %d)' % (n, nhd, nhc))
    g_wd = torch.zeros(wd.size, dtype=torch.float32, device=dev)
    g_wc = torch.zeros(wc.size, dtype=torch.float32, device=dev)
    denc_t = torch.full((32, n), SENTINEL, dtype=torch.float32, device=dev)
    td = T(draw_g, dev)
    lst = ops.live_rows(td, n, n_dev=n_dev) if live else None
    ops.nerf_mlp_bwd(enc_t, T(dirs, dev), n, T(wd, dev), T(wc, dev), nhd, nhc, td, g_wd, g_wc, denc_t=denc_t, n_dev=n_dev,
                     row0=row0, count=count, live=lst)
    what = '%s n=%d (%d, %d) valid=%s live=%s rows=[%d, %d)' % (arith, n, nhd, nhc, n_valid, live, lo, hi)
    B.mlp_close(g_wd.cpu().numpy(), ref['dwd'], arith, 'dWd ' + what)
    B.mlp_close(g_wc.cpu().numpy(), ref['dwc'], arith, 'dWc ' + what)
    d = denc_t.cpu().numpy().T
    # rows outside [row0, row0 + count) and behind the count: untouched; with a live list, the rows outside it: untouched;
    # otherwise the dead rows inside the range: exactly zero (ops.nerf_mlp_bwd)
    end = n if count is None else lo + count
    outside = np.ones(n, bool)
    outside[lo:end] = False
    assert (d[outside] == SENTINEL).all(), (what, 'rows outside the launch were written')
    if hi < end:                      # behind the device-side count: untouched (fused kernels) or zero (layer by layer)
        behind = d[hi:end]
        assert ((behind == SENTINEL).all(1) | (behind == 0).all(1)).all(), (what, 'rows behind the count hold garbage')
    zero_rows = ~(draw[sel] != 0).any(1)
    if live:
        assert (d[sel][zero_rows] == SENTINEL).all(), (what, 'rows outside the live list were written')
        got = d[sel].copy()
        got[zero_rows] = 0.0
    else:
        got = d[sel]
        assert not got[zero_rows].any(), (what, 'dead rows must get an exactly-zero dL/d(encoding)')
    B.denc_close(got, ref['denc'], arith, 'denc ' + what)
    return ref, d


@pytest.mark.parametrize('n', [1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 5000, 40001])
@pytest.mark.parametrize('arith', MODES)
def test_mlp_backward_against_float64(dev, n, arith, monkeypatch):
    monkeypatch.setenv('XR_MLP_BWD_DW', arith)
    mlp_case(dev, n, arith, seed=n)


@pytest.mark.parametrize('arith', MODES)
def test_mlp_backward_against_float64_at_full_size(dev, arith, monkeypatch):
    """2^18 rows of which 230000 are valid, NaN behind the count"""
    monkeypatch.setenv('XR_MLP_BWD_DW', arith)
    mlp_case(dev, 1 << 18, arith, n_valid=230000, seed=18)


def topo_arith(nhd, nhc, path):
    """the bars of a topology's path: XR_MLP_BWD_DW on the (1, 2) kernel; the streamed deep kernel and the layer-by-layer linear
    kernels recompute with the default forward's split operands and split their products (measured: beyond the fp32 bars) -> h2f"""
    return B.mode() if (nhd, nhc) == (1, 2) and path == 'streamed' else 'h2f'


@pytest.mark.parametrize('path', ['streamed', 'layered'])
@pytest.mark.parametrize('nhd,nhc', [(1, 2), (1, 1), (2, 1), (3, 4), (5, 5), (8, 8)])
def test_mlp_topologies_against_float64(dev, nhd, nhc, path, monkeypatch):
    from xrnerf_amd import ops
    monkeypatch.delenv('XR_MLP_BWD_DW', raising=False)
    if path == 'layered':
        monkeypatch.setattr(ops, '_FUSED_FWD', ())
        monkeypatch.setattr(ops, '_FUSED_BWD', ())
    arith = topo_arith(nhd, nhc, path)
    mlp_case(dev, 1025, arith, nhd, nhc, seed=nhd * 10 + nhc)
    mlp_case(dev, 3000, arith, nhd, nhc, n_valid=2100, seed=nhd * 10 + nhc + 1)


def live_layouts(n, rng):
    """dead-row masks: none dead, all dead, half (random), and live runs across the 1024-row segments of the live list"""
    cross = np.ones(n, bool)
    for a, b in ((1000, 1100), (2040, 2060), (3071, 3073)):
        cross[a:min(b, n)] = False
    return {'all': np.zeros(n, bool), 'none': np.ones(n, bool), 'half': rng.uniform(size=n) < 0.5, 'segments': cross}


@pytest.mark.parametrize('layout', ['all', 'none', 'half', 'segments'])
@pytest.mark.parametrize('live', [False, True])
def test_mlp_backward_live_rows_against_float64(dev, layout, live, monkeypatch):
    monkeypatch.delenv('XR_MLP_BWD_DW', raising=False)
    n = 3300
    dead = live_layouts(n, np.random.default_rng(3))[layout]
    mlp_case(dev, n, B.mode(), dead=dead, live=live, seed=33)
    mlp_case(dev, n, B.mode(), dead=dead, live=live, n_valid=2500, seed=34)


@pytest.mark.parametrize('row0,count', [(0, 1025), (1000, 1100), (2047, 1)])
def test_mlp_backward_row_range_against_float64(dev, row0, count, monkeypatch):
    monkeypatch.delenv('XR_MLP_BWD_DW', raising=False)
    mlp_case(dev, 3300, B.mode(), row0=row0, count=count, seed=row0 + count)


def backward_against_float64(O, dev, table, wd, wc, pts, dirs, draw, nhd=1, nhc=2, n_valid=None):
    """the float64 companion of the oracle checks in tests/test_gpu_tcnn.py: the same inputs, the samples at kink risk for the current
    arithmetic with a zero dL/d(raw) on both sides, one more backward + scatter -> dWd, dWc per entry, dL/d(encoding) row by row
    against float64, the table gradient of the kernel's own dL/d(encoding) entry by entry"""
    from xrnerf_amd import ops
    arith = B.mode() if (nhd, nhc) == (1, 2) else 'h2f'
    meta = ops.GridMeta()
    n = pts.shape[0]
    nv = n if n_valid is None else n_valid
    tt, tp = T(table, dev), T(pts, dev)
    enc_t = ops.hashgrid_fwd(tt, tp, meta)
    enc = enc_t[:, :nv].t().cpu().numpy()
    draw = draw.copy()
    draw[nv:] = 0.0
    draw[:nv][B.at_risk(R.mlp64(enc, dirs[:nv], wd, wc, nhd, nhc, None)['margin'], arith)] = 0.0
    ref = R.mlp64(enc, dirs[:nv], wd, wc, nhd, nhc, draw[:nv])
    n_dev = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device=dev)
    g_wd = torch.zeros(wd.size, dtype=torch.float32, device=dev)
    g_wc = torch.zeros(wc.size, dtype=torch.float32, device=dev)
    denc_t = ops.nerf_mlp_bwd(enc_t, T(dirs, dev), n, T(wd, dev), T(wc, dev), nhd, nhc, T(draw, dev), g_wd, g_wc, n_dev=n_dev)
    what = '%s n=%d (%d, %d)' % (arith, n, nhd, nhc)
    B.mlp_close(g_wd.cpu().numpy(), ref['dwd'], arith, 'dWd ' + what)
    B.mlp_close(g_wc.cpu().numpy(), ref['dwc'], arith, 'dWc ' + what)
    g = denc_t[:, :nv].t().cpu().numpy()
    B.denc_close(g, ref['denc'], arith, 'denc ' + what)
    g_t = torch.zeros(meta.n_params, dtype=torch.float32, device=dev)
    ops.hashgrid_bwd(tp, denc_t, meta, g_t, n_dev=n_dev)
    B.scatter_close(g_t.cpu().numpy(), R.table_grad64(O, pts[:nv], g, meta), meta, g, n, what='table ' + what)


# ------------------------------------------------------------------------------------------------ table scatter
def scatter_inputs(O, dev, n, layout, seed):
    """positions in `layout` (tests/scatter_emu_case.py) and the MLP backward's own fp32 dL/d(encoding) for them"""
    from xrnerf_amd import ops, synthetic as S
    import scatter_emu_case as SC
    meta = ops.GridMeta()
    rng = np.random.default_rng(seed)
    x = SC.positions(n, {'uniform': 'rand'}.get(layout, layout), rng)
    table = T(S.hash_table(meta.n_params, scale=0.5), dev)
    wd, wc = S.mlp_weights(32, 64, 1, 16, 4), S.mlp_weights(32, 64, 2, 16, 5)
    tx = T(x, dev)
    enc_t = ops.hashgrid_fwd(table, tx, meta)
    dirs = T(rng.uniform(0, 1, (n, 3)).astype(np.float32), dev)
    draw = T(rng.normal(0, 1, (n, 4)).astype(np.float32), dev)
    g_wd = torch.zeros(wd.size, dtype=torch.float32, device=dev)
    g_wc = torch.zeros(wc.size, dtype=torch.float32, device=dev)
    denc_t = ops.nerf_mlp_bwd(enc_t, dirs, n, T(wd, dev), T(wc, dev), 1, 2, draw, g_wd, g_wc)
    return meta, x, tx, denc_t


def scatter_case(O, dev, n, layout, repeats=1, seed=None):
    from xrnerf_amd import ops
    meta, x, tx, denc_t = scatter_inputs(O, dev, n, layout, n if seed is None else seed)
    g = denc_t[:, :n].t().cpu().numpy()
    t = R.table_grad64(O, x, g, meta)
    first = None
    for k in range(repeats):
        out = torch.zeros(meta.n_params, dtype=torch.float32, device=dev)
        ops.hashgrid_bwd(tx, denc_t, meta, out)
        got = out.cpu().numpy()
        if first is None:
            first = got
            B.scatter_close(got, t, meta, g, n, what='%s n=%d' % (layout, n))
        else:
            assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), ('launch %d differs from the first' % k, layout, n)
    return meta, x, tx, denc_t, g


@pytest.mark.parametrize('n', [16383, 16384, 16385, 50001])
@pytest.mark.parametrize('layout', ['uniform', 'rays', 'cluster', 'faces'])
def test_scatter_against_float64(O, dev, n, layout):
    scatter_case(O, dev, n, layout)


@pytest.mark.parametrize('layout', ['uniform', 'rays', 'cluster', 'faces'])
def test_scatter_against_float64_at_full_size_same_bits(O, dev, layout):
    scatter_case(O, dev, 1 << 18, layout, repeats=3)


def scatter_variants(O, dev, n, layout):
    """live list with half the rows dead (NaN in them), device-side count, level ranges, overwrite against accumulate into a
    non-zero table"""
    from xrnerf_amd import ops
    meta, x, tx, denc_t = scatter_inputs(O, dev, n, layout, n + 1)
    g = denc_t[:, :n].t().cpu().numpy().copy()
    rng = np.random.default_rng(n)
    live = np.flatnonzero(rng.uniform(size=n) < 0.5).astype(np.int32)
    g_live = np.zeros_like(g)
    g_live[live] = g[live]
    rows = torch.zeros(n, dtype=torch.int32)
    rows[:len(live)] = torch.from_numpy(live)
    dtp = denc_t.clone()
    dtp[:, np.setdiff1d(np.arange(n), live)] = float('nan')
    out = torch.full((meta.n_params,), 5.0, dtype=torch.float32, device=dev)
    ops.hashgrid_bwd(tx, dtp.contiguous(), meta, out, live=(rows.to(dev), torch.tensor([len(live), 0, 0, 0], dtype=torch.int32, device=dev)),
                     overwrite=True)
    B.scatter_close(out.cpu().numpy(), R.table_grad64(O, x, g_live, meta), meta, g_live, n, what='live half %s n=%d' % (layout, n))
    nd = n // 3
    g_nd = g.copy()
    g_nd[nd:] = 0.0
    out = torch.zeros(meta.n_params, dtype=torch.float32, device=dev)
    ops.hashgrid_bwd(tx, denc_t, meta, out, n_dev=torch.tensor([nd], dtype=torch.int32, device=dev))
    B.scatter_close(out.cpu().numpy(), R.table_grad64(O, x, g_nd, meta), meta, g_nd, n, what='n_dev %s n=%d' % (layout, n))
    init = rng.normal(0, 1e-2, meta.n_params).astype(np.float32)
    for lv in ((0, 8), (8, 16)):
        for ow in (False, True):
            out = T(init.copy(), dev)
            ops.hashgrid_bwd(tx, denc_t, meta, out, levels=lv, overwrite=ow)
            t = R.table_grad64(O, x, g, meta, levels=lv, init=None if ow else init)
            if ow:                      # the launch's levels are written, the others keep the initial values
                a, b = 2 * int(meta.offset[lv[0]]), 2 * int(meta.offset[lv[1]])
                t['ref'][:a], t['ref'][b:] = init[:a], init[b:]
            B.scatter_close(out.cpu().numpy(), t, meta, g, n, levels=lv, outside=init,
                            what='levels %r overwrite=%s %s n=%d' % (lv, ow, layout, n))


@pytest.mark.parametrize('layout', ['uniform', 'rays', 'cluster', 'faces'])
def test_scatter_variants_against_float64(O, dev, layout):
    scatter_variants(O, dev, 50001, layout)
