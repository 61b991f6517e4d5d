"""The float64 references of tests/ref64_ngp.py pinned once against the fp32 oracle (oracle/ngp_oracle.c), on the CPU: the MLP chain
(raw, weight gradients, dL/d(encoding) through the table gradient it feeds, the kink margin) within the oracle's own fp32 error, the
corner table (cell, weights, dense / hashed / upper-face indices) and the table gradient built from it."""
import numpy as np
import pytest

import ref64_ngp as R


def _scene(O, n, seed, nhd=1, nhc=2):
    from xrnerf_amd import synthetic as S
    om = O.GridMeta()
    rng = np.random.default_rng(seed)
    table = S.hash_table(om.n_params, scale=0.5)
    wd, wc = S.mlp_weights(32, 64, nhd, 16, 4), S.mlp_weights(32, 64, nhc, 16, 5)
    pts = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    pts[0], pts[1] = [1.0, 1.0, 1.0], [0.0, 1.0, 0.5]
    dirs = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    draw = rng.normal(0, 1, (n, 4)).astype(np.float32)
    return om, table, wd, wc, pts, dirs, draw


@pytest.mark.parametrize('nhd,nhc', [(1, 2), (3, 4)])
def test_mlp64_against_the_oracle(O, nhd, nhc):
    n = 3000
    om, table, wd, wc, pts, dirs, draw = _scene(O, n, nhd * 10 + nhc, nhd, nhc)
    enc = O.hashgrid_fwd(table, pts, om)
    margin32 = O.nerf_mlp_kink_margin(table, wd, wc, pts, dirs, om, nhd, nhc)
    draw[margin32 < 1e-4] = 0.0                  # both sides must take the same side of every ReLU
    ref = R.mlp64(enc, dirs, wd, wc, nhd, nhc, draw)
    raw = O.nerf_mlp_fwd(table, wd, wc, pts, dirs, om, nhd, nhc)
    assert np.abs(raw - ref['raw']).max() <= 1e-6 * np.abs(ref['raw']).max()
    gt, gd, gc = O.nerf_mlp_bwd(table, wd, wc, pts, dirs, draw, om, nhd, nhc)
    # the oracle sums n fp32 products serially into each weight entry: within n u of the sum of |terms| <= that of the largest entry
    for got, want in ((gd, ref['dwd']), (gc, ref['dwc'])):
        assert np.abs(got - want).max() <= n * 2.0 ** -24 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()
        assert np.linalg.norm(got - want) <= 1e-5 * np.linalg.norm(want)
    # dL/d(encoding), through the table gradient it feeds (the oracle's fp32 table sums against table_grad64's float64 ones)
    t = R.table_grad64(O, pts, ref['denc'].astype(np.float32), om)
    assert np.abs(gt - t['ref']).max() <= 1e-5 * np.abs(t['ref']).max()
    # the kink margin: the same measure, float64 against the oracle's fp32 pre-activations
    assert np.abs(ref['margin'] - margin32).max() <= 1e-5
    # float64 denc against the oracle's own chain (xo_mlp_bwd) row by row
    if (nhd, nhc) == (1, 2):
        dout, actd = O.mlp_fwd(wd, enc, 32, 64, 1, 16, want_acts=True)
        cin = np.concatenate([dout[:, 1:16], O.sh4(dirs), np.ones((n, 1), np.float32)], 1)
        _, actc = O.mlp_fwd(wc, cin, 32, 64, 2, 16, want_acts=True)
        dyc = np.zeros((n, 16), np.float32); dyc[:, :3] = draw[:, :3]
        _, dcin = O.mlp_bwd(wc, cin, actc, dyc, 32, 64, 2, 16)
        dyd = np.zeros((n, 16), np.float32); dyd[:, 0] = draw[:, 3]; dyd[:, 1:16] = dcin[:, :15]
        _, denc = O.mlp_bwd(wd, enc, actd, dyd, 32, 64, 1, 16)
        rmax = np.abs(ref['denc']).max(1)
        assert (np.abs(denc - ref['denc']).max(1) <= 1e-5 * rmax + 1e-30).all()


def test_sh4_64_against_the_oracle(O):
    d = np.random.default_rng(0).uniform(0, 1, (1000, 3)).astype(np.float32)
    import torch
    assert np.abs(R.sh4_64(torch.from_numpy(d).double()).numpy() - O.sh4(d)).max() <= 1e-6


@pytest.mark.parametrize('layout', ['rand', 'faces', 'cluster'])
def test_corner_table_against_the_oracle(O, layout):
    """the corners reproduce the oracle's forward (dense, hashed and upper-face indices) and their weights sum to one"""
    import scatter_emu_case as SC
    from xrnerf_amd import synthetic as S
    om = O.GridMeta()
    x = SC.positions(2000, layout, np.random.default_rng(1))
    table = S.hash_table(om.n_params, scale=1.0)
    idx, w = O.hashgrid_corners(x, om)
    assert idx.shape == (2000, 16, 8) and w.dtype == np.float64
    assert np.abs(w.sum(-1) - 1.0).max() <= 1e-12
    for lv in range(om.n_levels):
        assert (idx[:, lv] >= int(om.offset[lv])).all() and (idx[:, lv] < int(om.offset[lv + 1])).all()
    enc = np.stack([(table[2 * idx + f] * w).sum(-1) for f in range(2)], -1).reshape(2000, 32)
    ref = O.hashgrid_fwd(table, x, om)
    assert np.abs(enc - ref).max() <= 1e-6
    a, b = O.hashgrid_corners(x, om, (3, 9))
    assert np.array_equal(a, idx[:, 3:9]) and np.array_equal(b, w[:, 3:9])
    # upper faces: x = 1 on a dense level lands on grid coordinate res - 1 + 1 / 2 -> the +1 corner is tcnn's linear index past the
    # lattice row (no clamp), taken modulo the level's size
    if layout == 'faces':
        res = int(om.resolution[0])
        p = np.float32(1.0) * om.scale[0] + np.float32(0.5)
        g = int(np.floor(p))
        assert idx[1, 0, 7] == ((g + 1) + (g + 1) * res + (g + 1) * res * res) % (int(om.offset[1]) - int(om.offset[0]))


def test_table_grad64_against_the_oracle(O):
    import scatter_emu_case as SC
    om = O.GridMeta()
    rng = np.random.default_rng(2)
    for layout in ('rand', 'rays', 'faces'):
        x = SC.positions(3000, layout, rng)
        dy = rng.normal(0, 1, (3000, 32)).astype(np.float32)
        dy[5:9] = 0
        t = R.table_grad64(O, x, dy, om)
        ref = O.hashgrid_bwd(x, dy, om)
        # the oracle adds fp32 products in fp32: within (count + 6) u of the budget per entry
        assert (np.abs(ref - t['ref']) <= (t['count'] + 6) * 2.0 ** -24 * t['budget'] + 1e-30).all(), layout
        assert (t['budget'] >= np.abs(t['ref'])).all() and t['count'].sum() == 8 * 16 * 2 * (3000 - 4)
