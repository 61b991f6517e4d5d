"""The hash grid at level geometries other than the default one, without a GPU: the oracle (oracle/ngp_oracle.c) and the kernels'
host build (tests/hip_emu) against the numpy float64 restatement tests/hashgrid_ref64.py at every geometry of
tests/hashgrid_geometries.py, and grad_bars.level_kinds -- the tests' mirror of xr_scatter.hip's s3_layout -- against its earlier
output on the default geometry and against the library's own answer (ops.hashgrid_bwd_adam_supported).  The scatter on the host
build runs in child processes (tests/test_emu_scatter.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))

import grad_bars as B                   # noqa: E402
import hashgrid_geometries as HG        # noqa: E402
import hashgrid_ref64 as H64            # noqa: E402

GIDS = list(HG.GEOMETRIES)
N = 3000
FWD_BAR = 2e-6                          # the bar of test_hashgrid_fwd_bwd, table in [-1, 1]


@pytest.fixture(scope='module')
def edev():
    import emulib
    ctx = emulib.emulated_ops()
    dev = ctx.__enter__()
    yield dev
    ctx.__exit__(None, None, None)


@functools.lru_cache(maxsize=None)
def case(gid):
    """(oracle meta, table, positions, float64 encoding) of a geometry, computed once and shared by the tests below"""
    import oracle as O
    meta = O.GridMeta(*HG.GEOMETRIES[gid])
    rng = np.random.default_rng(sorted(HG.GEOMETRIES).index(gid))
    table = rng.uniform(-1, 1, meta.n_params).astype(np.float32)
    x = HG.positions(N, rng)
    ref = H64.encode64(table, x, meta)
    for a in (table, x, ref):
        a.setflags(write=False)
    return meta, table, x, ref


@pytest.mark.parametrize('gid', GIDS)
def test_paths_of_the_geometries(gid, monkeypatch):
    """the mirror of s3_layout gives every geometry the paths it is in the list for (default XR_SC_TEST, from min_n rows on)"""
    monkeypatch.delenv('XR_SC_TEST', raising=False)
    meta = case(gid)[0]
    for n in (16384, 20001):
        assert HG.paths(meta, n) == HG.PATHS[gid], (gid, n, HG.paths(meta, n))
    assert HG.paths(meta, 16383) == 'A' * meta.n_levels
    if gid in HG.ENTRIES:
        assert int(meta.offset[-1]) == HG.ENTRIES[gid]


def level_kinds_before(meta, n):
    """grad_bars.level_kinds as it stood while only the default geometry was tested"""
    t = B.sc_test()
    out = []
    for lv in range(meta.n_levels):
        hsize = int(meta.offset[lv + 1]) - int(meta.offset[lv])
        dense = int(meta.resolution[lv]) ** 3 <= hsize
        out.append('atomic' if n < t['min_n'] else 'rl' if (dense and hsize <= B.RL_MAX_ENTRIES and t['rl']) else 'bin')
    return out


@pytest.mark.parametrize('sc', ['', 'min_n=256', 'min_n=256,rl=0', 'rl=0', 'block=1024', 'min_n=256,block=2048,rl_chunks=3', 'min_n=1'])
def test_level_kinds_of_the_default_geometry_are_what_they_were(sc, monkeypatch):
    """at every row count a launch of at most S3_MAX_SB sample blocks can have (beyond it the library sends every level to the atomic
    kernel, which the earlier function did not know)"""
    monkeypatch.setenv('XR_SC_TEST', sc)
    meta = case('default')[0]
    block = B.sc_test()['block']
    for n in (1, 255, 256, 257, 1000, 16383, 16384, 16385, 20001, 50001, 1 << 18, B.MAX_SB * block):
        assert B.level_kinds(meta, n) == level_kinds_before(meta, n), (sc, n)
    assert B.level_kinds(meta, B.MAX_SB * block + 1) == ['atomic'] * 16


@pytest.mark.parametrize('gid', GIDS)
def test_level_kinds_agree_with_the_library(gid, edev, monkeypatch):
    """the fused update is available exactly when no level is 'atomic' (the library's s3_layout on the host build).  The library reads
    XR_SC_TEST once per process and grad_bars at every call: the tests of this suite that set it do so in child processes only, and
    here it is cleared so that both sides use the defaults"""
    from xrnerf_amd import ops
    monkeypatch.delenv('XR_SC_TEST', raising=False)
    meta = ops.GridMeta(*HG.GEOMETRIES[gid])
    for n in (1000, 16384, 20001):
        assert ops.hashgrid_bwd_adam_supported(n, meta) == ('atomic' not in B.level_kinds(meta, n)), (gid, n, B.level_kinds(meta, n))


def index_with_a_32_bit_stride(x, meta, lv):
    """the published loop read literally with a uint32 stride (what oracle/ngp_oracle.c did before it was given 64 bits), corner 0 only"""
    res, hsize, _, _ = H64.level_geometry(meta, lv)
    p = (np.ascontiguousarray(x, np.float32) * np.float32(meta.scale[lv])).astype(np.float32) + np.float32(0.5)
    c = np.floor(p).astype(np.int64) & H64.M32
    stride, index = 1, np.zeros(len(c), np.int64)
    for d in range(3):
        if stride > hsize:
            break
        index = (index + c[:, d] * stride) & H64.M32
        stride = (stride * res) & H64.M32
    if hsize < stride:
        index = c[:, 0] ^ ((c[:, 1] * H64.P1) & H64.M32) ^ ((c[:, 2] * H64.P2) & H64.M32)
    return index % hsize


def test_geometry_k_tells_a_32_bit_stride_from_a_64_bit_one():
    """the two readings differ exactly where 65536 <= res <= hsize: levels 12-15 of K (slices of 2^19 entries), nowhere in J (2^15)
    nor in the default geometry -- so K is what holds the oracle, the kernels and the restatement to the 64-bit rule below"""
    for gid, differ in (('K', (12, 13, 14, 15)), ('J', ()), ('default', ())):
        meta, _, x, _ = case(gid)
        for lv in range(meta.n_levels):
            res, hsize, _, _ = H64.level_geometry(meta, lv)
            assert (65536 <= res <= hsize) == (lv in differ), (gid, lv, res, hsize)
            same = float((index_with_a_32_bit_stride(x, meta, lv) == H64.corners(x, meta, lv)[0][:, 0]).mean())
            assert (same < 0.01) if lv in differ else (same == 1.0), (gid, lv, same)


@pytest.mark.parametrize('gid', GIDS)
def test_oracle_against_float64(gid, O):
    meta, table, x, ref = case(gid)
    err = float(np.abs(O.hashgrid_fwd(table, x, meta) - ref).max())
    assert err <= FWD_BAR, (gid, 'forward', err)
    idx, w = O.hashgrid_corners(x, meta)
    for lv in range(meta.n_levels):
        i64, w64 = H64.corners(x, meta, lv)
        assert np.array_equal(idx[:, lv, :], i64 + int(meta.offset[lv])), (gid, 'corner indices of level', lv)
        assert np.array_equal(w[:, lv, :], w64), (gid, 'corner weights of level', lv)
    rng = np.random.default_rng(7)
    g = rng.normal(0, 1, (N, 2 * meta.n_levels)).astype(np.float32)
    g[5:9] = 0
    t = H64.table_grad64(x, g, meta)
    got = O.hashgrid_bwd(x, g, meta).astype(np.float64)
    # a sequential fp32 sum of c contributions: the atomic kernel's bound (grad_bars.scatter_close)
    bound = (B.CONTRIB + (t['count'] + 1) * B.U) * t['budget'] + 2.0 ** -23 * np.abs(t['ref'])
    bad = np.flatnonzero(np.abs(got - t['ref']) > bound)
    assert not bad.size, (gid, 'table gradient entries over their bound', bad.size, int(bad[0]))


@pytest.mark.parametrize('gid', GIDS)
def test_host_build_forward_against_float64(gid, edev):
    from xrnerf_amd import ops
    _, table, x, ref = case(gid)
    meta = ops.GridMeta(*HG.GEOMETRIES[gid])
    enc_t = ops.hashgrid_fwd(torch.from_numpy(table.copy()), torch.from_numpy(x.copy()), meta)
    err = float(np.abs(enc_t[:, :N].t().numpy() - ref).max())
    assert err <= FWD_BAR, (gid, err)
