"""TEST INFRASTRUCTURE: bars for the training backward against the float64 references of tests/ref64_ngp.py, one per arithmetic.

MLP backward (xr_mlp.hip, XR_MLP_BWD_DW): every weight-gradient entry within ENTRY * max|ref|, the whole difference within NORM of
|ref| in the 2-norm, and dL/d(encoding) row by row within ROW of the row's own largest entry.  The bars sit at >= 3x the worst value
measured on the MI355X (the table in BARS) and >= 10x below what a split with its low half dropped produces.

ReLU kinks: a backward that recomputes a hidden pre-activation z in its own arithmetic can disagree with float64 about relu'(z) on a
sample whose margin |z| / sum |w x| is below that arithmetic's relative error (KINK: 2^-20 for the fp32 recompute of f32 / b2 / b2x,
2^-18 for the fp16 split of h2f and the deep kernel, 1e-5 for the bf16 split of b2f).  Those samples get a zero dL/d(raw) on BOTH sides (`at_risk`); fewer than 2 % may be at
risk, and then every entry is held to the plain bar.

Table scatter (xr_scatter.hip): entry i is held to its own bound
    |got - ref| <= A * budget_i + 2^-23 * |ref_i| + c_i * q_level
budget_i = |initial value| + sum |w g| over its contributions, c_i = their number, q_level = 2^-S of the level (s3_scale, restated in
`quantum`).  A is derived from the kernels' fp32 steps (`scatter_close`), not measured."""
import json
import os

import numpy as np

U = 2.0 ** -24                      # fp32 unit roundoff
# arithmetic -> (per entry / max|ref|, relative 2-norm, dL/denc per row / max|ref row|); worst measured on the MI355X in brackets.
# The split modes carry each product to ~2^-16 of |g||h| (the dropped low x low term and the low parts' rounding, xr_mlp.hip
# dw_mfma_b2): on sums with cancellation that is ~1e-5 of |ref| in the 2-norm, above the 2e-5 the norm bar started from, hence 4e-5;
# a split that loses its low half is 2^-8 per product, ~100x above every split bar.
BARS = {
    'f32': (1e-5, 2e-6, 1e-5),          # (6.2e-7, 3.9e-7, 9.6e-7)
    'b2': (1e-4, 2e-5, 1e-5),           # (1.0e-5, 5.3e-6, 9.6e-7): the dX chain is fp32
    'b2x': (1e-4, 4e-5, 3e-4),          # (1.5e-5, 1.1e-5, 5.2e-5)
    'b2f': (1e-4, 4e-5, 3e-4),          # (1.6e-5, 1.2e-5, 5.2e-5)
    'h2f': (1e-4, 4e-5, 4e-4),          # (1.5e-5, 1.2e-5, 1.3e-4 -- (8, 8): 16 split dX layers on the streamed deep kernel)
}
RAW_BAR = 4e-6                      # raw of the default forward (f16x2 split) against float64, per entry / max|raw| (1.1e-6, (5, 5))
# recompute error relative to sum |w x|: fp32 (f32 / b2 / b2x) ~2^-24 per layer; fp16 2-way split (h2f, XR_MLP_F16X2) ~4e-7; bf16
# 2-way split (b2f) ~2^-16
KINK = {'f32': 2.0 ** -20, 'b2': 2.0 ** -20, 'b2x': 2.0 ** -20, 'b2f': 1e-5, 'h2f': 2.0 ** -18}
MAX_AT_RISK = 0.02


def mode():
    """the backward's arithmetic for the current environment (XR_MLP_BWD_DW unset = h2f)"""
    return os.environ.get('XR_MLP_BWD_DW', 'h2f')


def _log(rec):
    """GRAD_BARS_LOG=<file>: append what each check measured (the calibration record)"""
    path = os.environ.get('GRAD_BARS_LOG')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(rec) + '\n')


def at_risk(margin, arith):
    """samples whose float64 kink margin is below the arithmetic's threshold; asserts they are fewer than 2 % (one, in a launch of
    fewer than 50 samples)"""
    risk = np.asarray(margin) < KINK[arith]
    assert risk.sum() <= max(1.0, MAX_AT_RISK * risk.size), ('kink-risk samples', int(risk.sum()), risk.size)
    return risk


def raw_close(got, ref, what=''):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    if not ref.size:
        return
    scale = max(float(np.abs(ref).max()), 1e-30)
    worst = float(np.abs(got - ref).max()) / scale
    _log(dict(check='raw', what=what, entry=worst))
    assert worst <= RAW_BAR, (what, worst, RAW_BAR)


def mlp_close(got, ref, arith, what=''):
    """weight gradient (any shape) of the arithmetic `arith` against float64: per entry and relative 2-norm"""
    entry, norm, _ = BARS[arith]
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    d = got - ref
    scale = float(np.abs(ref).max())
    if scale == 0.0:
        assert not d.any(), what
        return
    e = float(np.abs(d).max()) / scale
    r = float(np.linalg.norm(d)) / float(np.linalg.norm(ref))
    _log(dict(check='dw', arith=arith, what=what, entry=e, norm=r))
    assert e <= entry and r <= norm, (what, arith, 'entry', e, entry, 'norm', r, norm)


def denc_close(got, ref, arith, what=''):
    """dL/d(encoding) [n, 32] row by row: max_j |got - ref| <= ROW * max_j |ref| on every row; rows whose reference is exactly zero
    (dead rows) must be exactly zero"""
    _, _, row = BARS[arith]
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    if not ref.size:
        return
    rmax = np.abs(ref).max(1)
    zero = rmax == 0
    assert not got[zero].any(), (what, 'rows with a zero reference must be exactly zero', int(np.count_nonzero(got[zero].any(1))))
    if zero.all():
        return
    err = np.abs(got - ref).max(1)[~zero] / rmax[~zero]
    w = float(err.max())
    _log(dict(check='denc', arith=arith, what=what, row=w, median=float(np.median(err))))
    assert w <= row, (what, arith, 'row', w, row, int(np.argmax(err)))


# ------------------------------------------------------------------------------------------------ table scatter
BLOCK = 4096             # samples per binning workgroup (xr_scatter.hip S3Test::block)
MIN_N = 16384            # rows from which the binned / run-length paths run (S3Test::min_n)
MAX_SB = 1024            # sample blocks of a launch above which every level takes the atomic kernel (S3_MAX_SB)
PART_ENTRIES = 8192      # table entries of one accumulate partition, the LDS capacity (S3_ENTRIES)
MAX_PARTS = 256          # partitions of a binned level (S3_MAX_PARTS)
RL_MAX_ENTRIES = 65536   # dense levels up to this size take the run-length kernel (S3_R_MAX_ENTRIES)
RL_ROWS = 16             # consecutive rows a run-length thread sums in fp32 registers (S3_R_ROWS)
RL_CHUNKS = 8            # row chunks of a run-length partition, folded in fp32 by k_scatter_fold (S3Test::rl_chunks)
# one contribution w g in fp32: up to three 1 - w roundings, two weight products, the product with g (binned levels: the same six
# operations, split between the binning and the accumulate kernel)
CONTRIB = 6 * U
# binned levels: the contribution, then the quantised exact sum rounded once to fp32 (s3_val) -- <= 7u of the budget, inside 2^-21
A_BIN = 2.0 ** -21
# run-length levels: the contribution, a thread's fp32 sum of <= 16 rows' contributions (15 roundings of partial sums of the
# budget's terms), the chunk's quantised sum rounded to fp32 (1), k_scatter_fold's fp32 sum of the initial value and the chunks'
# slabs (rl_chunks roundings): (6 + 15 + 1 + 8) u = 30 u to first order at the default 8 chunks -- between 2^-19 and 2^-18
assert CONTRIB + U <= A_BIN


def sc_test():
    """the scatter's layout switch XR_SC_TEST="min_n=..,block=..,rl_chunks=..,rl=.." of this process, as xr_scatter.hip parses it"""
    v = dict(min_n=MIN_N, block=BLOCK, rl_chunks=RL_CHUNKS, rl=1)
    for kv in filter(None, os.environ.get('XR_SC_TEST', '').split(',')):
        k, _, val = kv.partition('=')
        if k in v:
            v[k] = int(val)
    v['block'] = v['block'] if v['block'] in (1024, 2048) else 4096
    v['rl_chunks'] = v['rl_chunks'] if 1 <= v['rl_chunks'] <= 64 else 8
    return v


def level_kinds(meta, n):
    """per level, the path xr_scatter.hip's s3_layout gives it at n rows: 'rl' (run-length, kind R: dense, <= 2^16 entries), 'bin'
    (bin / accumulate: kind H, a hashed power-of-two slice of 1 .. 256 partitions of 2^13 entries at an even offset with res < 2^13, or
    kind D, a larger dense level with 8 <= res <= 128) or 'atomic' (fp32 atomics: every level below min_n rows or above MAX_SB sample
    blocks, and the levels no kind fits)"""
    t = sc_test()
    if n < t['min_n'] or -(-n // t['block']) > MAX_SB:
        return ['atomic'] * meta.n_levels
    out = []
    for lv in range(meta.n_levels):
        res, off = int(meta.resolution[lv]), int(meta.offset[lv])
        hsize = int(meta.offset[lv + 1]) - off
        hashed = res ** 3 > hsize
        kind_h = (hashed and hsize & (hsize - 1) == 0 and hsize >= PART_ENTRIES and hsize // PART_ENTRIES <= MAX_PARTS
                  and res < PART_ENTRIES and off % 2 == 0)
        kind_r = not hashed and hsize <= RL_MAX_ENTRIES and bool(t['rl'])
        kind_d = not hashed and not kind_r and 8 <= res <= 128
        out.append('rl' if kind_r else 'bin' if (kind_h or kind_d) else 'atomic')
    return out


def quantum(g, meta, n):
    """q per level = 2^-S of s3_scale: max |dL/d feature| of the level over the rows the launch reads (m < 2^e) and the row bound
    n_bound = ceil(n / block) * block (8 n_bound < 2^L): S = min(62 - L, 46) - e"""
    g = np.asarray(g, np.float32)
    block = sc_test()['block']
    nb = -(-n // block) * block
    L = int(8 * nb).bit_length()
    q = np.zeros(meta.n_levels)
    for lv in range(meta.n_levels):
        m = float(np.abs(g[:, 2 * lv:2 * lv + 2]).max()) if g.size else 0.0
        e = int(np.frexp(m)[1]) if m > 0 else 0
        q[lv] = 2.0 ** -(min(62 - L, 46) - e)
    return q


def scatter_close(got, t, meta, g, n, levels=None, outside=None, what=''):
    """table gradient of xr_hashgrid_bwd against table_grad64's dict `t` (g: the gradient it was built from, n: the launch's row
    count), every entry of the launched levels against its own bound; entries outside the levels must hold `outside` (the table
    before the launch, default zeros) bit for bit"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    l0, l1 = (0, meta.n_levels) if levels is None else levels
    kinds = level_kinds(meta, n)
    q = quantum(g, meta, n)
    a_rl = CONTRIB + ((RL_ROWS - 1) + 1 + sc_test()['rl_chunks']) * U * (1 + 2.0 ** -10)     # (30 u at the default 8 chunks; + 2nd order)
    a, b = 2 * int(meta.offset[l0]), 2 * int(meta.offset[l1])
    keep = np.zeros_like(got) if outside is None else np.asarray(outside, np.float64)
    assert np.array_equal(got[:a], keep[:a]) and np.array_equal(got[b:], keep[b:]), (what, 'entries outside the levels changed')
    worst, bad_levels = {}, []
    for lv in range(l0, l1):
        s = slice(2 * int(meta.offset[lv]), 2 * int(meta.offset[lv + 1]))
        ref, budget, c = t['ref'][s], t['budget'][s], t['count'][s]
        if kinds[lv] == 'atomic':      # fp32 atomics: the contribution, then a sum of c_i + 1 fp32 values in any order
            bound = (CONTRIB + (c + 1) * U) * budget + 2.0 ** -23 * np.abs(ref)
        else:
            bound = (a_rl if kinds[lv] == 'rl' else A_BIN) * budget + 2.0 ** -23 * np.abs(ref) + c * q[lv]
        err = np.abs(got[s] - ref)
        worst[lv] = float((err / np.where(bound > 0, bound, 1.0)).max())
        bad = np.flatnonzero(err > bound)
        if bad.size:
            bad_levels.append((lv, kinds[lv], 'entries over their bound', bad.size, 'first', int(bad[0]) + s.start, float(got[s][bad[0]]),
                               float(ref[bad[0]]), float(bound[bad[0]]), int(c[bad[0]])))
    _log(dict(check='scatter', what=what, n=n, worst={str(k): v for k, v in worst.items()}))
    assert not bad_levels, (what, bad_levels)
    return worst
