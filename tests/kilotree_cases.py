"""The bodies of the xr_kilotree_val_metrics checks, shared by the GPU tier (tests/test_gpu_kilotree.py) and the host emulation of the same
source (tests/test_emu_kilotree.py).  The specification is tests/kilotree_restatement.py; the reference's own numbers are the fixture
tests/golden/ref_kilotree.npz (tests/golden/make_golden_kilotree.py).

Bounds.  Means: 1 fp32 ulp of the restatement (the double sums differ only in order; a rounding boundary may flip).  Quantiles,
saturation, NaN and refusals: bit for bit.  Split threshold: bit for bit wherever the crossing is decided beyond the accumulator's
quantisation -- every weight is rounded to a multiple of the unit q = 2^-(61 - b - e) (max metric < 2^e, P <= 2^b), so a running sum of at
most P weights is off by at most P q / 2; the case is compared when |S_k - half| > P q for the crossing coordinate and the one before it (q counts as 0 where
every weight is a whole number of units: tied errors such as 0.25 are, and then a running sum that equals the half exactly is decided).
With q below 2^-36 of the largest weight that leaves out next to nothing: check_* count what they leave out and the callers bound it."""
import os

import numpy as np
import torch

import kilotree_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'ref_kilotree.npz')
SMALL_P = (1, 2, 63, 64, 65, 300, 1025)
# the workgroup walks a network's points 256 at a time: one either side of one and of two rounds
BLOCK_P = (255, 256, 257, 511, 512, 513)
FRACTIONS = (0.99, 0.5, 0.0)


def inputs(N, P, seed, tie_coords=False, tie_errors=False):
    """generated out / targets / points: rendered-looking values in [0, 1], points in a box"""
    rng = np.random.default_rng(seed)
    tgt = rng.random((N, P, 4)).astype(np.float32)
    out = (tgt + rng.normal(0, 0.05, (N, P, 4))).astype(np.float32)
    pts = rng.uniform(-0.8, 0.8, (N, P, 3)).astype(np.float32)
    if tie_coords:
        pts = (np.round(pts * 4) / 4).astype(np.float32)            # 7 distinct coordinates per axis, -0. among them
    if tie_errors:
        out = (tgt + np.float32(0.25) * (rng.integers(0, 3, (N, P, 1)) - 1)).astype(np.float32)
    return out, tgt, pts


def example_rows(dev, out, tgt, pts):
    """the layout val_step hands over: targets and points are column slices of [N, P, 10] example rows"""
    N, P = out.shape[:2]
    ex = torch.zeros((N, P, 10), dtype=torch.float32)
    ex[..., 0:3], ex[..., 6:10] = torch.from_numpy(pts), torch.from_numpy(tgt)
    ex = ex.to(dev)
    return torch.from_numpy(out).to(dev), ex[..., 6:10], ex[..., 0:3]


def run(dev, out, tgt, pts, qi, axis=None, metric='mse', want_pm=False):
    from xrnerf_amd import ops
    o, t, p = example_rows(dev, out, tgt, pts)
    table, pm = ops.kilo_val_metrics(o, t, qi, points=p if axis is not None else None, split_axis=axis, split_metric=metric, want_point_metric=want_pm)
    return table.cpu().numpy(), None if pm is None else pm.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def ulps(got, want):
    """distance in fp32 steps between finite values of one sign (inf for a NaN on one side only, 0 for NaN on both)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    d = np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64)).astype(np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    d[np.isnan(got) ^ np.isnan(want)] = np.inf
    d[both_nan] = 0
    return d


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert np.array_equal(g, w), '%s: %r against %r' % (what, np.asarray(got).ravel()[:8], np.asarray(want).ravel()[:8])


def compare(got, want, P, what):
    """got: the kernel's table; want: the restatement's dict.  -> the number of split cases the quantisation condition leaves out"""
    t = want['table']
    print('%s: worst mean distance %g ulp' % (what, ulps(got[:, :9], t[:, :9]).max()))
    assert (ulps(got[:, :9], t[:, :9]) <= 1).all(), '%s: means\n%r\n%r' % (what, got[:, :9], t[:, :9])
    same_bits(got[:, R.QUANTILE:R.QUANTILE + 3], t[:, R.QUANTILE:R.QUANTILE + 3], what + ': quantile_se')
    same_bits(got[:, R.SATURATION], t[:, R.SATURATION], what + ': saturation')
    same_bits(got[:, R.METRIC_MAX:], t[:, R.METRIC_MAX:], what + ': metric max')
    decided = (want['margin'] > P * want['unit']) | ((want['unit'] == 0) & np.isfinite(want['margin']))
    same_bits(got[decided, R.THRESHOLD], t[decided, R.THRESHOLD], what + ': split threshold')
    return int((~decided).sum())


def check_shape(dev, N, P, seed=0):
    """every fraction, every split metric and axis at one shape, against the restatement"""
    out, tgt, pts = inputs(N, P, 1000 * N + P + seed)
    left_out = 0
    for i, frac in enumerate(FRACTIONS):
        qi = int(P * frac)
        metric = R.METRICS[i % 3]
        axis = [(n + i) % 3 for n in range(N)]
        got, pm = run(dev, out, tgt, pts, qi, axis, metric, want_pm=True)
        want = R.val_metrics(out, tgt, qi, pts, axis, metric)
        left_out += compare(got, want, P, 'N %d P %d fraction %g %s' % (N, P, frac, metric))
        same_bits(pm, want['point_metric'], 'point metric')
    assert left_out == 0, 'uniform random inputs never sit within P q of the half: %d did' % left_out


def check_ties(dev):
    """tied coordinates (the crossing falls inside a group of equal coordinates: the group's coordinate comes back whatever the order),
    tied errors (the order statistic sits in a run of equal values)"""
    for N, P in ((5, 300), (2, 1025)):
        for tc, te in ((True, False), (False, True), (True, True)):
            out, tgt, pts = inputs(N, P, 7 + P, tie_coords=tc, tie_errors=te)
            for ax in range(3):
                axis = [ax] * N
                got, _ = run(dev, out, tgt, pts, P // 2, axis, 'mae')
                assert compare(got, R.val_metrics(out, tgt, P // 2, pts, axis, 'mae'), P, 'ties %s %s axis %d' % (tc, te, ax)) == 0


def check_odd_values(dev):
    """a NaN in out, a zero-total network, split_axis = -1 and no split_axis at all"""
    N, P = 5, 300
    out, tgt, pts = inputs(N, P, 11)
    out[1, 17, 2] = np.nan                       # colour: total and colour quantiles see a NaN at the top rank, density does not
    out[2] = tgt[2]                              # zero total
    out[3, 5, 3] = np.inf
    axis = [0, 1, 2, 1, -1]
    for qi in (0, P - 1):
        for metric in R.METRICS:
            got, _ = run(dev, out, tgt, pts, qi, axis, metric)
            want = R.val_metrics(out, tgt, qi, pts, axis, metric)
            assert compare(got, want, P, 'odd values rank %d %s' % (qi, metric)) == 0
            assert np.isnan(got[[1, 2, 3, 4], R.THRESHOLD]).all() and not np.isnan(got[0, R.THRESHOLD])
    assert np.isnan(got[1, R.QUANTILE]) and np.isnan(got[1, R.QUANTILE + 1]) and not np.isnan(got[1, R.QUANTILE + 2])
    got, _ = run(dev, out, tgt, pts, 3, None)
    want = R.val_metrics(out, tgt, 3)
    compare(got, want, P, 'no split')
    assert np.isnan(got[:, R.THRESHOLD]).all()


def saturation_rows():
    """crafted rows, P = 70 (more than a wave): (out, targets, expected flag)"""
    P = 70
    rng = np.random.default_rng(5)
    base_t = (0.2 + 0.6 * rng.random((P, 4))).astype(np.float32)
    rows = []

    def row(edit, flag):
        o, t = (base_t + np.float32(0.01)).astype(np.float32), base_t.copy()
        edit(o, t)
        rows.append((o, t, flag))
    row(lambda o, t: None, False)

    def zero_out(o, t): o[:, 1] = 0.0005
    row(zero_out, True)                                    # channel 1 all below tolerance, target not

    def zero_both(o, t): o[:, 1] = 0.0005; t[:, 1] = -0.0005
    row(zero_both, False)                                  # ... and the target agrees

    def zero_but_one(o, t): o[:, 1] = 0.0005; o[P - 1, 1] = 0.002
    row(zero_but_one, False)                               # one point (in the second wave) breaks the all

    def one_out(o, t): o[:, 2] = 0.9995
    row(one_out, True)

    def one_both(o, t): o[:, 2] = 1.0005; t[:, 2] = 0.9995
    row(one_both, False)

    def one_but_one(o, t): o[:, 2] = 0.9995; o[0, 2] = 0.99
    row(one_but_one, False)

    def target_but_one(o, t): o[:, 0] = 0.0; t[:, 0] = 0.0; t[33, 0] = 0.5
    row(target_but_one, True)                              # the target's all broken by one point: saturated

    def density_only(o, t): o[:, 3] = 0.0
    row(density_only, False)                               # the density channel does not count

    def at_tolerance(o, t): o[:, 0] = np.float32(0.001)
    row(at_tolerance, False)                               # |out| < tol is strict
    return rows


def check_saturation(dev):
    rows = saturation_rows()
    out = np.stack([r[0] for r in rows])
    tgt = np.stack([r[1] for r in rows])
    got, _ = run(dev, out, tgt, np.zeros(out.shape[:2] + (3,), np.float32), 0)
    want = np.array([1.0 if r[2] else 0.0 for r in rows], np.float32)
    assert np.array_equal(got[:, R.SATURATION], want), (got[:, R.SATURATION], want)
    assert np.array_equal(R.val_metrics(out, tgt, 0)['table'][:, R.SATURATION], want)


def check_repeat_and_permutation(dev):
    """two runs give the same bits; permuting a network's points changes no output bit"""
    for N, P in ((5, 1025), (2, 300)):
        out, tgt, pts = inputs(N, P, 23, tie_coords=True)
        axis = [n % 3 for n in range(N)]
        a, _ = run(dev, out, tgt, pts, int(P * 0.99), axis, 'mape')
        b, _ = run(dev, out, tgt, pts, int(P * 0.99), axis, 'mape')
        same_bits(a, b, 'two runs')
        perm = np.random.default_rng(3).permutation(P)
        c, _ = run(dev, out[:, perm], tgt[:, perm], pts[:, perm], int(P * 0.99), axis, 'mape')
        same_bits(a, c, 'permuted points')


def check_refusals(dev):
    from xrnerf_amd import _lib
    out, tgt, pts = inputs(2, 10, 1)
    for qi in (-1, 10, 11):
        try:
            run(dev, out, tgt, pts, qi, [0, 1])
        except _lib.XrError as e:
            assert '-22' in str(e), e
        else:
            raise AssertionError('quantile_index %d was accepted' % qi)
    try:
        run(dev, out, tgt, pts, 0, [0, 1], 'rmse')
    except _lib.XrError:
        pass
    else:
        raise AssertionError('an unknown split metric was accepted')


# ------------------------------------------------------------------ the reference's own numbers
def gold():
    return np.load(GOLD)


def check_reference_metrics(dev, key):
    """case `key` of the fixture: calculate_error_metrics and get_equal_error_split_threshold of the reference on generated inputs.
    A mean may be as far from the reference as the reference is from the restatement, plus 1 ulp; the density quantile is the reference's
    bit for bit; total and colour quantiles within 4 * 2^-24 relative (the reference's fp32 channel mean carries at most three roundings,
    and an order statistic moves no further than its inputs)."""
    g = gold()
    if key + '.out' in g.files:
        out, tgt, pts = g[key + '.out'], g[key + '.targets'], g[key + '.points']
    else:                                         # too large to commit: generated again, and checked to be what the reference saw
        import hashlib
        import kilotree_scenarios as S
        P = int(key[1:])
        out, tgt, pts = inputs(g[key + '.table'].shape[0], P, S.metric_seed(P))
        h = hashlib.sha256()
        for a in (out, tgt, pts):
            h.update(np.ascontiguousarray(a).tobytes())
        assert h.hexdigest() == str(g[key + '.sha256']), 'the generated inputs of %s are not the ones the fixture was made from' % key
    N, P = out.shape[:2]
    qi = int(g[key + '.quantile_index'])
    ref = g[key + '.table']                       # [N, 12]: the reference's nine means and three quantiles
    for ax in range(3):
        got, _ = run(dev, out, tgt, pts, qi, [ax] * N, 'mse')
        want = R.val_metrics(out, tgt, qi, pts, [ax] * N, 'mse')
        compare(got, want, P, '%s axis %d' % (key, ax))
        if ax == 0:
            with np.errstate(all='ignore'):
                allowed = np.abs(ref[:, :9].astype(np.float64) - want['exact']) + np.spacing(np.abs(ref[:, :9])).astype(np.float64)
                dist = np.abs(got[:, :9].astype(np.float64) - ref[:, :9].astype(np.float64))
            print('%s: means, worst distance / allowed %g' % (key, np.nanmax(dist / allowed)))
            assert (dist <= allowed).all(), (dist, allowed)
            same_bits(got[:, R.QUANTILE + 2], ref[:, 11], key + ': density quantile against the reference')
            rel = np.abs(got[:, R.QUANTILE:R.QUANTILE + 2].astype(np.float64) - ref[:, 9:11]) / np.abs(ref[:, 9:11]).astype(np.float64)
            print('%s: quantiles, worst relative distance %g' % (key, rel.max()))
            assert (rel <= 4 * 2.0 ** -24).all(), rel
            same_bits(got[:, R.SATURATION], g[key + '.saturation'].astype(np.float32), key + ': saturation against the reference')
        if P <= 1025:
            same_bits(got[:, R.THRESHOLD], g[key + '.threshold'][:, ax], '%s axis %d: threshold against the reference' % (key, ax))
