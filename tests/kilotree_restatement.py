"""The float64 restatement of include/xrnerf_mi355_kilotree.h in numpy: what xr_kilotree_val_metrics must give per network.  The
per-element errors are fp32 exactly as the tensor ops form them (d = a - b; d d; |d|; |d| / (|t| + 0.1f)); every sum over them is float64,
divided once and rounded to fp32 once; the order statistics and the split threshold are defined on values, not on a permutation."""
import math

import numpy as np

F32 = np.float32
COLS = 16
MSE, MAE, MAPE, QUANTILE, SATURATION, THRESHOLD, METRIC_MAX = 0, 3, 6, 9, 12, 13, 14
METRICS = ('mse', 'mae', 'mape')
CANONICAL_NAN = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]


def element_errors(out, tgt):
    """out, tgt [P, 4] fp32 -> dict of [P, 4] fp32"""
    out, tgt = np.asarray(out, F32), np.asarray(tgt, F32)
    with np.errstate(all='ignore'):
        d = out - tgt
        ae = np.abs(d)
        return {'mse': d * d, 'mae': ae, 'mape': ae / (np.abs(tgt) + F32(0.1))}


def mean4(x):
    """[P, 4] fp32 -> [P] fp32: (float)((((x0 + x1) + x2) + x3) / 4.0), the sum in float64"""
    x = x.astype(np.float64)
    with np.errstate(all='ignore'):
        return ((((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]) / 4.0).astype(F32)


def mean3(x):
    x = x.astype(np.float64)
    with np.errstate(all='ignore'):
        return (((x[:, 0] + x[:, 1]) + x[:, 2]) / 3.0).astype(F32)


def means(x):
    """[P, 4] fp32 -> (all, colour, density) as float64 BEFORE the rounding to fp32, sums by math.fsum (exact, so order-free)"""
    P = x.shape[0]
    c = [math.fsum(x[:, k].astype(np.float64).tolist()) if np.isfinite(x[:, k]).all() else float(x[:, k].astype(np.float64).sum()) for k in range(4)]
    colour = (c[0] + c[1]) + c[2]
    return (colour + c[3]) / (4.0 * P), colour / (3.0 * P), c[3] / float(P)


def order_statistic(v, rank):
    """rank-th smallest of v [P] fp32, NaN last (numpy's and torch's sort order); a NaN comes back canonical"""
    r = np.sort(np.asarray(v, F32))[rank]
    return CANONICAL_NAN if r != r else r


def saturation(out, tgt):
    out, tgt = np.asarray(out, F32)[:, :3], np.asarray(tgt, F32)[:, :3]
    tol = F32(0.001)
    with np.errstate(all='ignore'):
        o0, t0 = (np.abs(out) < tol).all(0), (np.abs(tgt) < tol).all(0)
        o1, t1 = (np.abs(out - F32(1)) < tol).all(0), (np.abs(tgt - F32(1)) < tol).all(0)
    return bool(((o0 & ~t0) | (o1 & ~t1)).any())


def fixed_unit(m, P):
    """one unit of the kernel's 64-bit fixed-point weights: 1 / 2^(61 - b - e), max m < 2^e, P <= 2^b"""
    mmax = float(np.max(m))
    _, e = math.frexp(mmax)
    b = 0
    while (1 << b) < P:
        b += 1
    return math.ldexp(1.0, -(61 - b - e))


def split_threshold(coords, m):
    """coords [P] fp32, m [P] fp32 (per-point metric) -> (threshold fp32 or NaN, margin): the smallest coordinate c whose running sum
    W(c) = sum of m over the points with coordinate <= c exceeds half the total, in exact arithmetic (math.fsum); margin = the smaller of
    |W - half| at that coordinate and at the one before it (what decides whether a quantised accumulator must agree)"""
    coords, m = np.asarray(coords, F32) + F32(0), np.asarray(m, F32)
    if not np.isfinite(m).all() or not (m.max() > 0):
        return CANONICAL_NAN, float('inf')
    order = np.argsort(coords, kind='stable')
    cs, ms = coords[order], m[order].astype(np.float64)
    half = math.fsum(ms.tolist()) / 2.0
    uniq, start = np.unique(cs, return_index=True)
    ends = list(start[1:]) + [len(cs)]
    prev = 0.0
    run = []
    for u, s0, s1 in zip(uniq, start, ends):
        run.append(math.fsum([prev] + ms[s0:s1].tolist()))
        prev = run[-1]
        if prev > half:
            k = len(run) - 1
            margin = abs(run[k] - half)
            if k > 0:
                margin = min(margin, abs(run[k - 1] - half))
            else:
                margin = min(margin, half)
            return F32(u), margin
    raise AssertionError('no crossing: unreachable with a positive total')


def val_metrics(out, tgt, quantile_index, points=None, split_axis=None, split_metric='mse'):
    """out, tgt [N, P, 4], points [N, P, 3], split_axis [N] ints or None -> dict:
    table [N, 16] fp32 (the kernel's columns), exact [N, 9] float64 (the means before rounding), point_metric [N, P] fp32,
    margin [N] (split decision margins, inf where no split), unit [N] (the fixed-point unit; 0 where no split, and where every weight is
    a whole number of units, so that nothing is rounded)"""
    out, tgt = np.asarray(out, F32), np.asarray(tgt, F32)
    N, P = out.shape[:2]
    if not 0 <= quantile_index < P:
        raise IndexError('quantile_index %d outside [0, %d)' % (quantile_index, P))
    table = np.zeros((N, COLS), F32)
    exact = np.zeros((N, 9), np.float64)
    pm = np.zeros((N, P), F32)
    margin, unit = np.full((N,), np.inf), np.zeros((N,))
    for n in range(N):
        e = element_errors(out[n], tgt[n])
        for mi, k in enumerate(METRICS):
            exact[n, 3 * mi:3 * mi + 3] = means(e[k])
        with np.errstate(all='ignore'):
            table[n, :9] = exact[n].astype(F32)
        table[n, QUANTILE] = order_statistic(mean4(e['mse']), quantile_index)
        table[n, QUANTILE + 1] = order_statistic(mean3(e['mse']), quantile_index)
        table[n, QUANTILE + 2] = order_statistic(e['mse'][:, 3], quantile_index)
        table[n, SATURATION] = 1.0 if saturation(out[n], tgt[n]) else 0.0
        pm[n] = mean4(e[split_metric])
        table[n, THRESHOLD] = CANONICAL_NAN
        ax = -1 if split_axis is None else int(split_axis[n])
        if 0 <= ax <= 2:
            finite = pm[n][np.isfinite(pm[n])]
            table[n, METRIC_MAX] = finite.max() if finite.size else 0.0
            table[n, THRESHOLD], margin[n] = split_threshold(np.asarray(points, F32)[n, :, ax], pm[n])
            if np.isfinite(pm[n]).all() and pm[n].max() > 0:
                unit[n] = fixed_unit(pm[n], P)
                if not ((pm[n].astype(np.float64) / unit[n]) % 1.0).any():
                    unit[n] = 0.0               # every weight is a whole number of units: the integer running sum is exact
    return {'table': table, 'exact': exact, 'point_metric': pm, 'margin': margin, 'unit': unit}
