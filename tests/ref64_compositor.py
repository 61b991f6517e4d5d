"""TEST INFRASTRUCTURE ONLY (numpy): the Instant-NGP compositor (calc_rgb.cu:20-66 forward, :87-139 backward, :158-205 inference) in
float64, ray by ray, with a first-order running bound of the fp32 rounding error of every number a kernel writes.

The formula itself is ill-conditioned in fp32 -- alpha = 1 - expf(-x) has an ABSOLUTE error of about u, T *= (1 - alpha) reaches
exactly 0 while the true product is ~1e-8, the density gradient takes suffix = final - prefix (nearly equal sums), s(1 - s) cancels
-- so a bar built from |ref| or from sum |w c| is off by factors up to 1/u.  Instead the error of every intermediate is carried
beside its value, in units of u = 2^-24:

    dt = dtw (MAXW - MIN) + MIN      sigma = act_d(raw_w)     c = act_rgb(raw_xyz)     x = sigma dt     q = exp(-x)    alpha = 1 - q
    rho(v, act) = 0 (None / ReLU), 4 + 1.5 |v| (Logistic / Exponential)      relative error of an activation or its derivative; the
                                                                            |v| term is the fast exp's argument rounding
    eq      = 1 + x q (3 + rho(raw_w, act_d))                               absolute error of 1 - alpha
    tau     = 2^-102 (FLT_MIN / u: fp32 flushes to zero)
    T_0 = 1, eT_0 = tau;  T_{k+1} = T_k q_k;  eT_{k+1} = eT_k q_k + T_k eq_k + T_{k+1} + tau
    w  = alpha T_k          ew = eT_k alpha + T_k eq + w          ec = |c| rho(raw_c, act_rgb)
    C_k = sum_{j<=k} w_j c_j          eC_k = sum_{j<=k} (ew_j |c_j| + w_j ec_j + 2 w_j |c_j| + |C_j|)
    F  = C_{n-1} (+ T_n bg)           eF = eC_{n-1} (+ (eT_n + 2 T_n) |bg|) + |F|

and for the backward, with Ftilde = the fp32 final colour the kernel is given (the fused kernels: their own rgb_out), g = the fp32
dL/drgb it is given (the fused kernels: scale * Huber' in float64 at Ftilde and the fp32 target), ls = 128 / n_rays:

    d_c = ls (w g_c act_rgb'(raw_c) + max(0, l2 raw_c))
    e_c = ls (ew |g_c| act_rgb' + |w g_c act_rgb'| (3 + rho) + [Logistic] 2 |w g_c| + 2 max(0, l2 raw_c)) + |d_c|
    s = Ftilde - C_k     t_c = T_{k+1} c - s     dot = sum_c g_c t_c
    e_dot = sum_c |g_c| (eT_{k+1} |c| + T_{k+1} ec + eC_k + 3 (|T_{k+1} c| + |s|)) + 3 sum_c |g_c t_c|
    d_w = ls act_d' dt dot - [raw_w < 0] l1
    e_w = ls act_d' dt (e_dot + |dot| (6 + rho)) + [Logistic] 2 ls dt |dot| + |d_w| + [raw_w < 0] l1

A kernel passes when |got - ref| <= 2 u e for EVERY element it writes: 1 is the derived factor, the second 1 is for second-order
terms and the GPU's v_exp_f32 against libm.  It is not a measured budget (the sequential fp32 oracle sits at 0.73 on the cases of
tests/compositor_cases.py, its rgb at 0.46: profiles/compositor_f64_bounds.txt).  A row beyond it means a wrong kernel, or an fp32
operation the recursion does not name -- then that term is added here, by name; the factor stays."""
import numpy as np

U = 2.0 ** -24
TAU = 2.0 ** -102
FACTOR = 2.0
# xr_common.h's constants: their float32 values, taken to float64
MIN_STEP = np.float64(np.float32(1.73205080757) / np.float32(1024))
MAX_WARP_STEP = np.float64(np.float32(np.float32(1.73205080757) / np.float32(1024)) * np.float32(128))
WARP_SPAN = np.float64(np.float32(MAX_WARP_STEP) - np.float32(MIN_STEP))
L_REG = np.float64(np.float32(1e-4))            # l1 / l2 (calc_rgb.cu:103-104)
NONE, RELU, LOGISTIC, EXPONENTIAL = 0, 1, 2, 3


def _logistic(v):
    e = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def act(v, a, clamp=None):
    """an activation; `clamp`: the Exponential's argument clamp (10 for rgb; the density's forward has none)"""
    if a == NONE:
        return v.copy()
    if a == RELU:
        return np.maximum(v, 0.0)
    if a == LOGISTIC:
        return _logistic(v)
    return np.exp(v if clamp is None else np.clip(v, -clamp, clamp))


def dact(v, a, clamp):
    """its derivative (Exponential: clamp 10 for rgb, 15 for the density)"""
    if a == NONE:
        return np.ones_like(v)
    if a == RELU:
        return (v > 0).astype(np.float64)
    if a == LOGISTIC:
        e = np.exp(-np.abs(v))
        return e / ((1.0 + e) * (1.0 + e))        # s (1 - s) without the cancellation
    return np.exp(np.clip(v, -clamp, clamp))


def rho(v, a):
    return np.zeros_like(v) if a in (NONE, RELU) else 4.0 + 1.5 * np.abs(v)


class Walk:
    """every sample of every ray, front to back over the UNCOMPACTED counts: a ray clipped to n samples ends at row n - 1 of the same walk"""

    def __init__(self, raw, coords, numsteps, rgb_act, density_act):
        raw = np.asarray(raw, np.float64)
        ns = np.asarray(numsteps, np.int64)
        S = raw.shape[0]
        self.rgb_act, self.density_act, self.n_rays, self.S = rgb_act, density_act, ns.shape[0], S
        self.raw = raw
        self.dt = np.asarray(coords, np.float64)[:S, 3] * WARP_SPAN + MIN_STEP
        sigma = act(raw[:, 3], density_act)
        self.c = act(raw[:, :3], rgb_act, 10.0)
        x = sigma * self.dt
        q = np.exp(-x)
        alpha = -np.expm1(-x)
        self.rho_w = rho(raw[:, 3], density_act)
        self.rho_c = rho(raw[:, :3], rgb_act)
        xq = np.where(q > 0, x * q, 0.0)
        eq = 1.0 + xq * (3.0 + self.rho_w)
        self.ec = np.abs(self.c) * self.rho_c
        z = lambda *s: np.zeros(s, np.float64)
        self.T0, self.T1, self.eT0, self.eT1, self.w, self.ew = z(S), z(S), z(S), z(S), z(S), z(S)
        self.C, self.eC = z(S, 3), z(S, 3)
        self.ray = np.full(S, -1, np.int64)
        self.k = np.zeros(S, np.int64)
        for i in range(ns.shape[0]):
            n, b = int(ns[i, 0]), int(ns[i, 1])
            if n == 0:
                continue
            sl = slice(b, b + n)
            self.ray[sl] = i
            self.k[sl] = np.arange(n)
            T1 = np.cumprod(q[sl])
            T0 = np.concatenate([[1.0], T1[:-1]])
            e, e0, e1 = TAU, [], []
            for qk, t0, t1, eqk in zip(q[sl].tolist(), T0.tolist(), T1.tolist(), eq[sl].tolist()):
                e0.append(e)
                e = e * qk + t0 * eqk + t1 + TAU
                e1.append(e)
            e0, e1 = np.array(e0), np.array(e1)
            w = alpha[sl] * T0
            ew = e0 * alpha[sl] + T0 * eq[sl] + w
            c, ac = self.c[sl], np.abs(self.c[sl])
            C = np.cumsum(w[:, None] * c, 0)
            eC = np.cumsum(ew[:, None] * ac + w[:, None] * self.ec[sl] + 2.0 * w[:, None] * ac + np.abs(C), 0)
            self.T0[sl], self.T1[sl], self.eT0[sl], self.eT1[sl], self.w[sl], self.ew[sl] = T0, T1, e0, e1, w, ew
            self.C[sl], self.eC[sl] = C, eC
        for a in (self.T1, self.eT1, self.C, self.eC):
            assert np.isfinite(a).all()

    def ends(self, counts_bases):
        """-> (C, eC, T, eT, empty) per ray at the given (count, base) pairs: C_{n-1}, eC_{n-1}, T_n, eT_n"""
        cb = np.asarray(counts_bases, np.int64)
        n, b = cb[:, 0], cb[:, 1]
        empty = n == 0
        last = np.where(empty, 0, b + n - 1)
        m = (~empty)[:, None]
        return (np.where(m, self.C[last], 0.0), np.where(m, self.eC[last], 0.0), np.where(empty, 1.0, self.T1[last]),
                np.where(empty, TAU, self.eT1[last]), empty)

    def forward(self, counts_bases, bg, add_bg):
        """-> (F, eF, empty): the final colour at the given counts, the background added where `add_bg`; rays without samples are the
        background exactly (e = 0)"""
        C, eC, T, eT, empty = self.ends(counts_bases)
        bg = np.broadcast_to(np.asarray(bg, np.float64), C.shape)
        add = (np.asarray(add_bg, bool) & ~empty)[:, None]
        F = C + np.where(add, T[:, None] * bg, 0.0)
        eF = eC + np.where(add, (eT + 2.0 * T)[:, None] * np.abs(bg), 0.0) + np.abs(F)
        F = np.where(empty[:, None], bg, F)
        eF = np.where(empty[:, None], 0.0, eF)
        return F, eF, empty

    def alpha_out(self, counts_bases):
        """inference: 1 - T_n, bound eT_n + 1 (exactly 0 for a ray without samples)"""
        _, _, T, eT, empty = self.ends(counts_bases)
        return np.where(empty, 0.0, 1.0 - T), np.where(empty, 0.0, eT + 1.0)

    def written(self, counts_bases):
        """mask of the rows a backward writes: k < n of the row's ray"""
        n = np.asarray(counts_bases, np.int64)[:, 0]
        return (self.ray >= 0) & (self.k < n[np.maximum(self.ray, 0)])

    def backward(self, counts_bases, f_tilde, g, density_grid_mean):
        """-> (d, e, written): dL/d(raw) [S, 4] over the written rows (zero elsewhere)"""
        wr = self.written(counts_bases)
        r = np.maximum(self.ray, 0)
        Ft, g = np.asarray(f_tilde, np.float64)[r], np.asarray(g, np.float64)[r]
        ls = 128.0 / self.n_rays
        l2 = L_REG if self.rgb_act == EXPONENTIAL else 0.0
        l1 = L_REG if np.float32(density_grid_mean) < np.float32(0.01) else 0.0
        raw, w, ew = self.raw, self.w[:, None], self.ew[:, None]
        da_c = dact(raw[:, :3], self.rgb_act, 10.0)
        reg = np.maximum(0.0, l2 * raw[:, :3])
        d = np.zeros((self.S, 4))
        e = np.zeros((self.S, 4))
        d[:, :3] = ls * (w * g * da_c + reg)
        lg_c = 2.0 * np.abs(w * g) if self.rgb_act == LOGISTIC else 0.0
        e[:, :3] = ls * (ew * np.abs(g) * da_c + np.abs(w * g * da_c) * (3.0 + self.rho_c) + lg_c + 2.0 * reg) + np.abs(d[:, :3])
        T1, eT1 = self.T1[:, None], self.eT1[:, None]
        s = Ft - self.C
        t = T1 * self.c - s
        dot = (g * t).sum(1)
        e_dot = (np.abs(g) * (eT1 * np.abs(self.c) + T1 * self.ec + self.eC + 3.0 * (np.abs(T1 * self.c) + np.abs(s)))).sum(1) \
            + 3.0 * np.abs(g * t).sum(1)
        da_w = dact(raw[:, 3], self.density_act, 15.0)
        neg = (raw[:, 3] < 0) * l1
        d[:, 3] = ls * da_w * self.dt * dot - neg
        lg_w = 2.0 * ls * self.dt * np.abs(dot) if self.density_act == LOGISTIC else 0.0
        e[:, 3] = ls * da_w * self.dt * (e_dot + np.abs(dot) * (6.0 + self.rho_w)) + lg_w + np.abs(d[:, 3]) + neg
        d[~wr] = 0.0
        e[~wr] = 0.0
        assert np.isfinite(d).all() and np.isfinite(e).all()
        return d, e, wr


def huber_grad(f_tilde, target, delta=0.1, scale=5.0):
    """scale * Huber'(Ftilde - target) in float64 (utils/metrics.py:8-16); delta as the fp32 number the kernel is handed"""
    d = np.asarray(f_tilde, np.float64) - np.asarray(target, np.float64)
    dl = np.float64(np.float32(delta))
    return scale * np.where(np.abs(d) > dl, np.sign(d), d / dl)


def loss_scalars(rgb, target, alpha_mask, delta=0.1, scale=5.0):
    """-> (scale * sum HuberLoss, sum ((rgb - target) alpha)^2) in float64 over the given (the kernel's own) rgb"""
    d = np.asarray(rgb, np.float64) - np.asarray(target, np.float64)
    dl = np.float64(np.float32(delta))
    a = np.abs(d)
    hub = np.where(a > dl, a - 0.5 * dl, 0.5 / dl * a * a).sum()
    return scale * hub, ((d * np.asarray(alpha_mask, np.float64).reshape(-1, 1)) ** 2).sum()


def ratio(got, ref, e):
    """|got - ref| / (u e) per element; where the bound is 0 the number must be exact (-> 0 or inf)"""
    got, ref, e = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(e, np.float64)
    assert got.shape == ref.shape == e.shape
    if not np.isfinite(got).all():
        return np.inf
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(e > 0, err / (U * e), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0
