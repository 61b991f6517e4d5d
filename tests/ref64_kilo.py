"""TEST INFRASTRUCTURE ONLY: float64 reference of the KiloNeRF tiny MLPs (xrnerf_amd/csrc/xr_kilo.hip: k_kilo_mlp, k_kilo_mlp_bwd,
k_kilo_student_step, k_kilo_student_fwd), ONE network at a time over exactly the samples assigned to it, in plain numpy: no tiles, no
lanes, no padded slots.  Beside every value it returns a first-order running bound of the error an fp32 evaluation may show against it.

The one float32 step: the local coordinates.  The reference (transforms.py:35-45) and the kernel both evaluate the float32 statement
((2 (p - lo)) / (hi - lo)) - 1 with one rounding per operation (the kernel source is built without contraction), so `local_x` does the same
in numpy float32 and the value is the kernel's bit for bit: at frequency k a feature amplifies an error in x by 2^k.  Everything after it is
float64.

Constants of the bounds -- none is measured on the code under test:
  U      = 2^-24, the unit roundoff of fp32 round-to-nearest.  The fp32 MFMA is a k-ordered chain of fp32 fused multiply-adds with one
           rounding per step and no wider accumulator (the CDNA programming guide, "FP32-input MFMA: exact f32 at the vector rate":
           "bit-for-bit a k-ordered f32 fmaf chain ... one rounding per product"), i.e. it rounds to nearest: U is not doubled for it.
  gamma(n) = n U / (1 - n U): the classical bound of a sum of n rounded terms in ANY order (Higham, Accuracy and Stability of Numerical
           Algorithms, lemma 3.1 / section 4.2), so it holds for the MFMA chain, the butterfly sums and the float atomics alike.
  S_TRIG = 2: ulp error taken for sincosf.  HIP's math-API accuracy table is not shipped with the toolkit this suite runs against; 2 ulp
           is ASSUMED (the published table lists 1 ulp for sinf / cosf / sincosf).  A cos / sin value is below 1 in magnitude, so one ulp is
           at most U: the absolute error of a feature is S_TRIG U.  The argument x 2^k is exact (a power-of-two scaling).
  S_EXP  = 2: ulp error taken for expf (same source, published 1 ulp); an ulp is at most 2 U relative.
  sqrtf, the division and every single fp32 operation: correctly rounded, relative U each.
Rules (e_* are absolute bounds, all first order):
  layer z = W^T h + b with K inputs: its OWN term is gamma(K + 1) (|W|^T |h| + |b|) (+ |W|^T e for inputs that carry a sincosf error); the
    heads use the same rule.  What a node inherits is NOT |W|^T e_h layer after layer -- that multiplies by the 1-norm of every layer (about
    16 x per layer here: 0.05 on raw at (10, 4, 2), 5 000 at (16, 16, 8)) -- but each earlier node's own term carried through the SIGNED
    Jacobian between the two nodes (the product of W^T diag(relu') of the sample, the points being kink-free), absolute value taken at the
    end: e_m = own_m + sum_(l < m) |d node_m / d node_l| own_l.  Still a first-order bound for every sign pattern of the local roundings.
  deltas: the same with W transposed (the Jacobians are the forward's, transposed)
  weight gradient sum_n a_n d_n over a network's n samples:  sum_n (|a_n| e_d + e_a |d_n|) + gamma(n + 1) sum_n |a_n| |d_n|; bias: a = 1, e_a = 0
Kink margins: |z| / e_z of every hidden and direction-layer unit (and of the alpha pre-activation for the students' leaky_relu)."""
import numpy as np

U = 2.0 ** -24
S_TRIG = 2.0
S_EXP = 2.0
H = 32


def gamma(n):
    return n * U / (1.0 - n * U)


def local_x(p, lo, hi):
    """float32, one rounding per operation: the kernel's bits"""
    p, lo, hi = np.asarray(p, np.float32), np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return ((np.float32(2.0) * (p - lo)) / (hi - lo)) - np.float32(1.0)


def fourier(x, n_freq, drop=None):
    """[n, 3] float32 -> features [n, 3 (2F + 1)] float64 in the order x | cos(x 2^k) | sin(x 2^k) per channel, and their error bounds.
    drop = (channel or None for all three, 'sin' | 'cos', k): that feature is left out (zero) -- only the mutation checks use it."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = x.shape[0]
    f, e = [], []
    for c in range(3):
        f.append(x[:, c:c + 1]); e.append(np.zeros((n, 1)))
        arg = x[:, c:c + 1] * (2.0 ** np.arange(n_freq))[None, :]
        for name, fn in (('cos', np.cos), ('sin', np.sin)):
            v = fn(arg)
            if drop is not None and drop[0] in (None, c) and drop[1] == name:
                v[:, drop[2]] = 0.0
            f.append(v); e.append(np.full((n, n_freq), S_TRIG * U))
    return np.concatenate(f, 1), np.concatenate(e, 1)


def _margin(z, e):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(e > 0, np.abs(z) / e, np.inf)


class Net:
    """one network's parameters in float64: Ws / bs of the hidden layers, then (Wa, ba), (Wf, bf), (Wd, bd), (Wr, br); weights [in, out]"""

    def __init__(self, tensors, n):
        a = [np.asarray(t[n], np.float64) for t in tensors]
        self.n_hidden = len(a) // 2 - 4
        self.Ws, self.bs = a[0:2 * self.n_hidden:2], a[1:2 * self.n_hidden:2]
        self.Wa, self.ba, self.Wf, self.bf, self.Wd, self.bd, self.Wr, self.br = a[2 * self.n_hidden:]
        self.pos_freqs = (self.Ws[0].shape[0] // 3 - 1) // 2
        self.dir_freqs = ((self.Wd.shape[0] - H) // 3 - 1) // 2


def _own(W, b, h):
    """z = W^T h + b and the layer's OWN rounding term gamma(K + 1) (|W|^T |h| + |b|), with the magnitude"""
    mag = np.abs(h) @ np.abs(W) + np.abs(b)
    return h @ W + b, gamma(W.shape[0] + 1) * mag, mag


def _through(T, eps):
    """sum_k |T[n, j, k]| eps[n, k]: a source's bound carried to a later node through the SIGNED Jacobian, absolute value at the end"""
    return np.einsum('njk,nk->nj', np.abs(T), eps)


def forward(net, x, v, drop=None, drop_bias=None):
    """x [n, 3] float32 local coordinates, v [n, 3] float32 directions -> dict: raw [n, 4] (rgb, alpha) with e_raw, every node (hidden
    pre-activations, feature vector, direction-layer pre-activation) with its bound, the smallest kink margin |z| / e_z per sample, and the
    smallest |z| / (U (|W|^T |h| + |b|)) per sample (the margin in units of the unit's own layer).
    drop / drop_bias: a feature / the bias of hidden layer `drop_bias` left out -- only the mutation checks use them."""
    fx, e_fx = fourier(x, net.pos_freqs, drop)
    fv, e_fv = fourier(v, net.dir_freqs)
    n, L = fx.shape[0], net.n_hidden
    hs, zs, masks, own, S = [fx], [], [], [], []
    plain = np.full(n, np.inf)
    for l, (W, b) in enumerate(zip(net.Ws, net.bs)):
        z, e, mag = _own(W, np.zeros_like(b) if drop_bias == l else b, hs[-1])
        if l == 0:
            e = e + e_fx @ np.abs(W)                               # the features' sincosf error enters here, through one layer
        else:
            S.append(W.T[None] * masks[-1][:, None, :])            # d z_l / d z_(l-1) = W^T diag(relu')
        plain = np.minimum(plain, _margin(z, U * mag).min(1))
        zs.append(z); masks.append(z > 0); hs.append(np.maximum(z, 0.0)); own.append(e)
    hl = hs[-1]
    alpha, own_alpha, _ = _own(net.Wa, net.ba, hl)
    feat, own_feat, _ = _own(net.Wf, net.bf, hl)
    S.append(net.Wf.T[None] * masks[-1][:, None, :])
    din = np.concatenate([feat, fv], 1)
    zd, own_zd, mag = _own(net.Wd, net.bd, din)
    own_zd = own_zd + e_fv @ np.abs(net.Wd[H:])
    S.append(net.Wd[:H].T[None])
    plain = np.minimum(plain, _margin(zd, U * mag).min(1))
    maskd = zd > 0
    hd = np.maximum(zd, 0.0)
    rgb, own_rgb, _ = _own(net.Wr, net.br, hd)
    own += [own_feat, own_zd]                                      # nodes: z_0 .. z_(L-1), feat, zd
    M = L + 2
    # every node's bound: its own term + every earlier node's own term through the signed Jacobian between the two (T[m][l] = d node_m /
    # d node_l, a product of W^T diag(relu') per sample).  The Jacobians of all pairs are kept where the adjoint needs them (M <= 4).
    keep = M <= 4
    T = {}
    row = []
    e_node = [own[0]]
    for m in range(1, M):
        row = [np.matmul(S[m - 1], t) for t in row] + [np.broadcast_to(S[m - 1], (n, H, H))]
        e_node.append(own[m] + sum(_through(row[l], own[l]) for l in range(m)))
        if keep:
            for l in range(m):
                T[(m, l)] = row[l]
    margin = np.full(n, np.inf)
    for m in list(range(L)) + [M - 1]:
        margin = np.minimum(margin, _margin(([*zs, feat, zd])[m], e_node[m]).min(1))
    # the outputs: A_m = d raw / d node_m [n, 4, 32], the adjoint recursion
    A = np.zeros((n, 4, H))
    A[:, :3, :] = net.Wr.T[None] * maskd[:, None, :]
    e_raw = np.concatenate([own_rgb, own_alpha], 1) + np.einsum('nck,nk->nc', np.abs(A), own[M - 1])
    for m in range(M - 2, -1, -1):
        A = np.matmul(A, S[m])
        if m == L - 1:
            A[:, 3, :] += net.Wa[:, 0][None] * masks[-1]
        e_raw = e_raw + np.einsum('nck,nk->nc', np.abs(A), own[m])
    return dict(raw=np.concatenate([rgb, alpha], 1), e_raw=e_raw, hs=hs, zs=zs, masks=masks, maskd=maskd, e_node=e_node, T=T, din=din,
                e_fx=e_fx, e_fv=e_fv, zd=zd, hd=hd, margin=margin, plain_margin=plain,
                alpha_margin=_margin(alpha, e_raw[:, 3:4])[:, 0])


def _wgrad(a, e_a, d, e_d):
    n = a.shape[0]
    g = a.T @ d
    e = np.abs(a).T @ e_d + e_a.T @ np.abs(d) + gamma(n + 1) * (np.abs(a).T @ np.abs(d))
    return g, e


def _bgrad(d, e_d):
    n = d.shape[0]
    return d.sum(0), e_d.sum(0) + gamma(n + 1) * np.abs(d).sum(0)


def backward(net, f, draw, e_draw=None):
    """the adjoint of `forward` for dL/draw [n, 4] (rgb, alpha; e_draw its bound, zero for given data) -> (grads, bounds): lists in
    MultiNetwork.ordered_parameters() order, shapes without the network axis.  A delta's bound is its own rounding term (the layer rule with W
    transposed; what enters with dL/draw counts as the own term of the node it enters at) + every later node's own term through the transposed
    signed Jacobian between the two -- nothing is multiplied by |W| layer after layer."""
    draw = np.asarray(draw, np.float64)
    e_draw = np.zeros_like(draw) if e_draw is None else e_draw
    g_rgb, e_rgb, g_a, e_a = draw[:, :3], e_draw[:, :3], draw[:, 3:4], e_draw[:, 3:4]
    L = net.n_hidden
    M = L + 2
    T, e_node = f['T'], f['e_node']
    assert len(T) == M * (M - 1) // 2, 'the adjoint needs the Jacobians of all pairs of nodes (n_hidden <= 2)'
    d, own = [None] * M, [None] * M
    aW = np.abs
    d[M - 1] = (g_rgb @ net.Wr.T) * f['maskd']                                           # three terms per entry
    own[M - 1] = (e_rgb @ aW(net.Wr).T + gamma(4) * (aW(g_rgb) @ aW(net.Wr).T)) * f['maskd']
    d[M - 2] = d[M - 1] @ net.Wd[:H].T
    own[M - 2] = gamma(H + 1) * (aW(d[M - 1]) @ aW(net.Wd[:H]).T)
    # d hl = d feat Wf^T + g_a Wa^T: 33 terms in one sum
    d[L - 1] = (d[M - 2] @ net.Wf.T + g_a @ net.Wa.T) * f['masks'][L - 1]
    own[L - 1] = (gamma(H + 2) * (aW(d[M - 2]) @ aW(net.Wf).T + aW(g_a) @ aW(net.Wa).T) + e_a @ aW(net.Wa).T) * f['masks'][L - 1]
    for l in range(L - 2, -1, -1):
        d[l] = (d[l + 1] @ net.Ws[l + 1].T) * f['masks'][l]
        own[l] = gamma(H + 1) * (aW(d[l + 1]) @ aW(net.Ws[l + 1]).T) * f['masks'][l]
    e_d = [own[l] + sum(np.einsum('njk,nj->nk', aW(T[(m, l)]), own[m]) for m in range(l + 1, M)) for l in range(M)]
    pairs = []
    for l in range(L):
        pairs += [_wgrad(f['hs'][l], f['e_fx'] if l == 0 else e_node[l - 1], d[l], e_d[l]), _bgrad(d[l], e_d[l])]
    hl, e_hl = f['hs'][-1], e_node[L - 1]
    pairs += [_wgrad(hl, e_hl, g_a, e_a), _bgrad(g_a, e_a), _wgrad(hl, e_hl, d[M - 2], e_d[M - 2]), _bgrad(d[M - 2], e_d[M - 2])]
    pairs += [_wgrad(f['din'], np.concatenate([e_node[M - 2], f['e_fv']], 1), d[M - 1], e_d[M - 1]), _bgrad(d[M - 1], e_d[M - 1])]
    pairs += [_wgrad(f['hd'], e_node[M - 1], g_rgb, e_rgb), _bgrad(g_rgb, e_rgb)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


# ------------------------------------------------------------------------------------------ the students
def _sigmoid(o, e_o):
    """1 / (1 + exp(-o)) as the kernel forms it: expf, one addition, one division"""
    E = np.exp(-o)
    e_E = E * (e_o + 2.0 * S_EXP * U)
    s = 1.0 / (1.0 + E)
    return s, s * s * (e_E + U * (1.0 + E)) + U * s


def _alpha_out(a, e_a, ad, slope):
    """1 - exp(-act(a) ad), act = leaky_relu (slope 0.01: the students) or relu (slope 0: the teacher) -> value, bound, exp(.), its bound.
    The kernel's slope is the fp32 constant nearest to 0.01: one more U on the negative side."""
    la = np.where(a > 0, a, slope * a)
    e_la = np.where(a > 0, e_a, slope * e_a + 2.0 * U * np.abs(la))
    arg = -la * ad
    e_arg = ad * e_la + U * np.abs(arg)
    ea = np.exp(arg)
    e_ea = ea * (e_arg + 2.0 * S_EXP * U)
    return 1.0 - ea, e_ea + U * np.abs(1.0 - ea), ea, e_ea


def student_render(raw, e_raw, ad):
    """KiloNerfSimpleRender on the students' raw: sigmoid(rgb), 1 - exp(-leaky_relu(alpha, 0.01) d)"""
    ad = float(np.float32(ad))
    s, e_s = _sigmoid(raw[:, :3], e_raw[:, :3])
    oa, e_oa, _, _ = _alpha_out(raw[:, 3:4], e_raw[:, 3:4], ad, 0.01)
    return np.concatenate([s, oa], 1), np.concatenate([e_s, e_oa], 1)


def student_loss(f, teacher, ad, batch_for_scale=None):
    """both renders, the network's loss mean(mean((out - t)^2, 2), 1) and dL/draw, each with its bound.  batch_for_scale: the mutation
    checks' wrong batch size in d mean / d out."""
    raw, e_raw = f['raw'], f['e_raw']
    t = np.asarray(teacher, np.float64)
    B = raw.shape[0]
    ad = float(np.float32(ad))
    s, e_s = _sigmoid(raw[:, :3], e_raw[:, :3])
    st, e_st = _sigmoid(t[:, :3], np.zeros_like(t[:, :3]))
    oa, e_oa, ea, e_ea = _alpha_out(raw[:, 3:4], e_raw[:, 3:4], ad, 0.01)
    ta, e_ta, _, _ = _alpha_out(t[:, 3:4], np.zeros((B, 1)), ad, 0.0)
    err = np.concatenate([s - st, oa - ta], 1)
    e_err = np.concatenate([e_s + e_st, e_oa + e_ta], 1) + U * np.abs(err)
    # d out / d raw: s (1 - s) -- one subtraction, one product -- and exp(.) d slope -- two products, the slope constant on the negative side
    dsig_c = s * (1.0 - s)
    e_dsig_c = e_s * (1.0 - s) + s * (e_s + U * (1.0 - s)) + U * dsig_c
    slope = np.where(raw[:, 3:4] > 0, 1.0, 0.01)
    dsig_a = ea * ad * slope
    e_dsig_a = e_ea * ad * slope + 3.0 * U * dsig_a
    dsig, e_dsig = np.concatenate([dsig_c, dsig_a], 1), np.concatenate([e_dsig_c, e_dsig_a], 1)
    # per example (((e0^2 + e1^2) + e2^2) + e3^2) / 4: four rounded squares, three additions
    ls = (err ** 2).sum(1) / 4.0
    e_ls = (2.0 * np.abs(err) * e_err).sum(1) / 4.0 + gamma(5) * ls
    loss = ls.sum() / B
    e_loss = (e_ls.sum() + gamma(B + 1) * ls.sum()) / B + U * loss
    # dL/draw = ((2 / (4 B)) err) dsig: the scale's division and two products
    dscale = 2.0 / (4.0 * (B if batch_for_scale is None else batch_for_scale))
    gr = dscale * err * dsig
    e_gr = dscale * (e_err * dsig + np.abs(err) * e_dsig) + 3.0 * U * np.abs(gr)
    return dict(loss=loss, e_loss=e_loss, draw=gr, e_draw=e_gr)


def adam(p, m, v, g, e_g, step, lr, b1, b2, eps):
    """torch.optim.Adam's update in float64 (bias corrections 1 - beta^t, denominator sqrt(v) / sqrt(1 - beta2^t) + eps) on the float64
    gradient, with the bound of an fp32 evaluation of m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) g g, p <- p - step_size (m / (sqrt(v) /
    bc2s + eps)).  The hyper-parameters are the fp32 values the C-ABI takes (exact in float64; 1 - beta is exact in fp32 for beta in [1/2, 1));
    step_size and bc2s are rounded to fp32 once each."""
    lr, b1, b2, eps = (float(np.float32(c)) for c in (lr, b1, b2, eps))
    step_size, bc2s = lr / (1.0 - b1 ** step), np.sqrt(1.0 - b2 ** step)
    m1 = b1 * m + (1.0 - b1) * g
    e_m = (1.0 - b1) * e_g + 2.0 * U * (np.abs(b1 * m) + np.abs((1.0 - b1) * g))
    v1 = b2 * v + (1.0 - b2) * g * g
    e_v = 2.0 * (1.0 - b2) * np.abs(g) * e_g + 4.0 * U * (b2 * v + (1.0 - b2) * g * g)
    sq = np.sqrt(v1)
    e_sq = (np.sqrt(v1 + e_v) - np.sqrt(np.maximum(v1 - e_v, 0.0))) + U * sq        # |sqrt(a) - sqrt(b)| for every a, b within e_v of v1
    den = sq / bc2s + eps
    e_den = e_sq / bc2s + 2.0 * U * sq / bc2s + U * den
    q = m1 / den
    e_q = e_m / den + np.abs(m1) * e_den / den ** 2 + U * np.abs(q)
    # the gradient's own bound e_g moves m and the denominator TOGETHER (at step 1 the update is lr sign(g) whatever |g| is): where v1 is
    # safely positive it goes through the signed derivative dq/dg instead of through m and the denominator separately
    e_m0 = 2.0 * U * (np.abs(b1 * m) + np.abs((1.0 - b1) * g))
    e_v0 = 4.0 * U * (b2 * v + (1.0 - b2) * g * g)
    safe = v1 > 4.0 * e_v
    sqs = np.where(safe, sq, 1.0)
    e_den0 = (e_v0 / (2.0 * sqs) + U * sq) / bc2s + 2.0 * U * sq / bc2s + U * den
    dq = (1.0 - b1) / den - m1 * ((1.0 - b2) * g / (sqs * bc2s)) / den ** 2
    e_q = np.where(safe, np.abs(dq) * e_g + e_m0 / den + np.abs(m1) * e_den0 / den ** 2 + U * np.abs(q), e_q)
    upd = step_size * q
    e_upd = step_size * e_q + 2.0 * U * np.abs(upd)
    p1 = p - upd
    return (p1, e_upd + U * np.abs(p1)), (m1, e_m), (v1, e_v)
