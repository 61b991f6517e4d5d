"""TEST INFRASTRUCTURE: float64 references for the training backward, computed live on the CPU.

mlp64            the NeRF MLP chain the fused kernels evaluate (xr_mlp.hip), from the encoded features on: density net (nhd hidden
                 layers of 64, 16 outputs), SH-4 of `dirs`, colour input [dout[1:16] | sh | pad_value], colour net (nhc hidden
                 layers), raw = [cout[:3] | dout[0]] -- in torch float64 with autograd, on the flat weight layout of
                 ops.nerf_mlp_fwd / _bwd.  Returns raw, dWd, dWc, dL/denc and the per-sample kink margin (min over the hidden units of
                 |z| / sum |w x|, the measure of oracle xo_nerf_mlp_kink_margin, here in float64).
table_grad64     the table gradient as float64 sums over the corner table of the oracle (xo_hashgrid_corners: the kernels' cell, weights
                 in double), with what the per-entry bars of tests/grad_bars.py need: the budget sum |w g| and the contribution count."""
import numpy as np
import torch

SH_C = (0.28209479177387814, 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.31539156525251999,
        0.54627421529603959, 0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 1.4453057213202769)


def _layers(w, n_hidden, n_in=32, width=64, n_out=16):
    """views [out, in] of a flat parameter vector (row-major matrices in layer order)"""
    dims = [n_in] + [width] * n_hidden + [n_out]
    out, o = [], 0
    for a, b in zip(dims[:-1], dims[1:]):
        out.append(w[o:o + a * b].view(b, a))
        o += a * b
    assert o == w.numel(), (o, w.numel())
    return out


def sh4_64(dirs):
    """SH degree 4 of d' = 2 dirs - 1, float64 (the oracle's xo_sh4 formulas)"""
    d = 2.0 * dirs - 1.0
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    c = SH_C
    return torch.stack([torch.full_like(x, c[0]), -c[1] * y, c[1] * z, -c[1] * x, c[2] * xy, -c[2] * yz, c[3] * z2 - c[4], -c[2] * xz,
                        c[5] * x2 - c[5] * y2, c[6] * y * (-3.0 * x2 + y2), c[7] * xy * z, c[8] * y * (1.0 - 5.0 * z2),
                        c[9] * z * (5.0 * z2 - 3.0), c[8] * x * (1.0 - 5.0 * z2), c[10] * z * (x2 - y2), c[6] * x * (-x2 + 3.0 * y2)], 1)


def _net(h, ws, margin):
    for w in ws[:-1]:
        z = h @ w.t()
        with torch.no_grad():
            mag = h.abs() @ w.abs().t()
            r = torch.where(mag > 0, z.abs() / torch.where(mag > 0, mag, torch.ones_like(mag)), torch.full_like(mag, np.inf))
            torch.minimum(margin, r.amin(1), out=margin)
        h = torch.relu(z)
    return h @ ws[-1].t()


def mlp64(enc, dirs, wd, wc, nhd, nhc, draw, pad_value=1.0, chunk=1 << 16):
    """enc [n, 32], dirs [n, 3], draw [n, 4] (numpy or torch, any float type), wd / wc flat -> dict of float64 numpy arrays:
    raw [n, 4], dwd, dwc, denc [n, 32], margin [n].  Rows are independent; the weight gradients are float64 sums over them.
    draw=None: the forward only (raw, margin)."""
    f64 = lambda a: torch.as_tensor(np.asarray(a.cpu() if torch.is_tensor(a) else a), dtype=torch.float64)
    enc, dirs = f64(enc), f64(dirs)
    fwd_only = draw is None
    draw = torch.zeros((enc.shape[0], 4), dtype=torch.float64) if fwd_only else f64(draw)
    wd, wc = f64(wd).requires_grad_(True), f64(wc).requires_grad_(True)
    n = enc.shape[0]
    raw = torch.zeros((n, 4), dtype=torch.float64)
    denc = torch.zeros((n, 32), dtype=torch.float64)
    margin = torch.full((n,), np.inf, dtype=torch.float64)
    gwd, gwc = torch.zeros_like(wd), torch.zeros_like(wc)
    for s in range(0, n, chunk):
        e = enc[s:s + chunk].clone().requires_grad_(True)
        m = margin[s:s + chunk]
        with torch.enable_grad():
            dout = _net(e, _layers(wd, nhd), m)
            cin = torch.cat([dout[:, 1:16], sh4_64(dirs[s:s + chunk]), torch.full((e.shape[0], 1), float(pad_value), dtype=torch.float64)], 1)
            cout = _net(cin, _layers(wc, nhc), m)
            r = torch.cat([cout[:, :3], dout[:, :1]], 1)
            raw[s:s + chunk] = r.detach()
            if fwd_only:
                continue
            ge, a, b = torch.autograd.grad(r, [e, wd, wc], grad_outputs=draw[s:s + chunk])
        denc[s:s + chunk] = ge
        gwd += a
        gwc += b
    if fwd_only:
        return dict(raw=raw.numpy(), margin=margin.numpy())
    return dict(raw=raw.numpy(), dwd=gwd.detach().numpy(), dwc=gwc.detach().numpy(), denc=denc.numpy(), margin=margin.numpy())


def table_grad64(O, x, g, meta, levels=None, init=None):
    """x [n, 3] fp32 positions, g [n, 32] the fp32 dL/d(encoding) handed to the scatter (rows that must not count are zero), levels
    (l0, l1) -> dict: ref float64 [n_params] (= init + the levels' float64 sums; other entries = init), budget float64 [n_params]
    (|init| + sum |w g| per entry), count int64 [n_params] (contributions per entry: corners of rows with a non-zero gradient)"""
    x = np.ascontiguousarray(x, np.float32)
    g = np.asarray(g, np.float32)
    l0, l1 = (0, meta.n_levels) if levels is None else levels
    P = meta.n_params
    ref = np.zeros(P) if init is None else np.asarray(init, np.float64).copy()
    budget = np.abs(ref)
    count = np.zeros(P, np.int64)
    for lv in range(l0, l1):
        a, b = 2 * int(meta.offset[lv]), 2 * int(meta.offset[lv + 1])
        idx, w = O.hashgrid_corners(x, meta, (lv, lv + 1))
        loc = (idx[:, 0, :] - int(meta.offset[lv])).ravel()
        w = w[:, 0, :]
        hs = (b - a) // 2
        live = ((g[:, 2 * lv] != 0) | (g[:, 2 * lv + 1] != 0))
        cnt = np.bincount(loc, weights=np.repeat(live, 8).astype(np.float64), minlength=hs).astype(np.int64)
        for f in range(2):
            c = (w * g[:, 2 * lv + f].astype(np.float64)[:, None]).ravel()
            ref[a + f:b:2] += np.bincount(loc, weights=c, minlength=hs)
            budget[a + f:b:2] += np.bincount(loc, weights=np.abs(c), minlength=hs)
            count[a + f:b:2] = cnt
    return dict(ref=ref, budget=budget, count=count)
