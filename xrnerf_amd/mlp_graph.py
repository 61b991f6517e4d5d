"""The whole-MLP graph of the dense NeRFs on the device -- a relu trunk, then the reference's view head (nerf_mlp.py:62-94,
bungeenerf_mlp.py) -- as plain functions over the strided linear kernels (ops.linear_forward / linear_backward_input /
linear_backward_weight_bias).  vanilla._NerfMlpFn and bungee._BungeeMlpFn are autograd nodes that lay out their parameters and call these.

Same products, same order of the concatenated inputs as the per-layer graph; what is gone is the glue around them (19 % of the Mip-NeRF
step's GPU time in round 5: cat / split / pad copies, masked copies, two reductions per layer, per-layer autograd nodes).  Every activation
lives in a buffer laid out for its consumer, and every layer's weight and bias gradient come from one launch and one reduction over the M
ranges (ops.linear_backward_weight_bias)."""
import torch

from . import ops


def ceil4(n):
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------ weights of a layer that reads the embedding in place
def pad_weight_cols(w, ic):
    """`w` [N, ic + rest] takes [x_pts | rest] with x_pts the embedding's first ic columns.  input_ch is not a multiple of 4 (63 in the
    configs) and the kernels read whole float4s, so the layer reads Kx = ceil4(ic) columns of the embedding in place and its weight gets
    zero columns at [ic, Kx).  Exact: those columns of the input hold finite values (the first direction features, or the encoder's zero
    padding) and w * x = 0."""
    Kx = ceil4(ic)
    if Kx == ic:
        return w
    wp = w.new_zeros((w.shape[0], w.shape[1] + Kx - ic))
    wp[:, :ic] = w[:, :ic]
    wp[:, Kx:] = w[:, ic:]
    return wp


def unpad_grad_cols(dw, ic):
    """the gradient of pad_weight_cols' result without its zero columns: the gradient of `w`"""
    Kx = ceil4(ic)
    return dw if Kx == ic else torch.cat([dw[:, :ic], dw[:, Kx:]], 1)


# ------------------------------------------------------------------ trunk
def trunk_forward(h, layers, ic, out=None):
    """relu(linear) through `layers` = [(weight, bias), ...] starting from `h`, whose first ceil4(ic) columns are x_pts read in place (the
    first weight is padded for it) -> (the state trunk_backward needs, the last output).
    out: where the last layer writes, a column range of the NEXT consumer's [x_pts | h] buffer (an output row stride) -- a skip connection's
    concatenation is a buffer that x_pts was copied into once and that the layer in front of it writes its output INTO."""
    ws = [pad_weight_cols(layers[0][0], ic)] + [w for w, _ in layers[1:]]
    acts = []
    for i, w in enumerate(ws):
        y = ops.linear_forward(h, w, layers[i][1], True, out=out if i == len(ws) - 1 else None)
        acts.append((h, y))
        h = y
    return (acts, ws), h


def trunk_backward(dy, state, ic, first=False):
    """dy: the gradient of the last output; where that output is a column range of a [x_pts | h] buffer, dy is the same column range of
    the consumer's input gradient (the row stride goes to dy and to the relu mask alike).
    -> ([dW, db, dW, db, ...] in the layers' order, the gradient of the input -- None with `first`: the network's first layer reads the
    embedding, which has no gradient here)"""
    acts, ws = state
    grads = []
    for i in range(len(acts) - 1, -1, -1):
        xin, y = acts[i]
        dw, db = ops.linear_backward_weight_bias(dy, y, xin)
        grads[:0] = [unpad_grad_cols(dw, ic) if i == 0 else dw, db]
        if i > 0 or not first:
            dy = ops.linear_backward_input(dy, y, ws[i])
    return grads, (None if first else dy)


# ------------------------------------------------------------------ view head
def _view_cols(W, idr):
    """the view layer's input buffer V = [feature (W) | alpha 0 0 0 | dir (idr) | 0 ..]: (the directions' first column, V's width)"""
    o_dir = W + 4
    return o_dir, o_dir + ceil4(idr)


def view_head_forward(h, x_dir, head, dst):
    """h [M, W] -> dst [M, 4] = [rgb | alpha]; head = (views w, b, feature w, b, alpha w, b, rgb w, b); dst dense or one head's rows of
    raw [M, H, 4] (row stride 4 H).  Nothing is concatenated:
      * feature and alpha heads are ONE product (rows of one weight, padded to W + 4 rows) whose output lands in the view layer's input
        buffer V; the directions are copied in behind it;
      * the view layer's weight has zero columns under alpha and the padding (exact: the products are w * 0);
      * the rgb head has a fourth, zero output row, so its product writes whole float4 rows of dst; alpha is then copied into column 3.
    -> the state view_head_backward needs"""
    vw, vb, fw, fb, aw, ab, rw, rb = head
    W, W2, idr = fw.shape[0], vw.shape[0], x_dir.shape[1]
    o_dir, KV = _view_cols(W, idr)
    V = torch.empty((h.shape[0], KV), dtype=torch.float32, device=h.device)
    wb = torch.cat([fw, aw, fw.new_zeros((3, W))], 0)
    bb = torch.cat([fb, ab, fb.new_zeros((3,))], 0)
    ops.linear_forward(h, wb, bb, False, out=V[:, :o_dir])
    V[:, o_dir:o_dir + idr].copy_(x_dir)
    if KV > o_dir + idr:
        V[:, o_dir + idr:].zero_()
    wv2 = vw.new_zeros((W2, KV))
    wv2[:, :W] = vw[:, :W]
    wv2[:, o_dir:o_dir + idr] = vw[:, W:]
    hv = ops.linear_forward(V, wv2, vb, True)
    wr2 = torch.cat([rw, rw.new_zeros((1, W2))], 0)
    br2 = torch.cat([rb, rb.new_zeros((1,))], 0)
    ops.linear_forward(hv, wr2, br2, False, out=dst)
    dst[:, 3].copy_(V[:, W])
    return V, hv, wb, wv2, wr2, idr


def view_head_backward(d_raw_k, state, h):
    """d_raw_k [M, 4]: the gradient of view_head_forward's dst; h: the head's input
    -> (the eight parameter gradients in `head`'s order, dh)"""
    V, hv, wb, wv2, wr2, idr = state
    W = wb.shape[1]
    o_dir, _ = _view_cols(W, idr)
    dwr2, dbr2 = ops.linear_backward_weight_bias(d_raw_k, None, hv)
    dhv = ops.linear_backward_input(d_raw_k, None, wr2)
    dwv2, dbv = ops.linear_backward_weight_bias(dhv, hv, V)
    dV = ops.linear_backward_input(dhv, hv, wv2)
    dV[:, W].copy_(d_raw_k[:, 3])                          # alpha's gradient joins the feature gradient: one product for both heads
    dyb = dV[:, :o_dir]
    dwb, dbb = ops.linear_backward_weight_bias(dyb, None, h)
    dh = ops.linear_backward_input(dyb, None, wb)
    dvw = torch.cat([dwv2[:, :W], dwv2[:, o_dir:o_dir + idr]], 1)             # without the zero columns
    return [dvw, dbv, dwb[:W], dbb[:W], dwb[W:W + 1], dbb[W:W + 1], dwr2[:3], dbr2[:3]], dh
