"""Registry entries of the NeuralBody path (configs/neuralbody/nb_zjumocap_*.py): `NeuralBodyNetwork`, `SmplEmbedder` (with its
`SparseConvNet`) and `NB_NeRFMLP`.

The reference's only outside dependency here is `spconv` (SubMConv3d, SparseConv3d, SparseSequential, SparseConvTensor.dense()), which
has no ROCm build.  On the device a step is
  voxel coordinates of the SMPL vertices (the reference's torch lines) -> the frame's structure, built ONCE and shared by all 17
  convolutions (xr_nb_build_rows, xr_nb_subm_table, xr_nb_down_tables) -> the sparse network on [N, C] rows (xr_nb_conv per
  convolution, BatchNorm1d and ReLU as torch ops on the rows) -> trilinear sampling of the four levels' ROWS through their index
  volumes (xr_nb_sample_forward: no dense [1, C, D, H, W] volume is ever made) -> NB_NeRFMLP on the linear kernels -> NerfRender
with the backward through xr_nb_sample_backward, xr_nb_conv (input gradient) and xr_nb_conv_weight_grad (xrnerf_amd/csrc/
xr_neuralbody.hip).  Host tensors, a library handle without those entry points, or `tensor_op_path(True)` keep
the same step as tensor ops: the rulebook from torch.unique / searchsorted, a convolution as index_select + matmul per tap, gather-based
sampling.  That path is what the CPU tests run and the timing baseline of tools/microbench_neuralbody.py.

Semantics that spconv would decide are fixed in DESIGN.md section 13 ("unpinned against spconv"): rows in ascending linear index,
vertices of one voxel merged by summing their latent codes, cross-correlation taps k = (kz 3 + ky) 3 + kx, the strided output active
where any of its 27 inputs is.  State-dict keys are the reference's (`smpl_conv.xyzc_net.conv0.0.weight`, ...); convolution weights are
spconv 2.x's [Cout, 3, 3, 3, Cin], and 1.x's [3, 3, 3, Cin, Cout] is accepted on load.

`val_step` / `render_frame` build the structure and run the sparse network once per frame and reuse its four levels for every chunk
(the reference recomputes them per chunk with identical batch statistics; its running statistics then move once per chunk, here once
per frame: the one intended deviation).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import builder
from .aninerf import _EmbedFn, _RAY_KEYS, nb_recover_shape, synthetic_body, to_pose
from .builder import EMBEDDERS, MLPS, NETWORKS
from .networks import BaseNerfNetwork, get_dist_info, img2mse, mse2psnr, unfold_batching

LEVELS = 5
TAPS = 27
LEVEL_CHANNELS = (32, 64, 128, 128)         # the sampled levels (after conv1 .. conv4)
N_VERTS = 6890                              # nn.Embedding(6890, 16) is hard-wired in the reference
_TENSOR_OPS = False
CALLS = {'structure': 0, 'sparse_net': 0}   # how often the frame structure was built / the sparse network ran (tests, microbench)


def tensor_op_path(on):
    """True: every stage runs as tensor ops even on the device (the timing baseline).  Returns the previous setting."""
    global _TENSOR_OPS
    old, _TENSOR_OPS = _TENSOR_OPS, bool(on)
    return old


def _kernels(t):
    from . import ops
    return (not _TENSOR_OPS) and ops._on_device(t) and t.dtype == torch.float32 and ops.neuralbody_kernels_available()


def level_dims(out_sh, l):
    return tuple(int(v) >> l for v in out_sh)


# ------------------------------------------------------------------ the frame's structure
class Frame:
    """what `indice_key` is for in the reference: per level the rows (active cells, ascending linear index), the submanifold table
    [n, 27], per strided step the output- and input-stationary tables; on the kernel path also the int32 index volumes"""
    __slots__ = ('out_sh', 'n', 'rows', 'vols', 'vert_row', 'merge', 'subm', 'down_out', 'down_in', 'kernels')


def _decode(lin, dims):
    D, H, W = dims
    return lin // (H * W), (lin // W) % H, lin % W


def _lookup(rows, lin, valid):
    """row of every linear index in the sorted list `rows`, -1 where absent or not valid"""
    n = rows.shape[0]
    if n == 0:
        return torch.full_like(lin, -1)
    i = torch.searchsorted(rows, lin.clamp(min=0)).clamp(max=n - 1)
    return torch.where(valid & (rows[i] == lin), i, torch.full_like(i, -1))


def _taps(device):
    k = torch.arange(TAPS, device=device)
    return k // 9, (k // 3) % 3, k % 3


def _subm_table(rows, dims):
    D, H, W = dims
    z, y, x = _decode(rows, dims)
    kz, ky, kx = _taps(rows.device)
    nz, ny, nx = z[:, None] + kz - 1, y[:, None] + ky - 1, x[:, None] + kx - 1
    valid = (nz >= 0) & (nz < D) & (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
    return _lookup(rows, (nz * H + ny) * W + nx, valid)


def _down(rows_in, dims):
    """the strided step from a level with `dims`: (rows_out, out_tab [n_out, 27], in_tab [n_in, 27])"""
    D, H, W = dims
    Do, Ho, Wo = D // 2, H // 2, W // 2
    z, y, x = _decode(rows_in, dims)
    kz, ky, kx = _taps(rows_in.device)
    tz, ty, tx = z[:, None] + 1 - kz, y[:, None] + 1 - ky, x[:, None] + 1 - kx
    valid = (tz >= 0) & (tz % 2 == 0) & (tz // 2 < Do) & (ty >= 0) & (ty % 2 == 0) & (ty // 2 < Ho) & \
            (tx >= 0) & (tx % 2 == 0) & (tx // 2 < Wo)
    lin_o = ((tz // 2) * Ho + ty // 2) * Wo + tx // 2
    rows_out = torch.unique(lin_o[valid], sorted=True)
    in_tab = _lookup(rows_out, lin_o, valid)
    zo, yo, xo = _decode(rows_out, (Do, Ho, Wo))
    iz, iy, ix = 2 * zo[:, None] - 1 + kz, 2 * yo[:, None] - 1 + ky, 2 * xo[:, None] - 1 + kx
    v = (iz >= 0) & (iz < D) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    return rows_out, _lookup(rows_in, (iz * H + iy) * W + ix, v), in_tab


def _merge_table(vert_row, n0):
    """[n0, maxdup] vertex ids of every level-0 row in ascending order, padded with V: the fixed order in which the latent codes of
    the vertices of one voxel are summed (one count read from the device)"""
    V = vert_row.shape[0]
    vr = vert_row.long()
    vr = torch.where(vr < 0, torch.full_like(vr, n0), vr)
    sorted_rows, order = torch.sort(vr, stable=True)
    start = torch.searchsorted(sorted_rows, torch.arange(n0 + 1, device=vr.device))
    rank = torch.arange(V, device=vr.device) - start[sorted_rows]
    keep = sorted_rows < n0
    maxdup = int(rank[keep].max().item()) + 1 if n0 else 1
    table = torch.full((n0, maxdup), V, dtype=torch.int64, device=vr.device)
    table[sorted_rows[keep], rank[keep]] = order[keep]
    return table


def build_frame(coord, out_sh):
    """coord [V, 3] int32 (z, y, x), out_sh (D, H, W) -> Frame"""
    from . import ops
    out_sh = tuple(int(v) for v in out_sh)
    if any(v <= 0 or v % 32 for v in out_sh) or out_sh[0] * out_sh[1] * out_sh[2] > ops.NB_MAX_CELLS:
        raise ValueError('out_sh %r: every axis must be a positive multiple of 32, at most %d cells' % (out_sh, ops.NB_MAX_CELLS))
    CALLS['structure'] += 1
    f = Frame()
    f.out_sh = out_sh
    f.kernels = coord.dtype == torch.int32 and (not _TENSOR_OPS) and ops._on_device(coord) and ops.neuralbody_kernels_available()
    if f.kernels:
        f.vols, f.rows, f.vert_row, f.n = ops.nb_build_rows(coord.contiguous(), out_sh)
        f.subm = [ops.nb_subm_table(f.vols[l], f.rows[l], level_dims(out_sh, l)) for l in range(LEVELS)]
        f.down_out, f.down_in = [], []
        for l in range(LEVELS - 1):
            o, i = ops.nb_down_tables(f.vols[l], f.rows[l], f.vols[l + 1], f.rows[l + 1], level_dims(out_sh, l))
            f.down_out.append(o)
            f.down_in.append(i)
    else:
        D, H, W = out_sh
        c = coord.long()
        inside = (c[:, 0] >= 0) & (c[:, 0] < D) & (c[:, 1] >= 0) & (c[:, 1] < H) & (c[:, 2] >= 0) & (c[:, 2] < W)
        lin = (c[:, 0] * H + c[:, 1]) * W + c[:, 2]
        rows0 = torch.unique(lin[inside], sorted=True)
        f.vert_row = _lookup(rows0, lin, inside)
        f.vols = None
        f.rows, f.subm, f.down_out, f.down_in = [rows0], [], [], []
        for l in range(LEVELS - 1):
            r, o, i = _down(f.rows[l], level_dims(out_sh, l))
            f.rows.append(r)
            f.down_out.append(o)
            f.down_in.append(i)
        f.subm = [_subm_table(f.rows[l], level_dims(out_sh, l)) for l in range(LEVELS)]
        f.n = [int(r.shape[0]) for r in f.rows]
    f.merge = _merge_table(f.vert_row, f.n[0])
    return f


class _MergeFn(torch.autograd.Function):
    """level 0's input rows: the sum of the latent codes of every row's vertices, in ascending vertex order; the gradient of a row
    goes to each of its vertices (a gather: no atomics in either direction)"""

    @staticmethod
    def forward(ctx, code, table, vert_row):
        cp = torch.cat([code, code.new_zeros((1, code.shape[1]))], 0)
        x = cp[table[:, 0]]
        for d in range(1, table.shape[1]):
            x = x + cp[table[:, d]]
        ctx.save_for_backward(vert_row)
        return x

    @staticmethod
    def backward(ctx, g):
        vert_row, = ctx.saved_tensors
        vr = vert_row.long()
        out = g[vr.clamp(min=0)]
        return torch.where((vr >= 0)[:, None], out, torch.zeros_like(out)), None, None


# ------------------------------------------------------------------ sparse convolution
class _ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, tab, back_tab, flip):
        from . import ops
        x, w = x.detach().contiguous(), w.detach().contiguous()
        out = ops.nb_conv(x, tab, w)
        ctx.save_for_backward(x, w, tab, back_tab)
        ctx.flip = flip
        return out

    @staticmethod
    def backward(ctx, g):
        from . import ops
        x, w, tab, back_tab = ctx.saved_tensors
        g = g.contiguous()
        dx = ops.nb_conv(g, back_tab, w, transposed=True, flip=ctx.flip) if ctx.needs_input_grad[0] else None
        dw = ops.nb_conv_weight_grad(x, tab, g) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None, None


def _conv_tensor_ops(x, w, tab):
    """out[r] = sum_k x[tab[r, k]] W[k]^T as index_select + matmul per tap (rows of tab = -1 read a zero row)"""
    n_in = x.shape[0]
    xp = torch.cat([x, x.new_zeros((1, x.shape[1]))], 0)
    idx = torch.where(tab < 0, torch.full_like(tab, n_in), tab).long()
    wk = w.reshape(w.shape[0], TAPS, w.shape[4])
    out = x.new_zeros((tab.shape[0], w.shape[0]))
    for k in range(TAPS):
        out = out + xp.index_select(0, idx[:, k]) @ wk[:, k, :].t()
    return out


def sparse_conv(x, w, frame, level, strided):
    """the submanifold convolution on `level`, or the strided one from `level` to `level + 1`; x [n_level, Cin], w [Cout,3,3,3,Cin]"""
    tab = frame.down_out[level] if strided else frame.subm[level]
    if frame.kernels and _kernels(x):
        if tab.shape[0] == 0:
            return x.new_zeros((0, w.shape[0])) + 0 * w.sum()
        return _ConvFn.apply(x, w, tab, frame.down_in[level] if strided else tab, not strided)
    return _conv_tensor_ops(x, w, tab)


class SparseConv3d(nn.Module):
    """SubMConv3d(k=3) / SparseConv3d(k=3, s=2, p=1) without bias: only the parameter; `SparseConvNet` applies it on a Frame"""

    def __init__(self, cin, cout, strided):
        super().__init__()
        self.cin, self.cout, self.strided = cin, cout, strided
        self.weight = nn.Parameter(torch.empty(cout, 3, 3, 3, cin))
        nn.init.kaiming_uniform_(self.weight.data.view(cout, -1), a=math.sqrt(5))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = prefix + 'weight'
        w = state_dict.get(k)
        # spconv 1.x stores [3, 3, 3, Cin, Cout]; a channel count is never 3, so the first axis tells the layouts apart
        if w is not None and w.dim() == 5 and w.shape[0] == 3 and tuple(w.shape) == (3, 3, 3, self.cin, self.cout):
            state_dict[k] = w.permute(4, 0, 1, 2, 3).contiguous()
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def extra_repr(self):
        return '%d, %d, %s' % (self.cin, self.cout, 'stride 2' if self.strided else 'submanifold')


def _block(cin, cout, n, strided=False):
    mods = []
    for i in range(n):
        mods += [SparseConv3d(cin if i == 0 else cout, cout, strided), nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01), nn.ReLU()]
    return nn.Sequential(*mods)


class SparseConvNet(nn.Module):
    """neuralbody_embedder.py:59-98 with its sub-module names (conv0.0, conv0.1, ..., down3.0, conv4.7)"""

    def __init__(self):
        super().__init__()
        self.conv0 = _block(16, 16, 2)
        self.down0 = _block(16, 32, 1, True)
        self.conv1 = _block(32, 32, 2)
        self.down1 = _block(32, 64, 1, True)
        self.conv2 = _block(64, 64, 3)
        self.down2 = _block(64, 128, 1, True)
        self.conv3 = _block(128, 128, 3)
        self.down3 = _block(128, 128, 1, True)
        self.conv4 = _block(128, 128, 3)

    @staticmethod
    def _run(block, x, frame, level):
        for m in block:
            x = sparse_conv(x, m.weight, frame, level, m.strided) if isinstance(m, SparseConv3d) else m(x)
        return x

    def forward(self, x, frame):
        """x [n_0, 16] -> the rows of levels 1..4 after conv1..conv4: [n_1, 32], [n_2, 64], [n_3, 128], [n_4, 128]"""
        CALLS['sparse_net'] += 1
        out = []
        net = self._run(self.conv0, x, frame, 0)
        for l, (down, conv) in enumerate(((self.down0, self.conv1), (self.down1, self.conv2), (self.down2, self.conv3),
                                          (self.down3, self.conv4))):
            net = self._run(down, net, frame, l)
            net = self._run(conv, net, frame, l + 1)
            out.append(net)
        return out


# ------------------------------------------------------------------ feature sampling
def grid_coords(pts, R, T, min_xyz, voxel, out_sh):
    """prepare_sparseconv_data's pts_idx: ((p - T) R - min_xyz) / voxel / out_sh[[2, 1, 0]] * 2 - 1 with the pose product in the
    kernel's order (k ascending, un-fused) -> [N, 3] (x, y, z)"""
    q = to_pose(pts.reshape(-1, 3), R, T.reshape(3))
    sh = torch.tensor([out_sh[2], out_sh[1], out_sh[0]], dtype=pts.dtype, device=pts.device)
    return (q - min_xyz) / voxel / sh * 2 - 1


def _sample_tensor_ops(feats, frame, c):
    """F.grid_sample(dense volume, c, padding_mode='zeros', align_corners=True) of the four levels, gathered from the rows"""
    out = []
    for l in range(1, LEVELS):
        D, H, W = level_dims(frame.out_sh, l)
        rows, feat = frame.rows[l].long(), feats[l - 1]
        fp = torch.cat([feat, feat.new_zeros((1, feat.shape[1]))], 0)
        f = [((c[:, j] + 1) / 2) * (s - 1) for j, s in enumerate((W, H, D))]
        lo = [torch.floor(v) for v in f]
        acc = feat.new_zeros((c.shape[0], feat.shape[1]))
        for corner in range(8):
            b = (corner & 1, (corner >> 1) & 1, corner >> 2)
            cc = [lo[j] + b[j] for j in range(3)]
            w3 = [(f[j] - lo[j]) if b[j] else ((lo[j] + 1) - f[j]) for j in range(3)]
            w = (w3[0] * w3[1]) * w3[2]
            inside = (cc[0] >= 0) & (cc[0] <= W - 1) & (cc[1] >= 0) & (cc[1] <= H - 1) & (cc[2] >= 0) & (cc[2] <= D - 1)
            ci = [torch.where(inside, v, torch.zeros_like(v)).long() for v in cc]
            row = _lookup(rows, (ci[2] * H + ci[1]) * W + ci[0], inside)
            row = torch.where(row < 0, torch.full_like(row, feat.shape[0]), row)
            acc = acc + fp.index_select(0, row) * w[:, None]
        out.append(acc)
    return torch.cat(out, 1)


class _SampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f1, f2, f3, f4, frame, pts, R, T, min_xyz, voxel):
        from . import ops
        feats = [t.detach().contiguous() for t in (f1, f2, f3, f4)]
        out = ops.nb_sample_forward(pts, R, T, min_xyz, voxel, frame.out_sh, frame.vols[1:], feats)
        ctx.frame, ctx.voxel = frame, voxel
        ctx.save_for_backward(pts, R, T, min_xyz)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import ops
        pts, R, T, min_xyz = ctx.saved_tensors
        fr = ctx.frame
        gs = ops.nb_sample_backward(pts, R, T, min_xyz, ctx.voxel, fr.out_sh, fr.vols[1:], fr.n[1:], g)
        return gs[0], gs[1], gs[2], gs[3], None, None, None, None, None, None


def sample_features(feats, frame, pts, R, T, min_xyz, voxel):
    """the four levels' rows sampled at the world points pts [N, 3] -> [N, 352]; the points get no gradient"""
    pts = pts.detach().reshape(-1, 3)
    if frame.kernels and _kernels(pts):
        return _SampleFn.apply(feats[0], feats[1], feats[2], feats[3], frame, pts.contiguous(), R.contiguous(), T.reshape(3).contiguous(),
                               min_xyz.contiguous(), float(voxel))
    return _sample_tensor_ops(feats, frame, grid_coords(pts, R, T, min_xyz, voxel, frame.out_sh))


# ------------------------------------------------------------------ embedder
class FrameLevels:
    """a frame's structure with the sparse network's four levels: what every chunk of a frame shares"""
    __slots__ = ('frame', 'feats', 'min_xyz')


@EMBEDDERS.register_module()
class SmplEmbedder(nn.Module):
    def __init__(self, **kwargs):
        super().__init__()
        vs = kwargs['voxel_size']
        vs = [float(v) for v in vs] if isinstance(vs, (list, tuple)) else [float(vs)] * 3
        if not (vs[0] == vs[1] == vs[2]):
            raise NotImplementedError('SmplEmbedder: the three voxel sizes must be equal (every NeuralBody config uses one)')
        self.voxel_size = vs
        self.latent_codes = nn.Embedding(N_VERTS, 16)
        self.xyzc_net = SparseConvNet()

    def prepare(self, datas):
        """prepare_sparseconv_data's lines for the vertices: -> (coord [V, 3] int32 (z, y, x), out_sh [D, H, W], min_xyz [3]).
        out_sh is read from the device, as the reference's `.tolist()` does."""
        R, T = datas['smpl_R'], datas['smpl_T'].reshape(3)
        canonical = to_pose(datas['smpl_verts'].reshape(-1, 3), R, T)
        min_xyz = canonical.min(0)[0].clone()
        min_xyz[2] = min_xyz[2] - 0.05
        max_xyz = canonical.max(0)[0].clone()
        max_xyz[2] = max_xyz[2] + 0.05
        voxel = torch.tensor(self.voxel_size).to(canonical)
        coord = torch.round((canonical - min_xyz) / voxel).int()[..., [2, 1, 0]].contiguous()
        out_sh = torch.ceil((max_xyz - min_xyz) / voxel)[[2, 1, 0]].int()
        out_sh = ((out_sh | 31) + 1).tolist()
        return coord, out_sh, min_xyz

    def encode_frame(self, datas):
        """the structure of the frame's vertices and the sparse network on their latent codes -> FrameLevels"""
        coord, out_sh, min_xyz = self.prepare(datas)
        fl = FrameLevels()
        fl.frame = build_frame(coord, out_sh)
        fl.min_xyz = min_xyz
        code = self.latent_codes(torch.arange(0, coord.shape[0], device=coord.device))
        x = _MergeFn.apply(code, fl.frame.merge, fl.frame.vert_row)
        fl.feats = self.xyzc_net(x, fl.frame)
        return fl

    def sample_frame(self, fl, datas):
        return sample_features(fl.feats, fl.frame, datas['pts'], datas['smpl_R'], datas['smpl_T'], fl.min_xyz, self.voxel_size[0])

    def forward(self, datas, levels=None, reference_layout=False):
        """-> xyzc_features [N, 352] (row-major), or the reference's [1, 352, N] with reference_layout"""
        fl = self.encode_frame(datas) if levels is None else levels
        out = self.sample_frame(fl, datas)
        return out.t()[None] if reference_layout else out


# ------------------------------------------------------------------ MLP
def _embed(p, L):
    """BaseEmbedder's encoding of [N, 3] values that carry no gradient -> [N, 3 + 6 L]"""
    from . import ops
    p = p.detach()
    k = 3 + 6 * L
    if _kernels(p) and p.shape[0] > 0 and ops.vanilla_kernels_available():
        return _EmbedFn.apply(p, int(L))[:, :k]
    parts = [p]
    for i in range(L):
        parts += [torch.sin(p * float(2.0 ** i)), torch.cos(p * float(2.0 ** i))]
    return torch.cat(parts, -1)


def _lin(x, w, b, relu=False):
    if _TENSOR_OPS:
        y = F.linear(x, w, b)
        return F.relu(y) if relu else y
    # exact fp32 products (the fp32-MFMA kernel, forward and backward): this family's bars are 4 x the reference's own float32 error,
    # which the default split arithmetic of the linear kernels (2^-16 per gradient product) does not meet
    from .linear import linear_act_padded
    return linear_act_padded(x, w, b, relu, exact=True)


@MLPS.register_module()
class NB_NeRFMLP(nn.Module):
    def __init__(self, num_frame, embedder):
        super().__init__()
        self.appearance_code = nn.Embedding(num_frame, 128)
        self.actvn = nn.ReLU()
        self.fc_0 = nn.Conv1d(352, 256, 1)
        self.fc_1 = nn.Conv1d(256, 256, 1)
        self.fc_2 = nn.Conv1d(256, 256, 1)
        self.alpha_fc = nn.Conv1d(256, 1, 1)
        self.feature_fc = nn.Conv1d(256, 256, 1)
        self.latent_fc = nn.Conv1d(384, 256, 1)
        self.view_fc = nn.Conv1d(346, 128, 1)
        self.rgb_fc = nn.Conv1d(128, 3, 1)
        self.embedder = builder.build_embedder(embedder)
        self.multires, self.multires_dirs = int(embedder['multires']), int(embedder['multires_dirs'])
        assert 256 + 3 * (1 + 2 * self.multires) + 3 * (1 + 2 * self.multires_dirs) == 346, 'NB_NeRFMLP is hard-wired to 346 view channels'

    def forward(self, xyzc_features, datas):
        """xyzc_features [N, 352] (or the reference's [1, 352, N]); a 1x1 Conv1d is a linear layer, the appearance code's product in
        latent_fc a per-call bias, and rays_d is encoded once per ray"""
        x = xyzc_features[0].t() if xyzc_features.dim() == 3 else xyzc_features
        n_ray, n_s = datas['pts'].shape[:2]
        w = lambda m: m.weight[:, :, 0]
        net = _lin(x, w(self.fc_0), self.fc_0.bias, True)
        net = _lin(net, w(self.fc_1), self.fc_1.bias, True)
        net = _lin(net, w(self.fc_2), self.fc_2.bias, True)
        alpha = _lin(net, w(self.alpha_fc), self.alpha_fc.bias)
        feat = _lin(net, w(self.feature_fc), self.feature_fc.bias)
        latent = self.appearance_code(datas['latent_idx'].reshape(-1)[:1].long())[0]
        wl = w(self.latent_fc)
        feat = _lin(feat, wl[:, :256], self.latent_fc.bias + wl[:, 256:] @ latent)
        vd = _embed(datas['rays_d'].reshape(-1, 3), self.multires_dirs)
        vd = vd[:, None, :].expand(n_ray, n_s, vd.shape[1]).reshape(n_ray * n_s, -1)
        lp = _embed(datas['pts'].reshape(-1, 3), self.multires)
        net = _lin(torch.cat([feat, vd, lp], 1), w(self.view_fc), self.view_fc.bias, True)
        rgb = _lin(net, w(self.rgb_fc), self.rgb_fc.bias)
        datas['raw'] = torch.cat([rgb, alpha], 1).view(n_ray, n_s, 4)
        return datas


# ------------------------------------------------------------------ network
@NETWORKS.register_module()
class NeuralBodyNetwork(BaseNerfNetwork):
    def __init__(self, cfg, embedder=None, render=None):
        super().__init__()
        self.cfg = cfg = builder.ConfigDict.wrap(dict(cfg))
        self.chunk = cfg.chunk
        self.bs_data = cfg.bs_data
        self.phase = cfg.get('phase', 'train')
        self.idx = 0
        self.smpl_conv = builder.build_embedder(cfg.smpl_embedder)
        self.nerf_mlp = builder.build_mlp(cfg.nerf_mlp)
        self.render = builder.build_render(render)

    def forward(self, datas, is_test=False, levels=None):
        self.train()                                   # the batch norms stay in training mode (networks/neuralbody.py:31)
        xyzc_features = self.smpl_conv(datas, levels=levels)
        datas = self.nerf_mlp(xyzc_features, datas)
        datas, ret = self.render(datas, is_test)
        ret['xyzc_features'] = xyzc_features
        ret['raw'] = datas['raw']
        return ret

    def train_step(self, datas, optimizer, **kwargs):
        for k in datas:
            datas[k] = unfold_batching(datas[k])
        ret = self.forward(datas, is_test=False)
        loss = img2mse(ret['rgb'], datas['target_s'])
        return {'loss': loss, 'log_vars': {'loss': loss.item(), 'psnr': mse2psnr(loss.detach()).item()}, 'num_samples': ret['rgb'].shape[0],
                'ret': ret}

    def render_frame(self, datas):
        """every ray of a frame in chunks of `self.chunk`; the structure and the sparse network run ONCE, their four levels serve
        every chunk (the batch statistics of a frame do not depend on the chunk)"""
        self.train()
        N = datas[self.bs_data].shape[0]
        all_ret = {}
        with torch.no_grad():
            levels = self.smpl_conv.encode_frame(datas)
            for i in range(0, N, self.chunk):
                chunk = {k: (v[i:i + self.chunk] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == N and k in _RAY_KEYS else v)
                         for k, v in datas.items()}
                ret = self.forward(chunk, True, levels=levels)
                for k in ('rgb', 'disp', 'acc'):
                    all_ret.setdefault(k, []).append(ret[k])
        return {k: torch.cat(v, 0) for k, v in all_ret.items()}

    def val_step(self, datas, *args, **kwargs):
        rank, _ = get_dist_info()
        if rank != 0:
            return {}
        for k in datas:
            datas[k] = unfold_batching(datas[k])
        ret = self.render_frame(datas)
        rgb = nb_recover_shape(ret['rgb'], datas['src_shape'], datas['mask_at_box']).cpu().numpy()
        disp = nb_recover_shape(ret['disp'], datas['src_shape'], datas['mask_at_box']).cpu().numpy()
        outputs = {'rgbs': [rgb], 'disps': [disp], 'rgb': rgb, 'idx': self.idx}
        if self.phase != 'render':
            image = nb_recover_shape(datas['target_s'], datas['src_shape'], datas['mask_at_box']).cpu().numpy()
            outputs.update({'gt_imgs': [image], 'gt_img': image})
        self.idx += 1
        return outputs


def render_frame(net, datas):
    return net.render_frame(datas)


def train_step(net, datas, optimizer=None):
    """one optimisation step with the reference's img2mse loss: zero_grad, forward, backward, optimizer.step() -> train_step's dict"""
    if optimizer is not None:
        optimizer.zero_grad()
    out = net.train_step(datas, optimizer)
    out['loss'].backward()
    if optimizer is not None:
        optimizer.step()
    return out


def synthetic_frame(V=N_VERTS, seed=5, n_rays=32, n_samples=16, device=None, latent_idx=3):
    """aninerf.synthetic_body plus `latent_idx`: the `datas` of one NeuralBody frame, unbatched"""
    datas = synthetic_body(V, seed, n_rays, n_samples, device)
    datas['latent_idx'] = torch.tensor([latent_idx], dtype=torch.int64, device=device)
    return datas
