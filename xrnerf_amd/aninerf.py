"""Registry entries of the Animatable-NeRF path (configs/animatable_nerf/an_h36m_s9_train_pose.py): `AniNeRFNetwork`, `DeformField`,
`TPoseHuman`, `AN_BlendWeightMLP`, `AN_DensityMLP`, `AN_ColorMLP`, and `NovelPoseTraining` for the `novel_pose` phase.

On the device a step is
  world -> pose transform + nearest SMPL vertex (xr_ani_closest) -> "near the body" compaction (xr_ani_select, ONE count read) ->
  blend-weight MLP on the linear kernels -> softmax head (xr_ani_blend_forward) -> skinning pose -> T-pose -> canonical pose, points
  and directions in one launch (xr_ani_skin_forward) -> nearest canonical vertex -> blend-weight MLP again -> density and colour MLPs
  -> scatter back to [R, S, 4] -> NerfRender
with the backward through xr_ani_skin_backward, xr_ani_blend_backward and xr_ani_encode_backward (xrnerf_amd/csrc/xr_aninerf.hip;
DESIGN.md section 12).  Host tensors, a library handle without those entry points, or `tensor_op_path(True)` keep the same step as tensor
ops: the reference's composition, which is also the timing baseline of tools/microbench_aninerf.py.

Constructor signatures, `datas` keys and state-dict keys follow
  /root/reference/xrnerf/models/networks/aninerf.py, models/mlps/aninerf_mlp.py and models/networks/utils/aninerf.py:
`bw_linears.i.weight` is [out, in, 1] (Conv1d), `lin{l}.weight_g` / `weight_v` come from weight norm, the embeddings are `bw_latent`
and `color_latent`.  Inside, blend weights are [N, 24]; the reference's [1, 24, N] appears only in `deform_ret` / `calculate_neural_blend_weights`.
The 128-channel latent code is the same for every point of a call: its product is folded into the layer's bias.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import builder
from .builder import MLPS, NETWORKS
from .networks import BaseNerfNetwork, get_dist_info, img2mse, mse2psnr, unfold_batching

J = 24
_TENSOR_OPS = False
CLOSEST_CHUNK = 4096        # points per piece of the tensor-op nearest-vertex query: [4096, V, 3] differences = 339 MB at V = 6890


def tensor_op_path(on):
    """True: every stage runs as tensor ops even on the device (the timing baseline).  Returns the previous setting."""
    global _TENSOR_OPS
    old, _TENSOR_OPS = _TENSOR_OPS, bool(on)
    return old


def _kernels(t):
    from . import ops
    return (not _TENSOR_OPS) and ops._on_device(t) and t.dtype == torch.float32 and ops.aninerf_kernels_available()


# ------------------------------------------------------------------ stages: kernel or tensor ops
def to_pose(p, R, T):
    """world_points_to_pose_points in the kernel's operation order: q_j = sum_k (p_k - T_k) R_kj, k ascending"""
    d = p - T.reshape(1, 3)
    return (d[:, 0:1] * R[0] + d[:, 1:2] * R[1]) + d[:, 2:3] * R[2]


def closest(pts, verts, th, R=None, T=None):
    """nearest vertex of every point, both taken to the pose space first when (R, T) is given
    -> (q [N,3], idx [N] int32, dist [N], flag [N] int32); nothing here carries a gradient"""
    pts, verts = pts.detach().reshape(-1, 3), verts.detach().reshape(-1, 3)
    if _kernels(pts):
        from . import ops
        return ops.ani_closest(pts, verts, th, R, T)
    if R is not None:
        pts, verts = to_pose(pts, R, T.reshape(3)), to_pose(verts, R, T.reshape(3))
    idx, d2 = [], []
    for i in range(0, pts.shape[0], CLOSEST_CHUNK):
        d = pts[i:i + CLOSEST_CHUNK, None, :] - verts[None]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        m, j = dd.min(1)
        idx.append(j)
        d2.append(m)
    if not idx:
        z = pts.new_zeros((0,))
        return pts, z.int(), z, z.int()
    dist = torch.cat(d2).sqrt()
    return pts, torch.cat(idx).int(), dist, (dist < th).int()


def select(flag, dist):
    """indices (int64, ascending) of pind = flag; pind[argmin(dist)] = True.  One read of the count from the device."""
    if _kernels(dist):
        from . import ops
        lst, count = ops.ani_select(flag, dist)
        return lst[:int(count.item())].long()
    pind = flag.bool().clone()
    if pind.numel():
        pind[dist.argmin()] = True
    return pind.nonzero()[:, 0]


class _BlendFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, smpl_bw, idx):
        from . import ops
        bw = ops.ani_blend_forward(smpl_bw, idx, logits.detach())
        ctx.save_for_backward(bw)
        return bw

    @staticmethod
    def backward(ctx, g):
        from . import ops
        bw, = ctx.saved_tensors
        return ops.ani_blend_backward(bw, g.contiguous()), None, None


def blend_head(logits, smpl_bw, idx):
    """softmax_j(log(smpl_bw[idx, j] + 1e-9) + logits[:, j]) -> [N,24]"""
    if _kernels(logits):
        return _BlendFn.apply(logits.contiguous(), smpl_bw, idx)
    return F.softmax(torch.log(smpl_bw[idx.long()] + 1e-9) + logits, dim=1)


class _SkinFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bw, pts, dirs, a_from, a_to):
        from . import ops
        bw = bw.detach().contiguous()
        po, do = ops.ani_skin_forward(pts, dirs, bw, a_from, a_to)
        ctx.save_for_backward(bw, pts, dirs, a_from, a_to)
        if do is None:
            return po
        return po, do

    @staticmethod
    def backward(ctx, gp, gd=None):
        from . import ops
        bw, pts, dirs, a_from, a_to = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        return ops.ani_skin_backward(pts, dirs, bw, a_from, a_to, gp, gd), None, None, None, None


def skin(pts, dirs, bw, a_from, a_to):
    """pose_points_to_tpose_points(., bw, a_from) then tpose_points_to_pose_points(., bw, a_to), and the two direction functions:
    pts / dirs [N,3] (dirs may be None; neither carries a gradient), bw [N,24] -> (pts_out, dirs_out or None)"""
    pts = pts.detach()
    dirs = dirs.detach() if dirs is not None else None
    if _kernels(pts):
        out = _SkinFn.apply(bw, pts.contiguous(), dirs.contiguous() if dirs is not None else None, a_from.contiguous(), a_to.contiguous())
        return (out, None) if dirs is None else out
    A = torch.matmul(bw, a_from.reshape(J, 16)).view(-1, 4, 4)
    B = torch.matmul(bw, a_to.reshape(J, 16)).view(-1, 4, 4)
    r_inv = torch.inverse(A[:, :3, :3])
    p = torch.sum(r_inv * (pts - A[:, :3, 3])[:, None], dim=2)
    p = torch.sum(B[:, :3, :3] * p[:, None], dim=2) + B[:, :3, 3]
    if dirs is None:
        return p, None
    d = torch.sum(r_inv * dirs[:, None], dim=2)
    return p, torch.sum(B[:, :3, :3] * d[:, None], dim=2)


class _EmbedFn(torch.autograd.Function):
    """BaseEmbedder's encoding of [N,3] points (xr_nerf_encode) with its input gradient (xr_ani_encode_backward).  The output is the
    first ceil4(3 + 6 L) columns of the kernel's padded rows: finite values behind column 3 + 6 L, which the consumers meet with zero
    weight columns."""

    @staticmethod
    def forward(ctx, p, L):
        from . import ops
        p = p.detach().contiguous()
        e = ops.nerf_encode(p, p, L, 0)
        ctx.save_for_backward(p)
        ctx.L = L
        cp = 3 + 6 * L
        return torch.as_strided(e, (e.shape[0], (cp + 3) // 4 * 4), e.stride(), e.storage_offset())

    @staticmethod
    def backward(ctx, g):
        from . import ops
        p, = ctx.saved_tensors
        return ops.ani_encode_backward(p, g, ctx.L), None


def embed(p, L):
    """-> [N, K] with K = 3 + 6 L (tensor ops) or K rounded up to a multiple of 4 (kernels; the extra columns are to be ignored)"""
    from . import ops
    if _kernels(p) and p.shape[0] > 0 and ops.vanilla_kernels_available():
        return _EmbedFn.apply(p, int(L))
    parts = [p]
    for k in range(L):
        parts += [torch.sin(p * float(2.0 ** k)), torch.cos(p * float(2.0 ** k))]
    return torch.cat(parts, -1)


def _lin(x, w, b, relu=False):
    """act(x w^T + b): the linear kernels on the device (linear.linear_act_padded), torch on the host or with the tensor-op switch"""
    if _TENSOR_OPS:
        y = F.linear(x, w, b)
        return F.relu(y) if relu else y
    from .linear import linear_act_padded
    return linear_act_padded(x, w, b, relu)


def _cols(w, k):
    """weight columns for an input of k columns of which the first w.shape[1] are real"""
    return w if w.shape[1] == k else F.pad(w, (0, k - w.shape[1]))


# ------------------------------------------------------------------ MLPs
class _WeightNormLinear(nn.Module):
    """nn.utils.weight_norm(nn.Linear): parameters `weight_g` [out,1], `weight_v` [out,in] and `bias`; weight = g v / |v| per row"""

    def __init__(self, lin):
        super().__init__()
        w = lin.weight.detach()
        self.bias = nn.Parameter(lin.bias.detach().clone())          # (the state dict's order: bias, weight_g, weight_v)
        self.weight_g = nn.Parameter(w.norm(dim=1, keepdim=True))
        self.weight_v = nn.Parameter(w.clone())

    @property
    def weight(self):
        return torch._weight_norm(self.weight_v, self.weight_g, 0)


@MLPS.register_module()
class AN_BlendWeightMLP(nn.Module):
    def __init__(self, num_pose, embedder):
        super().__init__()
        self.bw_latent = nn.Embedding(num_pose + 1, 128)
        input_ch, D, W = 191, 8, 256
        self.skips = [4]
        self.bw_linears = nn.ModuleList([nn.Conv1d(input_ch, W, 1)] + [
            nn.Conv1d(W, W, 1) if i not in self.skips else nn.Conv1d(W + input_ch, W, 1) for i in range(D - 1)])
        self.bw_fc = nn.Conv1d(W, J, 1)
        self.embedder = builder.build_embedder(embedder)
        self.multires = int(embedder['multires'])
        assert 3 + 6 * self.multires + 128 == input_ch, 'AN_BlendWeightMLP is hard-wired to 63 + 128 input channels'

    def logits(self, pts, latent_index):
        """pts [N,3] -> the residual blend-weight logits [N,24]; a 1x1 Conv1d is a linear layer, the latent's product a bias"""
        e = embed(pts, self.multires)
        ce = 3 + 6 * self.multires
        latent = self.bw_latent(latent_index.reshape(-1)[:1].long())[0]
        net = None
        for i, layer in enumerate(self.bw_linears):
            w, b = layer.weight[:, :, 0], layer.bias
            if i == 0:
                net = _lin(e, _cols(w[:, :ce], e.shape[1]), b + w[:, ce:] @ latent, True)
            elif (i - 1) in self.skips:
                x = torch.cat([e, net], 1)
                net = _lin(x, torch.cat([_cols(w[:, :ce], e.shape[1]), w[:, ce + 128:]], 1), b + w[:, ce:ce + 128] @ latent, True)
            else:
                net = _lin(net, w, b, True)
        return _lin(net, self.bw_fc.weight[:, :, 0], self.bw_fc.bias)

    def neural_blend_weights(self, pts, smpl_bw, idx, latent_index):
        """pts [N,3], smpl_bw [V,24], idx [N] (nearest vertex) -> bw [N,24]"""
        return blend_head(self.logits(pts, latent_index), smpl_bw, idx)

    def calculate_neural_blend_weights(self, pose_pts, smpl_bw, latent_index):
        """the reference's signature: pose_pts [1,N,3], smpl_bw [1,24,N] (the gathered initial weights) -> [1,24,N]"""
        lg = self.logits(pose_pts[0], latent_index)
        return F.softmax(torch.log(smpl_bw[0].t() + 1e-9) + lg, dim=1).t()[None]


@MLPS.register_module()
class AN_DensityMLP(nn.Module):
    def __init__(self, embedder):
        super().__init__()
        d_out, d_hidden, n_layers = 257, 256, 8
        self.embedder = builder.build_embedder(embedder)
        self.multires = multires = int(embedder['multires'])
        input_ch, _ = self.embedder.get_embed_ch()
        dims = [input_ch] + [d_hidden] * n_layers + [d_out]
        self.skip_in = [4]
        self.num_layers = len(dims)
        bias = 0.5
        for l in range(self.num_layers - 1):
            out_dim = dims[l + 1] - dims[0] if l + 1 in self.skip_in else dims[l + 1]
            lin = nn.Linear(dims[l], out_dim)
            # geometric initialisation (aninerf_mlp.py:263-284)
            if l == self.num_layers - 2:
                torch.nn.init.normal_(lin.weight, mean=np.sqrt(np.pi) / np.sqrt(dims[l]), std=0.0001)
                torch.nn.init.constant_(lin.bias, -bias)
            elif multires > 0 and l == 0:
                torch.nn.init.constant_(lin.bias, 0.0)
                torch.nn.init.constant_(lin.weight[:, 3:], 0.0)
                torch.nn.init.normal_(lin.weight[:, :3], 0.0, np.sqrt(2) / np.sqrt(out_dim))
            elif multires > 0 and l in self.skip_in:
                torch.nn.init.constant_(lin.bias, 0.0)
                torch.nn.init.normal_(lin.weight, 0.0, np.sqrt(2) / np.sqrt(out_dim))
                torch.nn.init.constant_(lin.weight[:, -(dims[0] - 3):], 0.0)
            else:
                torch.nn.init.constant_(lin.bias, 0.0)
                torch.nn.init.normal_(lin.weight, 0.0, np.sqrt(2) / np.sqrt(out_dim))
            setattr(self, 'lin' + str(l), _WeightNormLinear(lin))
        self.activation = nn.Softplus(beta=100)

    def forward(self, inputs):
        """inputs [N,3] -> [N,257] = (alpha, 256 features)"""
        e = embed(inputs, self.multires)
        ce = 3 + 6 * self.multires
        x = e
        for l in range(self.num_layers - 1):
            lin = getattr(self, 'lin' + str(l))
            w = lin.weight
            if l in self.skip_in:
                x = torch.cat([x, e[:, :ce]], 1) / np.sqrt(2)
            x = _lin(x, _cols(w, x.shape[1]), lin.bias)
            if l < self.num_layers - 2:
                x = self.activation(x)
        return x


@MLPS.register_module()
class AN_ColorMLP(nn.Module):
    def __init__(self, num_train_pose, embedder):
        super().__init__()
        self.color_latent = nn.Embedding(num_train_pose, 128)
        d_feature, d_in, d_out, d_hidden = 256, 6, 3, 256
        self.embedder = builder.build_embedder(embedder)
        self.multires_dirs = int(embedder['multires_dirs'])
        _, input_ch = self.embedder.get_embed_ch()
        d0 = d_in + d_feature + (input_ch - 3)
        self.num_layers = 6
        self.lin0 = _WeightNormLinear(nn.Linear(d0, d_hidden))
        self.lin1 = _WeightNormLinear(nn.Linear(d_hidden, d_hidden))
        self.lin2 = _WeightNormLinear(nn.Linear(d_hidden, d_hidden))
        self.lin3 = _WeightNormLinear(nn.Linear(d_hidden + 128, d_hidden))
        self.lin4 = _WeightNormLinear(nn.Linear(d_hidden, d_out))

    @staticmethod
    def _w(lin):
        return lin.weight

    def forward(self, points, view_dirs, feature_vectors, latent_index):
        cd = 3 + 6 * self.multires_dirs
        x = torch.cat([points, embed(view_dirs, self.multires_dirs)[:, :cd], feature_vectors], dim=-1)
        net = _lin(x, self._w(self.lin0), self.lin0.bias, True)
        net = _lin(net, self._w(self.lin1), self.lin1.bias, True)
        net = _lin(net, self._w(self.lin2), self.lin2.bias, True)
        latent = self.color_latent(latent_index.reshape(-1)[:1].long())[0]
        w3 = self._w(self.lin3)
        H = net.shape[1]
        net = _lin(net, w3[:, :H], self.lin3.bias + w3[:, H:] @ latent, True)
        return _lin(net, self._w(self.lin4), self.lin4.bias)


# ------------------------------------------------------------------ deformation field
@MLPS.register_module()
class DeformField(nn.Module):
    def __init__(self, phase, smpl_threshold, bw_mlp, novel_pose_bw_mlp):
        super().__init__()
        self.phase = phase
        self.smpl_threshold = smpl_threshold
        self.bw_mlp = builder.build_mlp(bw_mlp)
        self.novel_pose_bw_mlp = builder.build_mlp(novel_pose_bw_mlp)

    def forward(self, datas):
        pts = datas['pts']
        n_ray, n_s = pts.shape[:2]
        R, T = datas['smpl_R'], datas['smpl_T'].reshape(3)
        with torch.no_grad():
            # world -> pose space, nearest posed vertex, "near the body" (get_posed_point_viewdir + get_points_near_smpl)
            q, idx, dist, flag = closest(pts.reshape(-1, 3), datas['smpl_verts'], self.smpl_threshold, R, T)
            sel = select(flag, dist)
            pose_pts, idx_p = q[sel], idx[sel]
            ray = torch.div(sel, n_s, rounding_mode='floor')
            pose_dirs = torch.matmul(datas['rays_d'], R)[ray]
        # transform_to_tpose (the second nearest-vertex query of the reference repeats the first on the selected points)
        if self.phase == 'novel_pose':
            pbw = self.novel_pose_bw_mlp.neural_blend_weights(pose_pts, datas['smpl_bw'], idx_p, datas['bw_latent_idx'])
        else:
            pbw = self.bw_mlp.neural_blend_weights(pose_pts, datas['smpl_bw'], idx_p, datas['bw_latent_idx'] + 1)
        tpose, tpose_dirs = skin(pose_pts, pose_dirs, pbw, datas['A'], datas['big_A'])
        # calculate_tpose_tbw
        _, idx_t, _, _ = closest(tpose, datas['canonical_smpl_verts'], self.smpl_threshold)
        tbw = self.bw_mlp.neural_blend_weights(tpose, datas['smpl_bw'], idx_t, torch.zeros_like(datas['bw_latent_idx']))
        pind = torch.zeros(n_ray * n_s, dtype=torch.bool, device=pts.device)
        pind[sel] = True
        return {'tpose': tpose, 'tpose_dirs': tpose_dirs, 'pind': pind[None], 'pbw': pbw.t()[None], 'tbw': tbw.t()[None],
                'sel': sel, 'pbw_rows': pbw, 'tbw_rows': tbw}


@MLPS.register_module()
class TPoseHuman(nn.Module):
    def __init__(self, **kwargs):
        super().__init__()
        self.density_network = builder.build_mlp(kwargs['density_mlp'])
        self.color_network = builder.build_mlp(kwargs['color_mlp'])

    def calculate_alpha(self, tpose):
        """tpose [1,N,3] -> [1,1,N]"""
        return self.density_network(tpose[0])[:, :1][None].transpose(1, 2)

    def forward(self, deform_ret, datas):
        wpts, viewdir = deform_ret['tpose'], deform_ret['tpose_dirs']
        out = self.density_network(wpts)
        rgb = self.color_network(wpts, viewdir, out[:, 1:], datas['color_latent_idx'])
        return torch.cat((rgb, out[:, :1]), dim=1)

    def filter_and_format_prediction(self, raw, deform_ret, datas, masked=False):
        """zero `raw` outside the canonical bounds, scatter it to [R, S, 4], and pick the blend-weight rows with alpha > 0 (plus the
        largest alpha).  masked: the rows stay whole and the choice comes back as a [N] mask (no device read)"""
        tpose = deform_ret['tpose']
        verts = datas['canonical_smpl_verts']
        min_xyz, max_xyz = verts.min(0)[0] - 0.05, verts.max(0)[0] + 0.05
        inside = ((tpose > min_xyz) & (tpose < max_xyz)).sum(1) == 3
        raw = torch.where(inside[:, None], raw, torch.zeros_like(raw))
        n_ray, n_s = datas['pts'].shape[:2]
        full = raw.new_zeros((n_ray * n_s, 4)).index_copy(0, deform_ret['sel'], raw)
        alpha = raw[:, 3].detach()
        alpha_ind = alpha > 0
        if alpha.numel():
            alpha_ind = alpha_ind.index_fill(0, alpha.argmax().reshape(1), True)
        datas['raw'] = full.view(n_ray, n_s, 4)
        if masked:
            ret = {'raw': datas['raw'], 'pbw_rows': deform_ret['pbw_rows'], 'tbw_rows': deform_ret['tbw_rows'], 'bw_mask': alpha_ind}
        else:
            ret = {'raw': datas['raw'], 'pbw': deform_ret['pbw_rows'][alpha_ind], 'tbw': deform_ret['tbw_rows'][alpha_ind]}
        return datas, ret


def masked_smooth_l1(a, b, mask):
    """F.smooth_l1_loss(a[mask], b[mask]) as a masked mean: no index list, no device read"""
    per = F.smooth_l1_loss(a, b, reduction='none').sum(1)
    m = mask.to(per.dtype)
    return (per * m).sum() / (m.sum() * a.shape[1])


# ------------------------------------------------------------------ novel-pose phase
class NovelPoseTraining:
    N_SAMPLES = 1024 * 64

    @staticmethod
    def calculate_bounds(points):
        return torch.stack([points.min(0)[0] - 0.05, points.max(0)[0] + 0.05])[None]

    @staticmethod
    def get_sampling_points(bounds, vals=None, n=None):
        """vals [1,n,3] uniform draws (made on the device when not given)"""
        if vals is None:
            vals = torch.rand((1, n or NovelPoseTraining.N_SAMPLES, 3), device=bounds.device)
        return (bounds[:, 1] - bounds[:, 0])[:, None] * vals.to(bounds.device) + bounds[:, 0][:, None]

    @staticmethod
    def _chosen(alpha):
        ind = alpha > 0
        return ind.index_fill(0, alpha.argmax().reshape(1), True)

    @staticmethod
    def ppts_to_tpose(net, world_pts, datas, canonical_bounds):
        th = net.cfg['deform_field']['smpl_threshold']
        df = net.deform_field
        pose_pts, idx_p, pnorm, _ = closest(world_pts, datas['smpl_verts'], th, datas['smpl_R'], datas['smpl_T'].reshape(3))
        pbw = df.novel_pose_bw_mlp.neural_blend_weights(pose_pts, datas['smpl_bw'], idx_p, datas['bw_latent_idx'])
        tpose, _ = skin(pose_pts, None, pbw, datas['A'], datas['big_A'])
        _, idx_t, _, _ = closest(tpose, datas['canonical_smpl_verts'], th)
        tbw = df.bw_mlp.neural_blend_weights(tpose, datas['smpl_bw'], idx_t, torch.zeros_like(datas['bw_latent_idx']))
        with torch.no_grad():
            alpha = net.tpose_human.density_network(tpose.detach())[:, 0]
            inside = ((tpose > canonical_bounds[0, 0]) & (tpose < canonical_bounds[0, 1])).sum(1) == 3
            alpha = torch.where(inside & (pnorm < th), alpha, torch.zeros_like(alpha))
            mask = NovelPoseTraining._chosen(alpha)
        return pbw, tbw, mask

    @staticmethod
    def tpose_to_ppts(net, tpose, datas):
        th = net.cfg['deform_field']['smpl_threshold']
        df = net.deform_field
        tpose = tpose.reshape(-1, 3)
        _, idx_t, tnorm, _ = closest(tpose, datas['canonical_smpl_verts'], th)
        tbw = df.bw_mlp.neural_blend_weights(tpose, datas['smpl_bw'], idx_t, torch.zeros_like(datas['bw_latent_idx']))
        pose_pts, _ = skin(tpose, None, tbw, datas['big_A'], datas['A'])
        # the posed vertices: the query's own (R, T) applies to points and vertices alike, the points are in the pose space already
        verts = to_pose(datas['smpl_verts'], datas['smpl_R'], datas['smpl_T'].reshape(3))
        _, idx_p, _, _ = closest(pose_pts, verts, th)
        pbw = df.novel_pose_bw_mlp.neural_blend_weights(pose_pts.detach(), datas['smpl_bw'], idx_p, datas['bw_latent_idx'])
        with torch.no_grad():
            alpha = net.tpose_human.density_network(tpose)[:, 0]
            alpha = torch.where(tnorm > th, torch.zeros_like(alpha), alpha)
            mask = NovelPoseTraining._chosen(alpha)
        return pbw, tbw, mask

    @staticmethod
    def calculate_loss(net, datas, draws=None):
        """draws: (world [1,n,3], canonical [1,n,3]) uniform draws in [0, 1), for tests; drawn on the device otherwise"""
        world_bounds = NovelPoseTraining.calculate_bounds(datas['smpl_verts'])
        canonical_bounds = NovelPoseTraining.calculate_bounds(datas['canonical_smpl_verts'])
        world_points = NovelPoseTraining.get_sampling_points(world_bounds, None if draws is None else draws[0])
        canonical_points = NovelPoseTraining.get_sampling_points(canonical_bounds, None if draws is None else draws[1])
        pbw0, tbw0, m0 = NovelPoseTraining.ppts_to_tpose(net, world_points[0], datas, canonical_bounds)
        pbw1, tbw1, m1 = NovelPoseTraining.tpose_to_ppts(net, canonical_points[0], datas)
        loss = masked_smooth_l1(pbw0, tbw0, m0) + masked_smooth_l1(pbw1, tbw1, m1)
        return {'loss': loss, 'log_vars': {'loss': loss.item()}, 'num_samples': world_points.shape[1],
                'bw_masks': (m0, m1), 'bw_rows': ((pbw0, tbw0), (pbw1, tbw1))}


# ------------------------------------------------------------------ network
@NETWORKS.register_module()
class AniNeRFNetwork(BaseNerfNetwork):
    def __init__(self, cfg, render=None):
        super().__init__()
        self.cfg = cfg = builder.ConfigDict.wrap(dict(cfg))
        self.chunk = cfg.chunk
        self.bs_data = cfg.bs_data
        self.phase = cfg.phase
        self.idx = 0
        self.tpose_human = builder.build_mlp(cfg.tpose_human)
        self.deform_field = builder.build_mlp(cfg.deform_field)
        self.render = builder.build_render(render)

    def get_params(self):
        if self.cfg.phase == 'train_pose':
            params = list(self.tpose_human.parameters()) + list(self.deform_field.bw_mlp.parameters())
            for p in self.deform_field.novel_pose_bw_mlp.parameters():
                p.requires_grad = False
        else:
            for p in self.tpose_human.parameters():
                p.requires_grad = False
            for p in self.deform_field.bw_mlp.parameters():
                p.requires_grad = False
            params = list(self.deform_field.novel_pose_bw_mlp.parameters())
        return params

    def forward(self, datas, is_test=False, masked=False):
        deform_ret = self.deform_field(datas)
        raw = self.tpose_human(deform_ret, datas)
        datas, tpose_ret = self.tpose_human.filter_and_format_prediction(raw, deform_ret, datas, masked=masked)
        datas, ret = self.render(datas, is_test)
        ret.update(tpose_ret)
        ret['deform'] = deform_ret
        return ret

    def train_pose_stage(self, datas):
        ret = self.forward(datas, is_test=False, masked=True)
        img_loss = img2mse(ret['rgb'], datas['target_s'])
        bw_loss = masked_smooth_l1(ret['pbw_rows'], ret['tbw_rows'], ret['bw_mask'])
        loss = img_loss + bw_loss
        return {'loss': loss, 'log_vars': {'loss': loss.item(), 'psnr': mse2psnr(img_loss).item()}, 'num_samples': ret['rgb'].shape[0],
                'img_loss': img_loss, 'bw_loss': bw_loss, 'ret': ret}

    def train_step(self, datas, optimizer, **kwargs):
        for k in datas:
            datas[k] = unfold_batching(datas[k])
        if self.cfg.phase == 'train_pose':
            return self.train_pose_stage(datas)
        return NovelPoseTraining.calculate_loss(self, datas, kwargs.get('draws'))

    def batchify_forward(self, datas, is_test=False):
        N = datas[self.bs_data].shape[0]
        all_ret = {}
        for i in range(0, N, self.chunk):
            chunk = {k: (v[i:i + self.chunk] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == N and k in _RAY_KEYS else v)
                     for k, v in datas.items()}
            ret = self.forward(chunk, is_test)
            for k in ('rgb', 'disp', 'acc'):
                all_ret.setdefault(k, []).append(ret[k])
        return {k: torch.cat(v, 0) for k, v in all_ret.items()}

    def val_step(self, datas, *args, **kwargs):
        rank, _ = get_dist_info()
        if rank != 0:
            return {}
        for k in datas:
            datas[k] = unfold_batching(datas[k])
        with torch.no_grad():
            ret = self.batchify_forward(datas, is_test=True)
        rgb = nb_recover_shape(ret['rgb'], datas['src_shape'], datas['mask_at_box']).cpu().numpy()
        disp = nb_recover_shape(ret['disp'], datas['src_shape'], datas['mask_at_box']).cpu().numpy()
        outputs = {'rgbs': [rgb], 'disps': [disp], 'rgb': rgb, 'idx': self.idx}
        if self.phase != 'render':
            image = nb_recover_shape(datas['target_s'], datas['src_shape'], datas['mask_at_box']).cpu().numpy()
            outputs.update({'gt_imgs': [image], 'gt_img': image})
        self.idx += 1
        return outputs


_RAY_KEYS = ('rays_o', 'rays_d', 'pts', 'z_vals', 'target_s', 'near', 'far', 'viewdirs')


def nb_recover_shape(data, to_shape, mask):
    """networks/utils/transforms.py:12-21: values of the masked pixels back into the [H, W] image"""
    shape = [int(v) for v in to_shape[:-1]]
    full = data.new_zeros([int(np.prod(shape))] + list(data.shape[1:]))
    full[mask.reshape(-1).bool()] = data
    return full.view(shape + list(data.shape[1:]))


# ------------------------------------------------------------------ a synthetic body (what synthetic_city is for BungeeNeRF)
def _rot(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def synthetic_body(V, seed, n_rays=32, n_samples=16, device=None):
    """`datas` of one frame of a made-up body, unbatched float32 tensors: 24 joints, V canonical vertices scattered around them,
    blend weights = softmax(-|v - joint|^2 / 0.02) in fp32 (far joints underflow to exactly 0, as real SMPL weights are sparse),
    `A` / `big_A` = rigid transforms about the joints with rotations up to 1.2 rad, a world transform `smpl_R` / `smpl_T`, the posed
    world vertices (linear blend skinning of the canonical ones), and rays whose samples cross the body."""
    rng = np.random.default_rng(seed)
    joints = rng.uniform([-0.45, -0.9, -0.15], [0.45, 0.9, 0.15], (J, 3))
    owner = rng.integers(0, J, V)
    canon = joints[owner] + rng.normal(0, 0.07, (V, 3))
    d2 = ((canon[:, None, :] - joints[None]) ** 2).sum(-1).astype(np.float32)
    lg = -d2 / np.float32(0.02)
    e = np.exp(lg - lg.max(1, keepdims=True), dtype=np.float32)
    bw = (e / e.sum(1, keepdims=True)).astype(np.float32)

    def rigid(max_angle, shift):
        out = np.zeros((J, 4, 4))
        for j in range(J):
            Rj = _rot(rng.normal(0, 1, 3), rng.uniform(0, max_angle))
            out[j, :3, :3] = Rj
            out[j, :3, 3] = joints[j] - Rj @ joints[j] + rng.normal(0, shift, 3)
            out[j, 3, 3] = 1
        return out
    A, big_A = rigid(1.2, 0.05), rigid(1.2, 0.05)
    Ab = (bw.astype(np.float64) @ A.reshape(J, 16)).reshape(V, 4, 4)
    Bb = (bw.astype(np.float64) @ big_A.reshape(J, 16)).reshape(V, 4, 4)
    # canonical = B A^-1 posed  ->  posed = A B^-1 canonical
    t = np.linalg.solve(Bb[:, :3, :3], (canon - Bb[:, :3, 3])[..., None])[..., 0]
    posed = np.einsum('vij,vj->vi', Ab[:, :3, :3], t) + Ab[:, :3, 3]
    R = _rot(rng.normal(0, 1, 3), rng.uniform(0.2, 1.0))
    T = rng.normal(0, 0.3, 3)
    world = posed @ R.T + T                                        # pose = (world - T) R
    # rays aimed at body vertices from a sphere around it; samples spread over +-0.6 around the hit
    centre = world.mean(0)
    o = rng.normal(0, 1, (n_rays, 3))
    o = centre + 3.0 * o / np.linalg.norm(o, axis=-1, keepdims=True)
    target = world[rng.integers(0, V, n_rays)] + rng.normal(0, 0.03, (n_rays, 3))
    d = target - o
    depth = np.linalg.norm(d, axis=-1, keepdims=True)
    d = d / depth
    edges = np.linspace(0.0, 1.0, n_samples + 1)
    z = depth - 0.6 + 1.2 * (edges[:-1] + (edges[1:] - edges[:-1]) * rng.uniform(0.05, 0.95, (n_rays, n_samples)))
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=device)
    return {'pts': f(pts), 'rays_o': f(o), 'rays_d': f(d), 'z_vals': f(z), 'near': f(z[:, :1]), 'far': f(z[:, -1:]),
            'target_s': f(rng.uniform(0, 1, (n_rays, 3))), 'smpl_verts': f(world), 'canonical_smpl_verts': f(canon), 'smpl_bw': f(bw),
            'A': f(A), 'big_A': f(big_A), 'smpl_R': f(R), 'smpl_T': f(T[None]), 'joints': f(joints),
            'bw_latent_idx': torch.tensor([3], dtype=torch.int64, device=device),
            'color_latent_idx': torch.tensor([3], dtype=torch.int64, device=device)}
