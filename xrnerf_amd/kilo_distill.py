"""KiloNeRF distillation (BASELINE config #5, configs/kilonerf/kilonerf_distill_*.py): the phase between the vanilla-NeRF
teacher and the fine-tuned students.  Registry entries `KiloNerfMultiNetwork` (MLPS), `KiloNerfSimpleRender` (RENDERS) and
`StudentNerfNetwork` (NETWORKS) with the constructor signatures, `data` keys and state_dict names / shapes of
  xrnerf/models/mlps/kilonerf_multinet.py:25-102, mlps/multi_modules.py:238-340,405-565 (`bmm` layout
  [N, out, in]), renders/kilonerf_simple_render.py, networks/student_nerf.py:17-147,
plus the occupancy grid (core/hooks/build_occupancy_tree_hook.py:32-123) and a fixed-resolution `distill` driver
(datasets/kilonerf_node_dataset.py, core/hooks/distill_cycle_hook.py, save_distill_results_hook.py) whose checkpoint
`KiloNerfMLP(distilled_checkpoint=...)` loads unchanged.

The hot path is xrnerf_amd/csrc/xr_kilo.hip: xr_kilo_student_step (forward + renders + loss + backward [+ Adam] of all
students in one launch), xr_kilo_student_forward, xr_kilo_distill_examples, xr_kilo_occupancy_points / _reduce.  The teacher
query between them is the caller's NerfMLP.  No CPU path: host tensors raise.
"""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, builder, ops
from .builder import MLPS, NETWORKS, RENDERS
from .kilo import MultiNetwork as _PackedNetwork
from .networks import BaseNerfNetwork, unfold_batching


def _f32(t):
    if t.dtype != torch.float32:
        raise _lib.XrError('KiloNeRF distillation ops take float32 tensors (got %s)' % t.dtype)
    return t.contiguous()


def param_floats(pos_freqs, dir_freqs, n_hidden):
    return int(_lib.load().xr_kilo_param_floats(int(pos_freqs), int(dir_freqs), int(n_hidden)))


# ------------------------------------------------------------------ C-ABI wrappers
def student_step(examples, teacher_raw, domain_mins, domain_maxs, params, pos_freqs, dir_freqs, n_hidden, alpha_distance,
                 loss=None, grad=None, adam=None):
    """xr_kilo_student_step.  examples [N, B, >= 6] (global positions, directions), teacher_raw [N, B, 4], params [N, stride]
    packed blocks.  -> (loss [N], grad [N, stride] or None).  adam: dict(m, v, step, lr, betas, eps) -> params / m / v
    updated in place (grad is then only written when passed)."""
    ex, tr = _f32(examples), _f32(teacher_raw)
    N, B, S = ex.shape
    if loss is None:
        loss = torch.empty((N,), dtype=torch.float32, device=ex.device)
    if grad is None and (adam is None or B > 128):
        grad = torch.empty_like(params)
    m = v = None
    step, lr, b1, b2, eps = 0, 0., 0.9, 0.999, 1e-8
    if adam is not None:
        m, v, step, lr, eps = adam['m'], adam['v'], int(adam['step']), float(adam['lr']), float(adam.get('eps', 1e-8))
        b1, b2 = adam.get('betas', (0.9, 0.999))
    L = _lib.load()
    _lib.check(L.xr_kilo_student_step(ops._ptr(ex), S, ops._ptr(tr), ops._ptr(_f32(domain_mins)), ops._ptr(_f32(domain_maxs)),
                                      ops._ptr(params), params.stride(0), N, B, int(pos_freqs), int(dir_freqs), int(n_hidden),
                                      float(alpha_distance), ops._ptr(loss), ops._ptr(grad), ops._ptr(m), ops._ptr(v), step, lr,
                                      float(b1), float(b2), eps, ops._stream()), 'xr_kilo_student_step')
    return loss, grad


def student_forward(examples, params, pos_freqs, dir_freqs, n_hidden, domain_mins=None, domain_maxs=None, render=False,
                    alpha_distance=0., out=None):
    """xr_kilo_student_forward: [N, M, >= 6] -> [N, M, 4] raw (render=False) or [sigmoid(rgb), alpha] (render=True);
    without domains the positions are local coordinates already"""
    ex = _f32(examples)
    N, M, S = ex.shape
    if out is None:
        out = torch.empty((N, M, 4), dtype=torch.float32, device=ex.device)
    L = _lib.load()
    _lib.check(L.xr_kilo_student_forward(ops._ptr(ex), S, M, ops._ptr(None if domain_mins is None else _f32(domain_mins)),
                                         ops._ptr(None if domain_maxs is None else _f32(domain_maxs)), ops._ptr(params),
                                         params.stride(0), N, int(pos_freqs), int(dir_freqs), int(n_hidden), 1 if render else 0,
                                         float(alpha_distance), ops._ptr(out), ops._stream()), 'xr_kilo_student_forward')
    return out


def distill_examples(domain_mins, domain_maxs, batch, seed, iteration, pool_size=1000000, out=None):
    """xr_kilo_distill_examples -> [N, batch, 6]: uniform points in each network's box and unit directions, the example index of a
    slot shared by all networks (ExampleSample); a function of (seed, iteration) only"""
    dm = _f32(domain_mins)
    N = dm.shape[0]
    if out is None:
        out = torch.empty((N, int(batch), 6), dtype=torch.float32, device=dm.device)
    _lib.check(_lib.load().xr_kilo_distill_examples(int(seed), int(iteration), int(pool_size), ops._ptr(dm), ops._ptr(_f32(domain_maxs)),
                                                    N, int(batch), out.shape[2], ops._ptr(out), ops._stream()), 'xr_kilo_distill_examples')
    return out


def occupancy_points(domain_min, domain_max, resolution, subsample_resolution, voxel_begin, n_voxels, device, out=None):
    """xr_kilo_occupancy_points -> [n_voxels * prod(sub), 3], the hook's lattice bit for bit"""
    import ctypes as C
    f3, i3 = C.c_float * 3, C.c_int32 * 3
    S = int(np.prod(subsample_resolution))
    if out is None:
        out = torch.empty((int(n_voxels) * S, 3), dtype=torch.float32, device=device)
    _lib.check(_lib.load().xr_kilo_occupancy_points(f3(*[float(v) for v in domain_min]), f3(*[float(v) for v in domain_max]),
                                                    i3(*[int(v) for v in resolution]), i3(*[int(v) for v in subsample_resolution]),
                                                    int(voxel_begin), int(n_voxels), ops._ptr(out), ops._stream()),
               'xr_kilo_occupancy_points')
    return out


def occupancy_reduce(raw, samples_per_voxel, threshold, out):
    """xr_kilo_occupancy_reduce: out[v] (uint8 / bool, contiguous) = any(raw[v * spv + s, 3] > threshold)"""
    r = _f32(raw)
    n_vox = r.shape[0] // int(samples_per_voxel)
    o = out.view(torch.uint8) if out.dtype == torch.bool else out
    _lib.check(_lib.load().xr_kilo_occupancy_reduce(ops._ptr(r), r.shape[1], int(samples_per_voxel), float(threshold), n_vox, ops._ptr(o),
                                                    ops._stream()), 'xr_kilo_occupancy_reduce')
    return out


# ------------------------------------------------------------------ KiloNerfMultiNetwork ('bmm' layout)
def _gain(nonlinearity, param):
    """multi_modules.py:30-53"""
    if nonlinearity in ('linear', 'sigmoid'):
        return 1
    if nonlinearity == 'tanh':
        return 5.0 / 3
    if nonlinearity == 'relu':
        return math.sqrt(2.0)
    if nonlinearity == 'leaky_relu':
        slope = 0.01 if param is None else param
        return math.sqrt(2.0 / (1 + slope ** 2))
    raise ValueError('Unsupported nonlinearity {}'.format(nonlinearity))


class MultiNetworkLinear(nn.Module):
    """multi_modules.py:238-340 with implementation='bmm': bias [N, out] (registered first), weight [N, out, in]; kaiming-uniform
    weights (a = sqrt(5)) and fan-in-uniform biases drawn from a generator state kept at CLASS level across instances when
    network_rng_seed is set (the second cycle's networks continue the first cycle's stream), optionally network 0 copied to all"""
    rng_state = None

    def __init__(self, num_networks, in_features, out_features, nonlinearity='leaky_relu',
                 use_same_initialization_for_all_networks=False, network_rng_seed=None):
        super().__init__()
        self.num_networks, self.in_features, self.out_features = num_networks, in_features, out_features
        self.bias = nn.Parameter(torch.empty(num_networks, out_features))
        self.weight = nn.Parameter(torch.empty(num_networks, out_features, in_features))
        with torch.no_grad():
            if network_rng_seed is not None:
                previous = torch.random.get_rng_state()
                if MultiNetworkLinear.rng_state is None:
                    torch.random.manual_seed(network_rng_seed)
                else:
                    torch.random.set_rng_state(MultiNetworkLinear.rng_state)
            bound = math.sqrt(3.0) * (_gain(nonlinearity, math.sqrt(5)) / math.sqrt(in_features))
            self.weight.uniform_(-bound, bound)
            bb = 1 / math.sqrt(in_features)
            self.bias.uniform_(-bb, bb)
            if network_rng_seed is not None:
                MultiNetworkLinear.rng_state = torch.random.get_rng_state()
                torch.random.set_rng_state(previous)
            if use_same_initialization_for_all_networks:
                self.weight[1:] = self.weight[0]
                self.bias[1:] = self.bias[0]


class StudentMultiNetwork(nn.Module):
    """multi_modules.py:405-565 (late_feed_direction, relu, no position re-feed, H = 32): layers constructed in the reference's
    order (pts_linears, direction_layer, feature_linear, alpha_linear, rgb_linear), which is also their state_dict order"""

    def __init__(self, num_networks, num_position_channels, num_direction_channels, num_output_channels=4, hidden_layer_size=32,
                 num_hidden_layers=2, refeed_position_index=None, late_feed_direction=True, direction_layer_size=32,
                 nonlinearity_initalization='pass_actual_nonlinearity', use_same_initialization_for_all_networks=False,
                 network_rng_seed=None, alpha_rgb_initalization='updated_yenchenlin'):
        super().__init__()
        if not late_feed_direction or refeed_position_index is not None or num_output_channels != 4:
            raise NotImplementedError('only the late_feed_direction / no-refeed / 4-output architecture of the reference configs')
        if hidden_layer_size != 32 or direction_layer_size != 32 or num_hidden_layers not in (1, 2):
            raise NotImplementedError('hidden_layer_size = direction_layer_size = 32 and 1 or 2 hidden layers (the reference configs)')
        self.num_networks, self.num_hidden_layers = num_networks, num_hidden_layers
        self.num_position_channels, self.num_direction_channels = num_position_channels, num_direction_channels
        H = hidden_layer_size

        def lin(i, o, actual):
            passed = actual if nonlinearity_initalization == 'pass_actual_nonlinearity' else 'leaky_relu'
            return MultiNetworkLinear(num_networks, i, o, passed, use_same_initialization_for_all_networks, network_rng_seed)
        yen = alpha_rgb_initalization == 'updated_yenchenlin'
        self.pts_linears = nn.ModuleList([lin(num_position_channels, H, 'relu')] +
                                         [lin(H, H, 'relu') for _ in range(num_hidden_layers - 1)])
        self.direction_layer = lin(num_direction_channels + H, direction_layer_size, 'relu')
        self.feature_linear = lin(H, H, 'linear')
        self.alpha_linear = lin(H, 1, 'linear' if yen else 'relu')
        self.rgb_linear = lin(direction_layer_size, 3, 'linear' if yen else 'sigmoid')

        self._single_network_args = (num_position_channels, num_direction_channels, num_output_channels, hidden_layer_size, num_hidden_layers,
                                     refeed_position_index, late_feed_direction, direction_layer_size, nonlinearity_initalization, False, None,
                                     alpha_rgb_initalization)

    def get_single_network(self, network_index):
        """extract_single_network (multi_modules.py:672-710): a one-network copy of network `network_index` on the host, what the
        distillation's tree keeps per fitted node ('bmm' layout [1, out, in]; kilo.tree_to_checkpoint reads it)"""
        with torch.random.fork_rng(devices=[]):          # the copy's own initial draw must not move the caller's stream
            single = StudentMultiNetwork(1, *self._single_network_args)
        with torch.no_grad():
            for dst, src in zip(single.parameters(), self.parameters()):
                dst.copy_(src[network_index:network_index + 1])
        return single

    def ordered_parameters(self):
        """(weight, bias) per layer in the packed block order, weights transposed to the kernels' [N, in, out]"""
        layers = list(self.pts_linears) + [self.alpha_linear, self.feature_linear, self.direction_layer, self.rgb_linear]
        return [t for l in layers for t in (l.weight.transpose(1, 2), l.bias)]

    def packed(self):
        with torch.no_grad():
            return _PackedNetwork.pack([p.detach() for p in self.ordered_parameters()])

    def load_packed(self, blocks):
        """packed blocks -> the parameters (in place)"""
        with torch.no_grad():
            layers = list(self.pts_linears) + [self.alpha_linear, self.feature_linear, self.direction_layer, self.rgb_linear]
            for l, (w, b) in zip(layers, _pairs(_PackedNetwork.unpack_like(blocks, self.ordered_parameters()))):
                l.weight.copy_(w.transpose(1, 2))
                l.bias.copy_(b)

    def grads_from_blocks(self, blocks):
        """gradient blocks -> one tensor per parameter, in self.parameters() order"""
        layers = list(self.pts_linears) + [self.alpha_linear, self.feature_linear, self.direction_layer, self.rgb_linear]
        g = {}
        for l, (w, b) in zip(layers, _pairs(_PackedNetwork.unpack_like(blocks, self.ordered_parameters()))):
            g[id(l.weight)], g[id(l.bias)] = w.transpose(1, 2).contiguous(), b.contiguous()
        return [g[id(p)] for p in self.parameters()]


def _pairs(flat):
    return list(zip(flat[0::2], flat[1::2]))


@MLPS.register_module()
class KiloNerfMultiNetwork(nn.Module):
    """kilonerf_multinet.py:25-102.  forward(data): data['batch_positions'] (local coordinates) / data['batch_directions']
    [N, B, 3] -> data['raw'] [N, B, 4] through xr_kilo_student_forward (Fourier features in registers).  Gradients are not
    taken through forward: StudentNerfNetwork.train_step runs the fused step (xr_kilo_student_step)."""

    def __init__(self, num_networks, alpha_rgb_initalization, bias_initialization_method, direction_layer_size, hidden_layer_size,
                 late_feed_direction, network_rng_seed, nonlinearity_initalization, num_hidden_layers, num_output_channels,
                 refeed_position_index, use_same_initialization_for_all_networks, weight_initialization_method, embedder=None,
                 embedder_dir=None):
        super().__init__()
        self.embedder = builder.build_embedder(embedder)
        pos_ch, dir_ch = self.embedder.get_embed_ch()
        # (the reference passes neither initialization method on to its layers: kaiming-uniform / fan-in-uniform always)
        self.multi_network = StudentMultiNetwork(num_networks, pos_ch, dir_ch, num_output_channels, hidden_layer_size,
                                                 num_hidden_layers, refeed_position_index, late_feed_direction, direction_layer_size,
                                                 nonlinearity_initalization, use_same_initialization_for_all_networks,
                                                 network_rng_seed, alpha_rgb_initalization)

    @property
    def arch(self):
        return self.embedder.multires, self.embedder.multires_dirs, self.multi_network.num_hidden_layers

    def get_single_network(self, network_index):
        """kilonerf_multinet.py:99-102"""
        return self.multi_network.get_single_network(network_index)

    def forward(self, data):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError('KiloNerfMultiNetwork.forward carries no gradient: train through StudentNerfNetwork.train_step '
                                      '(one fused step kernel) or call it under torch.no_grad()')
        ex = torch.cat([data['batch_positions'], data['batch_directions']], -1)
        data['raw'] = student_forward(ex, self.multi_network.packed(), *self.arch)
        return data


@RENDERS.register_module()
class KiloNerfSimpleRender(nn.Module):
    """kilonerf_simple_render.py: rgb = sigmoid(raw[..., :3]); alpha = 1 - exp(-act(raw[..., 3]) * alpha_distance) with act = relu
    for 2-D raw (the teacher) and leaky_relu for 3-D raw (the students)"""

    def __init__(self, white_bkgd=False, raw_noise_std=0, rgb_padding=0, density_bias=0, density_activation='relu',
                 convert_density_to_alpha=True, alpha_distance=0, **kwarg):
        super().__init__()
        self.white_bkgd, self.raw_noise_std, self.rgb_padding, self.density_bias = white_bkgd, raw_noise_std, rgb_padding, density_bias
        self.convert_density_to_alpha, self.alpha_distance = convert_density_to_alpha, alpha_distance

    def process_density(self, raw):
        if raw.dim() == 2:
            d = F.relu(raw[:, 3])
        else:
            d = F.leaky_relu(raw[:, :, 3])
        if self.convert_density_to_alpha:
            d = 1. - torch.exp(-d * self.alpha_distance)
        return d.unsqueeze(-1)

    def forward(self, data):
        raw = data['raw']
        ret = torch.cat((torch.sigmoid(raw[..., 0:3]), self.process_density(raw)), dim=-1)
        return data, ret


class _StudentLoss(torch.autograd.Function):
    """sum over networks of the per-network loss of xr_kilo_student_step; backward hands the kernel's gradient to the parameters"""

    @staticmethod
    def forward(ctx, loss_n, grads, *params):
        ctx.grads = grads
        return loss_n.sum()

    @staticmethod
    def backward(ctx, g):
        return (None, None) + tuple(t * g for t in ctx.grads)


@NETWORKS.register_module()
class StudentNerfNetwork(BaseNerfNetwork):
    """student_nerf.py:17-147.  The teacher is the caller's NerfMLP: `teacher` passed in directly, or built from
    pretrained_kwargs (config: a dict or a config file with `model`; checkpoint with 'state_dict'), queried under no_grad."""

    def __init__(self, cfg, pretrained_kwargs=None, multi_network=None, render=None, teacher=None):
        super().__init__()
        cfg = builder.ConfigDict.wrap(dict(cfg))
        self.outputs = cfg.get('outputs', 'color_and_density')
        self.query_batch_size = cfg.get('query_batch_size')
        self.test_batch_size = cfg.get('test_batch_size', 0)
        self.teacher_nerf = teacher
        if pretrained_kwargs is not None and teacher is None:
            self.teacher_nerf = self._load_teacher(builder.ConfigDict.wrap(dict(pretrained_kwargs)))
        if multi_network is not None:
            self.multi_network = builder.build_mlp(multi_network)
        if render is not None:
            self.render = builder.build_render(render)

    @staticmethod
    def _load_teacher(pk):
        cfg = pk.config
        if isinstance(cfg, str):
            import runpy
            cfg = runpy.run_path(cfg)
        net = builder.build_network(builder.ConfigDict.wrap(dict(cfg['model'])))
        net.load_state_dict(torch.load(pk.checkpoint, map_location='cpu', weights_only=True)['state_dict'])
        return net.mlp

    def get_params(self):
        return list(self.multi_network.parameters())

    def _teacher_raw(self, ex):
        """NerfMLP on every example ([N, B, >= 6]) -> raw [N, B, 4]"""
        N, B = ex.shape[:2]
        with torch.no_grad():
            d = {'pts': ex[..., 0:3].reshape(-1, 3), 'viewdirs': ex[..., 3:6].reshape(-1, 3)}
            return self.teacher_nerf(d)['raw'].reshape(N, B, 4)

    def _teacher_fill(self, data):
        """teacher_batchify_forward: batch_examples[..., 6:10] = the teacher's rendered [rgb, alpha]; -> the teacher's raw"""
        ex = data['batch_examples']
        raw = self._teacher_raw(ex)
        if ex.shape[-1] >= 10:
            with torch.no_grad():
                ex[..., 6:10] = self.render({'raw': raw.reshape(-1, 4)})[1].reshape(raw.shape)
        return raw

    def train_step(self, data, optimizer, **kwargs):
        for k in data:
            data[k] = unfold_batching(data[k])
        raw_t = self._teacher_fill(data)
        mn = self.multi_network
        loss_n, grad = student_step(data['batch_examples'], raw_t, data['domain_mins'], data['domain_maxs'], mn.multi_network.packed(),
                                    *mn.arch, self.render.alpha_distance)
        params = list(mn.multi_network.parameters())
        loss = _StudentLoss.apply(loss_n, mn.multi_network.grads_from_blocks(grad), *params)
        lv = float(loss.detach())
        N, B = data['batch_examples'].shape[:2]
        return {'loss': loss, 'log_vars': {'sum_loss': lv, 'avg_loss': lv / N}, 'num_samples': B}

    def val_step(self, data, **kwargs):
        for k in data:
            data[k] = unfold_batching(data[k])
        self._teacher_fill(data)
        ex = data['batch_examples']
        dmin, dmax = data['domain_mins'], data['domain_maxs']
        mn = self.multi_network
        out = student_forward(ex, mn.multi_network.packed(), *mn.arch, domain_mins=dmin, domain_maxs=dmax, render=True,
                              alpha_distance=self.render.alpha_distance)
        error_log = ['{} {}\n'.format(dmin[i].cpu().tolist(), dmax[i].cpu().tolist()) for i in range(ex.shape[0])]
        return {'out': out, 'target_s': ex[..., 6:10], 'test_points': ex[..., :3], 'error_log': error_log}


def calculate_error_metrics(out, test_targets, quantile_se=0.99, outputs='color_and_density'):
    """save_distill_results_hook.py:44-112 with torch ops on the device -> (errors_per_network, _color, _density, saturation)"""
    tol = 0.001
    c, t = out[:, :, :3], test_targets[:, :, :3]
    sat0 = ((c.abs() < tol).all(dim=1) & ~(t.abs() < tol).all(dim=1)).any(dim=1)
    sat1 = (((c - 1).abs() < tol).all(dim=1) & ~((t - 1).abs() < tol).all(dim=1)).any(dim=1)
    errors = {'mse': F.mse_loss(out, test_targets, reduction='none'), 'mae': (out - test_targets).abs()}
    errors['mape'] = errors['mae'] / (test_targets.abs() + 0.1)
    per_net, per_color, per_density = {}, {}, {}
    for k in ('mse', 'mape', 'mae'):
        per_net[k] = errors[k].mean(dim=2).mean(dim=1)
        if outputs == 'density':
            per_density[k] = per_net[k]
        else:
            per_color[k] = errors[k][:, :, :3].mean(dim=2).mean(dim=1)
            per_density[k] = errors[k][:, :, 3].mean(dim=1)
    qi = int(errors['mse'].size(1) * quantile_se)

    def quantile(se):
        return torch.sort(se, dim=1)[0][:, qi]
    per_net['quantile_se'] = quantile(errors['mse'].mean(dim=2))
    per_color['quantile_se'] = quantile(errors['mse'][:, :, :3].mean(dim=2))
    per_density['quantile_se'] = quantile(errors['mse'][:, :, 3])
    return per_net, per_color, per_density, sat0 | sat1


# ------------------------------------------------------------------ occupancy grid and the distillation driver
@torch.no_grad()
def build_occupancy_grid(teacher_mlp, domain_min, domain_max, resolution, subsample_resolution=(3, 3, 3), threshold=10,
                         voxel_batch_size=16384):
    """build_occupancy_tree_hook.py:32-123 -> bool [rx, ry, rz] on the teacher's device: the hook's sub-voxel lattice, the teacher's
    density there (the direction input does not matter), any(sigma > threshold) per voxel"""
    dev = next(teacher_mlp.parameters()).device
    res = [int(r) for r in resolution]
    S = int(np.prod(subsample_resolution))
    total = res[0] * res[1] * res[2]
    occ = torch.empty(res, dtype=torch.bool, device=dev)
    flat = occ.view(-1)
    nb = min(int(voxel_batch_size), total)
    pts = torch.empty((nb * S, 3), dtype=torch.float32, device=dev)
    dirs = torch.zeros((nb * S, 3), dtype=torch.float32, device=dev)
    dirs[:, 2] = 1.
    for v0 in range(0, total, nb):
        n = min(nb, total - v0)
        p = occupancy_points(domain_min, domain_max, res, subsample_resolution, v0, n, dev, out=pts[:n * S])
        raw = teacher_mlp({'pts': p, 'viewdirs': dirs[:n * S]})['raw']
        occupancy_reduce(raw, S, threshold, flat[v0:v0 + n])
    return occ


def fixed_resolution_domains(global_domain_min, global_domain_max, fixed_resolution):
    """get_nodes_fixed_resolution (kilonerf_node_dataset.py:108-135): numpy float64 boxes in itertools.product order -> float32 [N, 3]"""
    gmin, gmax, fr = np.array(global_domain_min), np.array(global_domain_max), np.array(fixed_resolution)
    voxel = (gmax - gmin) / fr
    mins, maxs = [], []
    for vi in itertools.product(*[range(r) for r in fixed_resolution]):
        mins.append((gmin + vi * voxel).tolist())
        maxs.append((gmin + (vi + np.array(1)) * voxel).tolist())
    return torch.tensor(mins, dtype=torch.float32), torch.tensor(maxs, dtype=torch.float32)


def _default_student(num_networks, network_rng_seed, pos_freqs, dir_freqs, num_hidden_layers):
    # configs/kilonerf/kilonerf_distill_Synthetic_NeRF_base01.py:88-115
    return KiloNerfMultiNetwork(num_networks, 'pass_actual_nonlinearity', 'standard', 32, 32, True, network_rng_seed,
                                'pass_actual_nonlinearity', num_hidden_layers, 4, None, True, 'kaiming_uniform',
                                embedder=dict(type='KiloNerfFourierEmbedder', num_networks=num_networks, multires=pos_freqs,
                                              multires_dirs=dir_freqs, input_ch=3))


def distill(teacher_mlp, global_domain_min, global_domain_max, fixed_resolution, max_num_networks=512, max_iters=150000,
            train_batch_size=128, lr=1e-3, alpha_distance=0.0211, pos_freqs=10, dir_freqs=4, num_hidden_layers=2,
            network_rng_seed=8078673, seed=0, num_examples_per_network=1000000, val_every=0, num_val_examples=1024,
            quantile_se=0.99, max_error=100000, log=None):
    """The fixed-resolution distillation of the shipped configs: ceil(N / max_num_networks) cycles of max_iters fused Adam steps
    (lr, betas 0.9 / 0.999, eps 1e-8) on train_batch_size device-generated examples per network, each iteration's examples labelled
    by the teacher.  A fixed validation set per cycle has its teacher targets computed once; every val_every iterations (and at the
    end of the cycle) the students are evaluated on it.  -> {'domain_mins', 'domain_maxs', 'state_dict' (multimatmul layout,
    networks in fixed-resolution order), 'num_hidden_layers', 'error_metrics'}: what KiloNerfMLP(distilled_checkpoint=...) reads."""
    if max_error < 100000:
        raise NotImplementedError('kd-tree splitting (max_error < 1e5) is not implemented: only the fixed-resolution distillation '
                                  'of the shipped configs')
    dev = next(teacher_mlp.parameters()).device
    dmins_all, dmaxs_all = fixed_resolution_domains(global_domain_min, global_domain_max, fixed_resolution)
    total = dmins_all.shape[0]
    render = KiloNerfSimpleRender(alpha_distance=alpha_distance)
    blocks, metrics = [], {'mse': [], 'mae': [], 'mape': [], 'quantile_se': []}
    for cycle in range((total + max_num_networks - 1) // max_num_networks):
        n0, n1 = cycle * max_num_networks, min(total, (cycle + 1) * max_num_networks)
        dmin, dmax = dmins_all[n0:n1].to(dev), dmaxs_all[n0:n1].to(dev)
        student = _default_student(n1 - n0, network_rng_seed, pos_freqs, dir_freqs, num_hidden_layers)
        params = student.multi_network.packed().to(dev)
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        arch = (pos_freqs, dir_freqs, num_hidden_layers)
        val_ex = distill_examples(dmin, dmax, num_val_examples, seed + 0x5eed0000 + cycle, 0, num_examples_per_network)
        with torch.no_grad():
            val_t = render({'raw': teacher_mlp({'pts': val_ex[..., :3].reshape(-1, 3),
                                                'viewdirs': val_ex[..., 3:6].reshape(-1, 3)})['raw']})[1].reshape(n1 - n0, -1, 4)
        ex = torch.empty((n1 - n0, train_batch_size, 6), dtype=torch.float32, device=dev)
        loss = torch.empty((n1 - n0,), dtype=torch.float32, device=dev)
        adam = dict(m=m, v=v, step=0, lr=lr)

        def validate():
            out = student_forward(val_ex, params, *arch, domain_mins=dmin, domain_maxs=dmax, render=True, alpha_distance=alpha_distance)
            return calculate_error_metrics(out, val_t, quantile_se)
        for it in range(max_iters):
            distill_examples(dmin, dmax, train_batch_size, seed + cycle, it, num_examples_per_network, out=ex)
            with torch.no_grad():
                raw_t = teacher_mlp({'pts': ex[..., :3].reshape(-1, 3), 'viewdirs': ex[..., 3:6].reshape(-1, 3)})['raw']
            adam['step'] = it + 1
            student_step(ex, raw_t.reshape(n1 - n0, train_batch_size, 4), dmin, dmax, params, *arch, alpha_distance, loss=loss, adam=adam)
            if val_every and (it + 1) % val_every == 0 and log is not None:
                log('cycle %d iter %d: train loss %.6g, val mse %.6g' % (cycle, it + 1, float(loss.sum()), float(validate()[0]['mse'].mean())))
        per_net = validate()[0]
        for k in metrics:
            metrics[k] += per_net[k].cpu().tolist()
        blocks.append(params)
    blocks = torch.cat(blocks, 0)
    # multimatmul layout under KiloNerfMLP's names
    ref = _PackedNetwork(total, 3 * (2 * pos_freqs + 1), 3 * (2 * dir_freqs + 1), 4, 32, num_hidden_layers)
    names = ['pts_linears.%d' % l for l in range(num_hidden_layers)] + ['alpha_linear', 'feature_linear', 'direction_layer', 'rgb_linear']
    tensors = _PackedNetwork.unpack_like(blocks, [p.to(blocks.device) for p in ref.ordered_parameters()])
    sd = {}
    for i, nm in enumerate(names):
        sd[nm + '.weight'], sd[nm + '.bias'] = tensors[2 * i].detach().cpu().contiguous(), tensors[2 * i + 1].detach().cpu().contiguous()
    return {'domain_mins': dmins_all, 'domain_maxs': dmaxs_all, 'state_dict': sd, 'num_hidden_layers': num_hidden_layers,
            'error_metrics': metrics}


class BuildOccupancyTreeHook:
    """core/hooks/build_occupancy_tree_hook.py:18-123: after the pretraining run, the occupancy grid of the trained coarse MLP
    (build_occupancy_grid over cfg.build_occupancy_tree_config) saved as <occupancy work_dir>/occupancy.pth -- the file the fine-tuning
    config's mlp loads"""

    def __init__(self, cfg=None):
        assert cfg, 'cfg not input in BuildOccupancyTreeHook'
        self.cfg = cfg
        self.occupancy_config = cfg.build_occupancy_tree_config

    def after_run(self, runner):
        import os
        from .kilodata import get_global_domain_min_and_max
        oc = self.occupancy_config
        pretrained_nerf = getattr(runner.model, 'module', runner.model).mlp
        gmin, gmax = get_global_domain_min_and_max(self.cfg, torch.device('cpu'))
        occupancy_grid = build_occupancy_grid(pretrained_nerf, gmin.tolist(), gmax.tolist(), list(oc.resolution), tuple(oc.subsample_resolution),
                                              oc.threshold, oc.voxel_batch_size)
        occupied = int(occupancy_grid.sum().item())
        runner.logger.info('{} out of {} voxels are occupied. {:.2f}%'.format(occupied, occupancy_grid.numel(),
                                                                           100 * occupied / occupancy_grid.numel()))
        os.makedirs(oc.work_dir, exist_ok=True)
        occupancy_filename = oc.work_dir + '/occupancy.pth'
        torch.save(occupancy_grid, occupancy_filename)
        runner.logger.info('Saved occupancy grid to {}'.format(occupancy_filename))
