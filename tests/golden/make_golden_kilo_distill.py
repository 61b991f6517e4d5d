"""Generates tests/golden/ref_kilo_distill.npz from the REFERENCE'S OWN KiloNeRF distillation code (BASELINE config #5), in the
build container only:  python tests/golden/make_golden_kilo_distill.py

Run unmodified through tests/golden/ref_import.py (plus the few names its package shells lack, added below):
  StudentNerfNetwork      (models/networks/student_nerf.py:17-147): train_step, val_step, teacher_batchify_forward
  KiloNerfMultiNetwork    (models/mlps/kilonerf_multinet.py:25-102, MultiNetwork 'bmm', MultiNetworkLinear.reset_parameters)
  KiloNerfSimpleRender    (models/renders/kilonerf_simple_render.py)
  NerfMLP                 (models/mlps/nerf_mlp.py) as the teacher (netwidth 64 keeps the file small)
  calculate_error_metrics (core/hooks/save_distill_results_hook.py:44-112, the function's own source)
and the occupancy grid of core/hooks/build_occupancy_tree_hook.py:32-123, whose tensor arithmetic is restated line by line
(the hook itself needs an mmcv runner and a CUDA device).
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

N, B, NV = 8, 32, 48
FIXED_RES = [2, 2, 2]
GMIN, GMAX = [-0.67, -1.2, -0.37], [0.67, 1.2, 1.03]
SEED = 8078673
OCC_RES, OCC_SUB = [6, 5, 4], [3, 3, 3]


def load():
    ns = ref_import.load_kilo()
    import importlib
    utils = sys.modules['xrnerf.models.networks.utils']
    tr = importlib.import_module('xrnerf.models.networks.utils.transforms')
    utils.transform_examples = tr.transform_examples
    utils.unfold_batching = importlib.import_module('xrnerf.models.networks.utils.batching').unfold_batching
    mmcv = sys.modules['mmcv']
    mmcv.Config = type('Config', (), {'fromfile': staticmethod(lambda p: None)})
    ns.KiloNerfMultiNetwork = importlib.import_module('xrnerf.models.mlps.kilonerf_multinet').KiloNerfMultiNetwork
    ns.KiloNerfSimpleRender = importlib.import_module('xrnerf.models.renders.kilonerf_simple_render').KiloNerfSimpleRender
    ns.StudentNerfNetwork = importlib.import_module('xrnerf.models.networks.student_nerf').StudentNerfNetwork
    src = open(os.path.join(ref_import.REF, 'xrnerf/core/hooks/save_distill_results_hook.py')).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == 'calculate_error_metrics'][0]
    g = {'torch': torch, 'nn': torch.nn}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), 'save_distill_results_hook.py', 'exec'), g)
    ns.calculate_error_metrics = g['calculate_error_metrics']
    return ns


def mn_cfg(num_networks, same):
    return dict(type='KiloNerfMultiNetwork', num_networks=num_networks, alpha_rgb_initalization='pass_actual_nonlinearity',
                bias_initialization_method='standard', direction_layer_size=32, hidden_layer_size=32, late_feed_direction=True,
                network_rng_seed=SEED, nonlinearity_initalization='pass_actual_nonlinearity', num_hidden_layers=2,
                num_output_channels=4, refeed_position_index=None, use_same_initialization_for_all_networks=same,
                weight_initialization_method='kaiming_uniform',
                embedder=dict(type='KiloNerfFourierEmbedder', num_networks=num_networks, input_ch=3, multires=10, multires_dirs=4))


def main():
    assert ref_import.available()
    ns = load()
    torch.manual_seed(0)
    rng = np.random.default_rng(7)
    out = {}
    # teacher: the vanilla NerfMLP, narrow, with a density that crosses the occupancy threshold somewhere
    teacher = ns.NerfMLP(skips=[4], netdepth=8, netwidth=64, output_ch=4, use_viewdirs=True,
                         embedder=dict(type='BaseEmbedder', i_embed=0, multires=10, multires_dirs=4, input_ch=3))
    with torch.no_grad():
        teacher.alpha_linear.bias += 2.0
    for k, v in teacher.state_dict().items():
        out['teacher.' + k] = v.numpy()
    # domains as get_nodes_fixed_resolution builds them
    import itertools
    gmin, gmax = np.array(GMIN), np.array(GMAX)
    voxel = (gmax - gmin) / np.array(FIXED_RES)
    dmins = torch.tensor([(gmin + np.array(vi) * voxel).tolist() for vi in itertools.product(*[range(r) for r in FIXED_RES])], dtype=torch.float32)
    dmaxs = torch.tensor([(gmin + (np.array(vi) + 1) * voxel).tolist() for vi in itertools.product(*[range(r) for r in FIXED_RES])], dtype=torch.float32)
    out.update(domain_mins=dmins.numpy(), domain_maxs=dmaxs.numpy())
    # two consecutive constructions: the class-level RNG state continues; the second copies network 0 to all
    class Cfg(dict):                                   # mmcv ConfigDict's attribute access
        __getattr__ = dict.__getitem__
    model_cfg = dict(type='StudentNerfNetwork', cfg=Cfg(outputs='color_and_density', test_batch_size=512, query_batch_size=80000),
                     pretrained_kwargs=None, multi_network=mn_cfg(N, False),
                     render=dict(type='KiloNerfSimpleRender', alpha_distance=0.0211, convert_density_to_alpha=True))
    net = ns.builder.build_network(model_cfg)
    net.teacher_nerf = teacher
    second = ns.builder.build_mlp(mn_cfg(N, True))
    for k, v in net.multi_network.state_dict().items():
        out['init.' + k] = v.detach().numpy().copy()
    for k, v in second.state_dict().items():
        out['init2.' + k] = v.detach().numpy().copy()
    # one batch of examples: uniform points in each box, normalised Gaussian directions
    u = torch.tensor(rng.uniform(0, 1, (N, B, 3)), dtype=torch.float32)
    pos = dmins[:, None] + u * (dmaxs - dmins)[:, None]
    d = torch.tensor(rng.normal(0, 1, (N, B, 3)), dtype=torch.float32)
    d = d / d.norm(dim=-1, keepdim=True)
    ex = torch.cat([pos, d, torch.zeros(N, B, 4)], -1)
    out['examples'] = ex[..., :6].numpy().copy()
    with torch.no_grad():
        out['teacher_raw'] = teacher({'pts': ex[..., :3].reshape(-1, 3).clone(), 'viewdirs': ex[..., 3:6].reshape(-1, 3).clone()})['raw'].reshape(N, B, 4).numpy()
    opt = torch.optim.Adam(net.multi_network.parameters(), lr=1e-3)
    for step in range(5):
        data = {'batch_examples': ex.clone()[None], 'domain_mins': dmins[None], 'domain_maxs': dmaxs[None]}
        opt.zero_grad()
        res = net.train_step(data, opt)
        if step == 0:
            res2 = net(data)        # the students' rendered output on the transformed batch
            out['student_out'] = res2.detach().numpy()
            out['target'] = data['batch_examples'][..., 6:10].numpy()
            out['loss'] = np.float32(res['loss'].item())
        res['loss'].backward()
        if step == 0:
            for k, p in net.multi_network.named_parameters():
                out['grad.' + k] = p.grad.numpy().copy()
        opt.step()
        if step in (0, 4):
            for k, v in net.multi_network.state_dict().items():
                out['adam%d.' % (step + 1) + k] = v.detach().numpy().copy()
    # val_step on a separate batch (its own teacher targets) and the per-network error metrics
    uv = torch.tensor(rng.uniform(0, 1, (N, NV, 3)), dtype=torch.float32)
    dv = torch.tensor(rng.normal(0, 1, (N, NV, 3)), dtype=torch.float32)
    dv = dv / dv.norm(dim=-1, keepdim=True)
    vex = torch.cat([dmins[:, None] + uv * (dmaxs - dmins)[:, None], dv, torch.zeros(N, NV, 4)], -1)
    out['val_examples'] = vex[..., :6].numpy().copy()
    with torch.no_grad():
        vo = net.val_step({'batch_examples': vex.clone()[None], 'domain_mins': dmins[None], 'domain_maxs': dmaxs[None]})
    out['val_out'], out['val_target'] = vo['out'].numpy(), vo['target_s'].numpy()
    cfg = types.SimpleNamespace(outputs='color_and_density', quantile_se=0.99)
    _, per_net, per_color, per_density, sat = ns.calculate_error_metrics(vo['out'], vo['target_s'], cfg)
    for k in ('mse', 'mae', 'mape', 'quantile_se'):
        out['metric.' + k] = per_net[k].numpy()
        out['metric_color.' + k] = per_color[k].numpy()
        out['metric_density.' + k] = per_density[k].numpy()
    out['metric.saturation'] = sat.numpy()
    # occupancy grid: build_occupancy_tree_hook.py:37-110, line by line (CPU)
    global_domain_min, global_domain_max = torch.tensor(GMIN), torch.tensor(GMAX)
    global_domain_size = global_domain_max - global_domain_min
    occupancy_res = OCC_RES
    total_num_voxels = occupancy_res[0] * occupancy_res[1] * occupancy_res[2]
    occupancy_resolution = torch.tensor(occupancy_res, dtype=torch.long)
    occupancy_voxel_size = global_domain_size / occupancy_resolution
    first_voxel_min = global_domain_min
    first_voxel_max = first_voxel_min + occupancy_voxel_size
    first_voxel_samples = []
    for dim in range(3):
        first_voxel_samples.append(torch.linspace(first_voxel_min[dim], first_voxel_max[dim], OCC_SUB[dim]))
    first_voxel_samples = torch.stack(torch.meshgrid(*first_voxel_samples, indexing='ij'), dim=3).view(-1, 3)
    ranges = [torch.arange(0, occupancy_res[dim]) for dim in range(3)]
    index_grid = torch.stack(torch.meshgrid(*ranges, indexing='ij'), dim=3)
    index_grid = (index_grid * occupancy_voxel_size).unsqueeze(3)
    points = first_voxel_samples.unsqueeze(0).unsqueeze(0).unsqueeze(0).expand(occupancy_res + list(first_voxel_samples.shape))
    points = points + index_grid
    points = points.view(total_num_voxels, -1, 3)
    with torch.no_grad():
        dens = teacher({'pts': points.reshape(-1, 3).clone(), 'viewdirs': torch.zeros(points.reshape(-1, 3).shape)})['raw'][:, 3]
    dens = dens.view(total_num_voxels, -1)
    threshold = float(np.quantile(dens.max(dim=1)[0].numpy(), 0.5))
    occupancy_grid = (dens > threshold).view(OCC_RES + [-1]).any(dim=3)
    out.update(occ_points=points.numpy(), occ_density=dens.numpy(), occ_threshold=np.float32(threshold), occ_grid=occupancy_grid.numpy(),
               occ_res=np.int64(OCC_RES), occ_sub=np.int64(OCC_SUB), gmin=np.float32(GMIN), gmax=np.float32(GMAX))
    path = os.path.join(HERE, 'ref_kilo_distill.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes; loss %.6f, occupied %d of %d' % (out['loss'], int(occupancy_grid.sum()), total_num_voxels))


if __name__ == '__main__':
    main()
