"""KiloNeRF's discovery loop on the MI355X, end to end (xrnerf_amd/kilo_tree.py): distill_from_config grows a kd-tree of students under the
analytic teacher of tests/test_gpu_kilo_distill.py, saves checkpoint.pth every cycle and hands its leaves to KiloNerfMLP; the
equal-error split takes its threshold from xr_kilotree_val_metrics; with max_error = 100000 the tree stays the fixed-resolution forest."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

AD = 0.0211
GMIN, GMAX = [-0.8, -0.7, -0.6], [0.8, 0.7, 0.6]            # longest axis x, then y


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def distill_cfg(work, tree_type='kdtree_longest', max_error=0, max_tree_cycles=None, max_num_networks=4, max_iters=20, val_examples=300,
                fixed_resolution=None):
    """the keys of configs/kilonerf/kilonerf_distill_*.py the loop reads, at test size"""
    emb = dict(type='KiloNerfFourierEmbedder', num_networks=max_num_networks, input_ch=3, multires=10, multires_dirs=4)
    base = dict(dataset_type='nsvf', global_domain_min=list(GMIN), global_domain_max=list(GMAX), mode='train', batch_index=0, work_dir=work,
                num_examples_per_network=100000, max_num_networks=max_num_networks, train_batch_size=128, outputs='color_and_density',
                is_batching=False)
    if fixed_resolution:
        base['fixed_resolution'] = fixed_resolution
    tensors = dict(type='ToTensor', enable=True, keys=['domain_mins', 'domain_maxs'])
    cfg = dict(method='kilo_nerf', phase='distill', optimizer=dict(type='Adam', lr=0.001), max_iters=max_iters, distributed=False,
               workflow=[('train', max_iters), ('val', 1)], train_runner=dict(type='KiloNerfDistillTrainRunner'), work_dir=work,
               max_num_networks=max_num_networks, num_networks=max_num_networks, outputs='color_and_density', alpha_distance=AD,
               quantile_se=0.99, tree_type=tree_type, test_error_metric='quantile_se', equal_split_metric='mse', max_error=max_error,
               model=dict(type='StudentNerfNetwork', cfg=dict(outputs='color_and_density', test_batch_size=512, query_batch_size=80000),
                          multi_network=dict(type='KiloNerfMultiNetwork', num_networks=max_num_networks,
                                             alpha_rgb_initalization='pass_actual_nonlinearity', bias_initialization_method='standard',
                                             direction_layer_size=32, hidden_layer_size=32, late_feed_direction=True, network_rng_seed=8078673,
                                             nonlinearity_initalization='pass_actual_nonlinearity', num_hidden_layers=2, num_output_channels=4,
                                             refeed_position_index=None, use_same_initialization_for_all_networks=True,
                                             weight_initialization_method='kaiming_uniform', embedder=emb),
                          render=dict(type='KiloNerfSimpleRender', alpha_distance=AD, convert_density_to_alpha=True)),
               data=dict(train=dict(type='KiloNerfNodeDataset', cfg=dict(base),
                                    pipeline=[dict(type='ExampleSample', enable=True, train_batch_size=128), tensors,
                                              dict(type='DeleteUseless', enable=True, keys=['all_examples'])]),
                         val=dict(type='KiloNerfNodeDataset', cfg=dict(base, mode='val', num_examples_per_network=val_examples), pipeline=[tensors])))
    if max_tree_cycles is not None:
        cfg['max_tree_cycles'] = max_tree_cycles
    return cfg


class Recorder:
    """keeps every validation's outputs by iteration (registered ahead of the distillation's own hooks)"""

    def __init__(self):
        self.outputs, self.models = {}, {}

    def after_val_iter(self, runner):
        self.outputs[runner.iter] = {k: v.clone() if torch.is_tensor(v) else list(v) for k, v in runner.outputs.items()}
        self.models[runner.iter] = runner.model


def run(cfg, dev):
    from test_gpu_kilo_distill import BoxFieldTeacher
    from xrnerf_amd import kilo_distill as KD, kilo_tree as T
    KD.MultiNetworkLinear.rng_state = None
    runner, datasets, workflow = T.build_distill_runner(cfg, teacher=BoxFieldTeacher().to(dev))
    rec = Recorder()
    runner.hooks.insert(0, rec)
    runner.run(datasets, workflow)
    return runner, T.final_cp(runner, datasets[0]), rec


def volume(lo, hi):
    return float(np.prod(np.array(hi, np.float64) - np.array(lo, np.float64)))


def check_longest_axis_tree(dev, work):
    from xrnerf_amd import kilo, kilo_distill as KD, kilo_tree as T
    from xrnerf_amd.kilodata import KiloNerfNodeDataset
    cfg = distill_cfg(work, max_tree_cycles=3)
    runner, cp, rec = run(cfg, dev)
    assert runner.iter == 60 and sorted(rec.outputs) == [20, 40, 60]                      # exactly three cycles
    assert [rec.outputs[i]['out'].shape[0] for i in (20, 40, 60)] == [1, 2, 4]            # of 1, 2 and 4 networks
    leaves = T.leaves_to_checkpoint(cp)
    want_min = [[-0.8, -0.7, -0.6], [-0.8, 0.0, -0.6], [0.0, -0.7, -0.6], [0.0, 0.0, -0.6]]   # x halved, then y: breadth-first
    want_max = [[0.0, 0.0, 0.6], [0.0, 0.7, 0.6], [0.8, 0.0, 0.6], [0.8, 0.7, 0.6]]
    assert np.allclose(leaves['domain_mins'].numpy(), want_min, atol=1e-7) and np.allclose(leaves['domain_maxs'].numpy(), want_max, atol=1e-7)
    vols = sum(volume(lo, hi) for lo, hi in zip(leaves['domain_mins'].tolist(), leaves['domain_maxs'].tolist()))
    assert math.isclose(vols, cp['total_volume'], rel_tol=1e-6) and math.isclose(cp['fitted_volume'], cp['total_volume'], rel_tol=1e-12)
    assert cp['num_networks_fitted'] == 4 and not cp['nodes_to_process'] and not cp['saturated_nodes_to_process']
    log = open(os.path.join(work, 'log.txt')).read()
    assert log.count('network_index:') == 7 and '[quantile_se]\ttotal | weighted mean' in log
    # checkpoint.pth is what the next batch would start from
    again = KiloNerfNodeDataset(dict(cfg['data']['train']['cfg'], batch_index=1), [], device=dev)
    assert again.cp['num_networks_fitted'] == 4 and again.node_batch == [] and len(again.cp['root_nodes']) == 1
    assert torch.equal(kilo.load_reference_distilled_checkpoint(os.path.join(work, 'checkpoint.pth'))['domain_mins'], leaves['domain_mins'])
    # the leaves render through KiloNerfMLP exactly as the last cycle's students evaluate
    emb = dict(type='KiloNerfFourierEmbedder', num_networks=1, input_ch=3, multires=10, multires_dirs=4)
    res = [32, 32, 16]                                                                    # fixed resolution [2, 2, 1]
    mlp = kilo.KiloNerfMLP.from_arrays(res, torch.ones(res, dtype=torch.bool).reshape(-1), leaves['domain_mins'], leaves['domain_maxs'],
                                       leaves['state_dict'], emb, leaves['num_hidden_layers']).to(dev)
    rng = np.random.default_rng(0)
    cell = rng.integers(0, 2, (64, 2))
    lo = np.array(want_min, np.float32)[cell[:, 0] * 2 + cell[:, 1]]
    hi = np.array(want_max, np.float32)[cell[:, 0] * 2 + cell[:, 1]]
    pts = (lo + (hi - lo) * (0.05 + 0.9 * rng.random((64, 3)))).astype(np.float32)
    dirs = rng.normal(size=(64, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    with torch.no_grad():
        raw = mlp({'pts': torch.from_numpy(pts).to(dev)[:, None], 'viewdirs': torch.from_numpy(dirs).to(dev),
                   'global_domain_min': torch.tensor(GMIN), 'global_domain_max': torch.tensor(GMAX)})['raw'].reshape(64, 4)
        students = rec.models[60].multi_network
        ex = torch.from_numpy(np.concatenate([pts, dirs], 1)).to(dev)[None].expand(4, 64, 6).contiguous()
        every = KD.student_forward(ex, students.multi_network.packed(), *students.arch, domain_mins=leaves['domain_mins'].to(dev),
                                   domain_maxs=leaves['domain_maxs'].to(dev))
    own = every[torch.from_numpy(cell[:, 0] * 2 + cell[:, 1]).to(dev), torch.arange(64, device=dev)]
    worst = (raw - own).abs().max().item()
    print('KiloNerfMLP against the students: worst |difference| %g, largest |raw| %g' % (worst, own.abs().max().item()))
    assert worst <= 1e-5 * max(1.0, own.abs().max().item())     # test_gpu_kilo_distill.py's bound for student_forward, per unit of raw


def check_equal_error_threshold(dev, work):
    from xrnerf_amd import ops
    cfg = distill_cfg(work, tree_type='kdtree_equal_error_split', max_tree_cycles=2, max_iters=10, val_examples=300)
    runner, cp, rec = run(cfg, dev)
    assert runner.iter == 20 and cp['num_networks_fitted'] == 2
    root = cp['root_nodes'][0]
    o = rec.outputs[10]
    table, _ = ops.kilo_val_metrics(o['out'], o['target_s'], int(300 * 0.99), points=o['test_points'], split_axis=[0], split_metric='mse')
    want = table[0, ops.KT_THRESHOLD].item()
    assert int(root.split_axis) == 0 and GMIN[0] < want < GMAX[0]
    assert np.float32(root.split_threshold) == np.float32(want) and not math.isnan(want)
    assert root.leq_child.domain_max[0] == root.split_threshold and root.gt_child.domain_min[0] == root.split_threshold
    assert math.isclose(cp['fitted_volume'], cp['total_volume'], rel_tol=1e-6)


def check_fixed_forest(dev, work):
    """max_error = 100000, the shipped configs' path: nobody splits, one cycle per max_num_networks nodes"""
    cfg = distill_cfg(work, max_error=100000, max_num_networks=2, max_iters=4, val_examples=64, fixed_resolution=[3, 1, 1])
    cfg['total_num_networks'] = 3                                                         # kilo_replace
    runner, cp, rec = run(cfg, dev)
    assert runner.iter == 8 and runner._max_iters == 8 and [rec.outputs[i]['out'].shape[0] for i in (4, 8)] == [2, 1]
    assert len(cp['root_nodes']) == 3 and all(hasattr(n, 'network') and not hasattr(n, 'leq_child') for n in cp['root_nodes'])
    assert cp['num_networks_fitted'] == 3 and math.isclose(cp['fitted_volume'], cp['total_volume'], rel_tol=1e-6)


def test_three_cycles_grow_the_longest_axis_tree(dev, tmp_path):
    check_longest_axis_tree(dev, str(tmp_path))


def test_equal_error_split_threshold_is_the_kernels(dev, tmp_path):
    check_equal_error_threshold(dev, str(tmp_path))


def test_max_error_of_the_shipped_configs_keeps_the_fixed_forest(dev, tmp_path):
    check_fixed_forest(dev, str(tmp_path))
