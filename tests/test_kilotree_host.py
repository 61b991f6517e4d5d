"""The host side of KiloNeRF's discovery loop (xrnerf_amd/kilo_tree.py) on the CPU: the tree bookkeeping replayed on the reference's own
per-network numbers (tests/golden/ref_kilotree_hook.json, made by tests/golden/make_golden_kilotree.py from the scripts of
tests/kilotree_scenarios.py) reproduces every queue, box, volume and log line; OccupationHook, kilo_replace, DistllCycleHook's iteration
arithmetic, the leaf order of leaves_to_checkpoint and the checkpoint round trip of get_single_network."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import kilotree_scenarios as S  # noqa: E402
from xrnerf_amd import kilo, kilo_distill, kilo_tree as T  # noqa: E402
from xrnerf_amd.builder import ConfigDict  # noqa: E402
from xrnerf_amd.kilodata import Node, calculate_volume  # noqa: E402

with open(os.path.join(ROOT, 'tests', 'golden', 'ref_kilotree_hook.json')) as _f:
    GOLD = json.load(_f)


def boxes(nodes):
    return [[[float(v) for v in n.domain_min], [float(v) for v in n.domain_max]] for n in nodes]


def fake_runner(work, max_iters):
    runner = types.SimpleNamespace(iter=0, _max_iters=max_iters, work_dir=str(work), outputs=None, logged=[])
    runner.logger = types.SimpleNamespace(info=lambda *a: runner.logged.append(a[0] % a[1:] if len(a) > 1 else a[0]))
    runner.model = types.SimpleNamespace(multi_network=types.SimpleNamespace(get_single_network=lambda i: int(i)))
    return runner


@pytest.mark.parametrize('run', GOLD['runs'], ids=[r['name'] for r in GOLD['runs']])
def test_bookkeeping_reproduces_the_reference(run, tmp_path):
    sc = [s for s in S.SCENARIOS if s['name'] == run['name']][0]
    cfg = ConfigDict.wrap(dict(sc['cfg']))
    cp = S.new_cp(sc, Node, calculate_volume)
    assert cp['total_volume'] == run['total_volume']
    runner = fake_runner(tmp_path, S.initial_max_iters(sc))
    if 'numpy_seed' in sc:
        np.random.seed(sc['numpy_seed'])
    cycle, hook, batch = -1, None, None
    for step in run['steps']:
        if step['cycle'] != cycle:
            cycle = step['cycle']
            saturated = not cp['nodes_to_process']
            queue = cp['saturated_nodes_to_process'] if saturated else cp['nodes_to_process']
            batch = [queue.popleft() for _ in range(min(sc['max_num_networks'], len(queue)))]
            cfg['num_networks'] = len(batch)
            info = {'cp': cp, 'processing_saturated_nodes': saturated, 'node_batch': batch}
            hook = T.SaveDistillResultsHook(cfg, types.SimpleNamespace(get_info=lambda info=info: info))
            runner.iter = cycle * cfg.max_iters
            hook.before_train_iter(runner)
            assert saturated == step['processing_saturated_nodes']
        runner.iter = step['iter']
        runner.outputs = {'error_log': list(step['error_log_in'])}
        hook.after_val_table(runner, torch.tensor(step['table'], dtype=torch.float32))
        what = '%s iteration %d' % (run['name'], step['iter'])
        assert hook.error_log == step['error_log_out'], what
        assert boxes(cp['nodes_to_process']) == step['nodes_to_process'], what
        assert boxes(cp['saturated_nodes_to_process']) == step['saturated_nodes_to_process'], what
        assert float(cp['fitted_volume']) == step['fitted_volume'] and cp['num_networks_fitted'] == step['num_networks_fitted'], what
        assert runner._max_iters == step['max_iters'], what
        for node, want in zip(batch, step['node_batch']):
            assert hasattr(node, 'network') == want['fitted'], what
            if want['fitted']:
                assert node.network == want['network'] and set(node.discovery_best_error) == set(T.METRICS)
            if want['children'] is not None:
                assert int(node.split_axis) == want['split_axis'] and float(node.split_threshold) == want['split_threshold'], what
                assert boxes([node.leq_child, node.gt_child]) == want['children'], what
            else:
                assert not hasattr(node, 'leq_child'), what
    assert not cp['nodes_to_process'] and not cp['saturated_nodes_to_process']
    if GOLD['numpy'].split('.')[0] == np.__version__.split('.')[0]:      # a numpy scalar in a printed box prints as its numpy prints it
        assert open(os.path.join(str(tmp_path), 'log.txt')).read() == run['log_txt']
    cp2 = torch.load(os.path.join(str(tmp_path), 'checkpoint.pth'), weights_only=False)
    assert cp2['num_networks_fitted'] == cp['num_networks_fitted'] and len(cp2['root_nodes']) == len(cp['root_nodes'])
    assert any('num networks below threshold' in line for line in runner.logged)


def test_max_tree_cycles_fits_every_node_in_flight(tmp_path):
    """the one extension: with max_error out of reach the reference never ends; max_tree_cycles = 2 records the second cycle's nodes"""
    sc = S.SCENARIOS[0]
    cfg = ConfigDict.wrap(dict(sc['cfg'], max_error=0, max_tree_cycles=2))
    cp = S.new_cp(sc, Node, calculate_volume)
    best = T.new_best_errors(2)
    for d in best:
        for m in d:
            d[m] = torch.ones(2)
    root = cp['nodes_to_process'].popleft()
    assert T.process_node_batch(cfg, cp, [root], False, *[{m: v[:1] for m, v in d.items()} for d in best], torch.zeros(1, dtype=torch.bool), cycles_run=1) == 0
    batch = [cp['nodes_to_process'].popleft() for _ in range(2)]
    assert T.process_node_batch(cfg, cp, batch, False, *best, torch.zeros(2, dtype=torch.bool), cycles_run=2) == 2
    assert not cp['nodes_to_process'] and cp['num_networks_fitted'] == 2 and cp['fitted_volume'] == pytest.approx(cp['total_volume'])


def test_a_missing_threshold_names_the_network():
    sc = S.SCENARIOS[2]
    cfg = ConfigDict.wrap(dict(sc['cfg']))
    cp = S.new_cp(sc, Node, calculate_volume)
    best = T.new_best_errors(1)
    with pytest.raises(ValueError, match='network 0'):
        T.process_node_batch(cfg, cp, [cp['root_nodes'][0]], False, *best, torch.zeros(1, dtype=torch.bool), thresholds=np.array([np.nan], np.float32))


def test_occupation_hook(tmp_path):
    runner = types.SimpleNamespace(work_dir=str(tmp_path))
    hook = T.OccupationHook()
    hook.after_train_iter(runner)
    flag = os.path.join(str(tmp_path), 'delete_me_to_stop')
    assert os.path.isdir(flag)
    hook.after_val_iter(runner)                  # still there: goes on
    os.rmdir(flag)
    with pytest.raises(SystemExit) as e:
        hook.after_train_iter(runner)
    assert e.value.code == 0


def test_kilo_replace():
    def cfg(phase):
        return ConfigDict.wrap(dict(phase=phase, resolution_table=dict(Lego=[9, 16, 10]), build_occupancy_tree_config=dict(),
                                    data=dict(train=dict(cfg=dict()), val=dict(cfg=dict())), model=dict(mlp=dict())))
    c = T.kilo_replace('Lego', cfg('distill'))
    assert c.fix_resolution == [9, 16, 10] and c.total_num_networks == 1440
    assert c.data['train'].cfg['fixed_resolution'] == [9, 16, 10] and c.data['val'].cfg['fixed_resolution'] == [9, 16, 10]
    assert T.kilo_replace('Lego', cfg('pretrain')).build_occupancy_tree_config['resolution'] == [9, 16, 10]
    assert T.kilo_replace('Lego', cfg('finetune')).model['mlp']['resolution'] == [9, 16, 10]


@pytest.mark.parametrize('total,most,cycles', [(1440, 512, 3), (1024, 512, 2), (1, 4, 1), (512, 512, 1), (513, 512, 2)])
def test_distill_cycle_hook_iteration_budget(total, most, cycles):
    runner = types.SimpleNamespace(_max_iters=None)
    T.DistllCycleHook(ConfigDict.wrap(dict(total_num_networks=total, max_num_networks=most, max_iters=150))).before_run(runner)
    assert runner._max_iters == cycles * 150


def test_distill_cycle_hook_refuses_distributed():
    hook = T.DistllCycleHook(ConfigDict.wrap(dict(distributed=True, max_iters=10)))
    with pytest.raises(NotImplementedError):
        hook._update_train_distill_cyle(types.SimpleNamespace(model=None), 1)


def student(n):
    kilo_distill.MultiNetworkLinear.rng_state = None
    return kilo_distill._default_student(n, 8078673, 10, 4, 2)


def small_tree():
    """root -> (a, b); a -> (a0, a1): breadth-first leaves are b, a0, a1"""
    def node(lo, hi):
        n = Node()
        n.domain_min, n.domain_max = lo, hi
        return n
    root, a, b = node([0., 0., 0.], [2., 1., 1.]), node([0., 0., 0.], [1., 1., 1.]), node([1., 0., 0.], [2., 1., 1.])
    a0, a1 = node([0., 0., 0.], [1., .5, 1.]), node([0., .5, 0.], [1., 1., 1.])
    root.leq_child, root.gt_child, a.leq_child, a.gt_child = a, b, a0, a1
    return root, (b, a0, a1)


def test_leaves_to_checkpoint_is_breadth_first():
    mn = student(3)
    with torch.no_grad():
        for i, p in enumerate(mn.multi_network.parameters()):
            p.copy_(torch.arange(p.shape[0], dtype=torch.float32).reshape([-1] + [1] * (p.dim() - 1)).expand_as(p) + 0.01 * i)
    root, leaves = small_tree()
    for i, leaf in enumerate(leaves):
        leaf.network = mn.get_single_network(2 - i)            # network 2 at the first leaf
    cp = T.leaves_to_checkpoint({'root_nodes': [root]})
    assert cp['domain_mins'].tolist() == [l.domain_min for l in leaves] and cp['domain_maxs'].tolist() == [l.domain_max for l in leaves]
    assert cp['num_hidden_layers'] == 2 and cp['state_dict']['pts_linears.0.weight'].shape == (3, 63, 32)
    assert cp['state_dict']['rgb_linear.bias'][:, 0].floor().tolist() == [2., 1., 0.]


def test_single_networks_round_trip_through_the_checkpoint_reader(tmp_path):
    mn = student(2)
    with torch.no_grad():
        for p in mn.parameters():
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())))
    before = torch.random.get_rng_state()
    singles = [mn.get_single_network(i) for i in range(2)]
    assert torch.equal(torch.random.get_rng_state(), before)    # the copies' own initial draw leaves the caller's stream alone
    assert singles[1].pts_linears[0].weight.shape == (1, 32, 63) and singles[0].num_hidden_layers == 2
    root = Node()
    root.domain_min, root.domain_max, root.split_axis, root.split_threshold = [0., 0., 0.], [2., 1., 1.], 0, 1.0
    root.leq_child, root.gt_child = Node(), Node()
    root.leq_child.domain_min, root.leq_child.domain_max, root.leq_child.network = [0., 0., 0.], [1., 1., 1.], singles[0]
    root.gt_child.domain_min, root.gt_child.domain_max, root.gt_child.network = [1., 0., 0.], [2., 1., 1.], singles[1]
    path = os.path.join(str(tmp_path), 'checkpoint.pth')
    torch.save({'root_nodes': [root], 'fitted_volume': 2.0, 'num_networks_fitted': 2}, path)
    cp = kilo.load_reference_distilled_checkpoint(path)
    assert cp['domain_mins'].tolist() == [[0., 0., 0.], [1., 0., 0.]] and cp['num_hidden_layers'] == 2
    m = mn.multi_network
    for name, layer in (('pts_linears.0', m.pts_linears[0]), ('pts_linears.1', m.pts_linears[1]), ('alpha_linear', m.alpha_linear),
                        ('feature_linear', m.feature_linear), ('direction_layer', m.direction_layer), ('rgb_linear', m.rgb_linear)):
        assert torch.equal(cp['state_dict'][name + '.weight'], layer.weight.detach().transpose(1, 2)), name
        assert torch.equal(cp['state_dict'][name + '.bias'], layer.bias.detach()), name
    emb = dict(type='KiloNerfFourierEmbedder', num_networks=1, input_ch=3, multires=10, multires_dirs=4)
    mlp = kilo.KiloNerfMLP(resolution=[2, 1, 1], distilled_checkpoint=path, embedder=emb, trust_pickle=True)
    assert mlp is not None
