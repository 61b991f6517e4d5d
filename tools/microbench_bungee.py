"""BungeeNeRF microbenchmark at the config's sizes (2048 rays, 65 coarse + 65 fine edges, netwidth 256) for cur_stage 0..3:
ms per train_step (at stage = cur_stage) and per train_iteration (the runner's stage loop over a batch with scale codes 0..cur_stage),
fused path (xrnerf_amd.bungee) against the composed-torch restatement (tests/bungee_restatement.py, fp32, same GPU); per-kernel us of
xr_bungee_zvals / _encode / _render_forward / _backward; ms per 800 x 800 validation frame.  One JSON line per cur_stage."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--stages', default='0,1,2,3')
    ap.add_argument('--frame', type=int, default=800)
    a = ap.parse_args()
    import bungee_restatement as RS
    import xrnerf_amd
    from xrnerf_amd import bungee, ops
    dev = torch.device('cuda')
    cfg = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'bungee_model_cfg.json')))
    sc = bungee.synthetic_city(H=64, W=80, n_per_scale=4, n_scales=4, seed=0)
    R, NZ = cfg['N_rand_per_sampler'], cfg['N_samples']
    for cs in [int(s) for s in a.stages.split(',')]:
        torch.manual_seed(0)
        first = sc['scale_split'][cs]                      # load.py keeps the images from scale_split[cur_stage] on
        table = bungee.BungeeRayTable(sc['H'], sc['W'], sc['focal'], sc['poses'][first:], sc['images'][first:], sc['scale_split'], cs,
                                      device=dev)
        b = bungee.bungee_zvals(table.batch(0, R), NZ, 'sphere', sc['scene_origin'], sc['scene_scale'])
        model = dict(cfg['model'])
        model['mlp'] = dict(model['mlp'], cur_stage=cs)
        net = xrnerf_amd.build_network(model).to(dev)
        ref = RS.RestatedNetwork(cs, 256, 0.01, NZ).to(dev)
        ref.mlp.load_state_dict({k[4:]: v for k, v in net.state_dict().items() if k.startswith('mlp.')})
        opt_f = torch.optim.Adam(net.parameters(), lr=5e-4)
        opt_r = torch.optim.Adam(ref.parameters(), lr=5e-4)
        lb = {k: v[None] for k, v in b.items()}
        rand = torch.rand((R, NZ), device=dev)

        def step_f():
            o = net.train_step(dict(lb), opt_f, stage=cs, rand=rand)
            opt_f.zero_grad()
            o['loss'].backward()

        def step_r():
            loss = ref.train_step(b, cs, rand)
            loss.item()
            opt_r.zero_grad()
            loss.backward()

        out = {'cur_stage': cs, 'rays': R, 'edges': NZ, 'netwidth': 256,
               'train_step_ms': {'fused': timed(step_f, a.reps), 'restatement': timed(step_r, a.reps)},
               'train_iteration_ms': {'fused': timed(lambda: bungee.train_iteration(net, lb, opt_f), a.reps),
                                      'restatement': timed(lambda: RS.train_iteration(ref, b, opt_r), a.reps)},
               'stages_in_batch': int(b['scale_code'].max()) + 1}
        k = {}
        k['zvals'] = 1e3 * timed(lambda: ops.bungee_zvals(b['rays_o'], b['viewdirs'], None, None, NZ, 'sphere', sc['scene_origin'],
                                                          sc['scene_scale']), a.reps)
        k['encode'] = 1e3 * timed(lambda: ops.bungee_encode(b['viewdirs'], 10, 4, frustum=(b['rays_o'], b['rays_d'], b['radii'],
                                                                                          b['z_vals'])), a.reps)
        raw = torch.randn(R, NZ - 1, cs + 1, 4, device=dev)
        g = torch.randn(R, 3, device=dev)
        k['render_forward'] = 1e3 * timed(lambda: ops.bungee_render_forward(raw, b['z_vals'], b['viewdirs'], cs), a.reps)
        k['render_backward'] = 1e3 * timed(lambda: ops.bungee_render_backward(raw, b['z_vals'], b['viewdirs'], g, cs), a.reps)
        out['kernel_us'] = k
        if a.frame:
            F = a.frame
            K = [[sc['focal'] * F / sc['W'], 0, 0.5 * F], [0, sc['focal'] * F / sc['W'], 0.5 * F], [0, 0, 1]]
            net.set_val_pipeline(bungee.make_val_pipeline(F, F, K, NZ, 'sphere', sc['scene_origin'], sc['scene_scale']))
            net.render.stage = cs
            pose = torch.tensor(sc['poses'][0], dtype=torch.float32, device=dev)
            ms = timed(lambda: net._render_pose(pose), 2, warmup=1)
            out['val_frame_ms'] = ms
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
