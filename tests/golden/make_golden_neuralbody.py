"""Generates tests/golden/ref_neuralbody.npz from the REFERENCE'S OWN NeuralBody code (configs/neuralbody/nb_zjumocap_313.py), in the
build container only:  python tests/golden/make_golden_neuralbody.py

Imported unmodified through tests/golden/ref_import.py::load_mip() plus the leaf modules models/embedders/neuralbody_embedder.py,
models/mlps/nb_mlp.py and models/networks/neuralbody.py; NerfRender is the reference's.

`spconv` (external, no ROCm build, absent here) is STUBBED by the dense restatement of tests/neuralbody_restatement.py: a masked
conv3d, max_pool3d of the mask for the strided step's active set, rows in ascending linear index, vertices of one voxel merged by
summing their latent codes -- the semantics DESIGN.md section 13 fixes ("unpinned against spconv").

Parameters are neuralbody_restatement.formula_tensor(key, shape, SEED), not stored.  One training step (SmplEmbedder.forward,
NB_NeRFMLP.forward, NerfRender.forward, img2mse, backward) on xrnerf_amd.neuralbody.synthetic_frame(6890, 5), 32 rays x 16 samples, at
VOXEL = 0.04 (an out_sh of a few tens of cells per axis); it runs twice, in float32 and in float64.  Expected values are the float64
run's; for every compared quantity the fixture also keeps the deviation of the float32 run from it (`dev.*`, relative to the
quantity's max |value|; for a gradient's sampled entries relative to `gmax.*`, the largest entry of the whole tensor), which is what the tests' bars are made of.

Voxel decisions are made unambiguous, and that is asserted: a vertex whose voxel coordinate is within 1e-3 of a rounding boundary in the
float64 run is moved by a quarter voxel; both runs must agree on every coordinate.  The share of post-batch-norm elements within 2^-20
of zero (ReLU kinks) is recorded per layer and asserted to be under 2 %."""
import copy
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402
import neuralbody_restatement as RS  # noqa: E402

SEED = 13
V, N_RAYS, N_S, VOXEL = 6890, 32, 16, 0.04
MARGIN = 1e-3
# what a NeuralBody step reads of synthetic_frame's `datas` (the skinning weights and matrices of the synthetic body are not stored)
IN_KEYS = ('pts', 'rays_o', 'rays_d', 'z_vals', 'near', 'far', 'target_s', 'smpl_verts', 'smpl_R', 'smpl_T', 'latent_idx')


def load_ref():
    ns = ref_import.load_mip()
    top, sub = RS.spconv_stand_in()
    sys.modules['spconv'], sys.modules['spconv.pytorch'] = top, sub
    utils = sys.modules['xrnerf.models.networks.utils']
    tr = importlib.import_module('xrnerf.models.networks.utils.transforms')
    utils.nb_recover_shape = tr.nb_recover_shape
    utils.__all__ = [n for n in vars(utils) if not n.startswith('_')]
    ns.emb = importlib.import_module('xrnerf.models.embedders.neuralbody_embedder')
    ns.mlp = importlib.import_module('xrnerf.models.mlps.nb_mlp')
    ns.NeuralBodyNetwork = importlib.import_module('xrnerf.models.networks.neuralbody').NeuralBodyNetwork
    return ns


def to_cfg(d):
    return ref_import.Cfg({k: to_cfg(v) for k, v in d.items()}) if isinstance(d, dict) else d


def cast(datas, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in datas.items()}


def step_lines(ns, net, datas, voxel):
    """NeuralBodyNetwork.forward + the img2mse loss, line by line; the batch norms' outputs are recorded"""
    bn_out = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: bn_out.append(out.detach()))
             for m in net.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    try:
        net.train()
        sp = ns.emb.prepare_sparseconv_data(datas, voxel)
        xyzc = net.smpl_conv(datas)
        datas = net.nerf_mlp(xyzc, datas)
        datas, ret = net.render(datas, False)
        loss = torch.mean((ret['rgb'] - datas['target_s']) ** 2)
    finally:
        for h in hooks:
            h.remove()
    return dict(coord=sp['coord'][:, 1:], out_sh=sp['out_sh'], pts_idx=sp['pts_idx'], features=xyzc[0].t(), raw=datas['raw'], rgb=ret['rgb'],
                loss=loss, bn_out=bn_out)


def rel(a, b):
    """max |a - b| / max |b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def main():
    assert ref_import.available(), 'needs the reference checkout (run in the build container)'
    ns = load_ref()
    from xrnerf_amd.neuralbody import synthetic_frame
    model = json.load(open(os.path.join(HERE, 'neuralbody_model_cfg.json')))['model']
    model['cfg']['smpl_embedder']['voxel_size'] = [VOXEL] * 3
    torch.manual_seed(0)
    net = ns.NeuralBodyNetwork(to_cfg(copy.deepcopy(model['cfg'])), render=model['render'])
    keys = list(net.state_dict().keys())
    shapes = [tuple(v.shape) for v in net.state_dict().values()]
    net.load_state_dict(RS.formula_state_dict(keys, shapes, SEED), strict=True)
    net64 = copy.deepcopy(net).double()
    out = {'seed': np.int64(SEED), 'voxel': np.float64(VOXEL), 'sd_keys': np.array(keys), 'sd_shapes': np.array([json.dumps(s) for s in shapes])}

    datas = synthetic_frame(V, 5, N_RAYS, N_S)
    voxel = [VOXEL] * 3
    # unambiguous voxels: move the vertices that sit on a rounding boundary (float64 run)
    moved = 0
    for _ in range(10):
        d64 = cast(datas, torch.float64)
        canon = torch.matmul(d64['smpl_verts'] - d64['smpl_T'], d64['smpl_R'])
        mn = canon.min(0)[0]
        mn[2] -= 0.05
        frac = (canon - mn) / VOXEL
        bad = ((frac - torch.floor(frac) - 0.5).abs() < MARGIN).any(1)
        # (the vertices that define min_xyz must stay where they are)
        bad &= ~(canon == canon.min(0)[0]).any(1) & ~(canon == canon.max(0)[0]).any(1)
        if not bool(bad.any()):
            break
        moved += int(bad.sum())
        shift = torch.matmul(torch.full((int(bad.sum()), 3), 0.25 * VOXEL, dtype=torch.float64), d64['smpl_R'].t())
        datas['smpl_verts'][bad] = (d64['smpl_verts'][bad] + shift).float()
    else:
        raise AssertionError('the voxel coordinates stay ambiguous')
    print('%d of %d vertices moved off a rounding boundary' % (moved, V))
    assert moved <= 0.05 * V

    ref64 = step_lines(ns, net64, cast(datas, torch.float64), voxel)
    net64.zero_grad()
    ref64['loss'].backward()
    net.zero_grad()
    res = step_lines(ns, net, {k: v.clone() for k, v in datas.items()}, voxel)
    res['loss'].backward()
    assert torch.equal(res['coord'], ref64['coord']) and list(res['out_sh']) == list(ref64['out_sh'])
    out_sh = [int(v) for v in ref64['out_sh']]
    assert len(set(out_sh)) > 1, 'out_sh must not be a cube'
    rows, vert_row = RS.all_rows(ref64['coord'], out_sh)
    print('out_sh %r, rows per level %r, %d distinct voxels of %d vertices' % (out_sh, [int(r.shape[0]) for r in rows], rows[0].shape[0], V))

    for k in IN_KEYS:
        out['in.' + k] = datas[k].numpy()
    out['out_sh'] = np.array(out_sh, np.int32)
    for l in range(RS.LEVELS):
        out['rows.%d' % l] = rows[l].numpy().astype(np.int32)
    f64, f32 = ref64['features'].detach().numpy(), res['features'].detach().numpy()
    out['features'] = f64.astype(np.float32)
    c0 = 0
    for l, c in enumerate(RS.CHANNELS):
        out['dev.features.%d' % (l + 1)] = np.float64(rel(f32[:, c0:c0 + c], f64[:, c0:c0 + c]))
        c0 += c
    for name in ('raw', 'rgb'):
        out[name] = ref64[name].detach().numpy()
        out['dev.' + name] = np.float64(rel(res[name].detach().numpy(), out[name]))
    out['loss'] = np.float64(ref64['loss'].item())
    out['dev.loss'] = np.float64(abs(res['loss'].item() - ref64['loss'].item()) / abs(ref64['loss'].item()))
    # gradients
    p64 = dict(net64.named_parameters())
    for k, p in net.named_parameters():
        assert p.grad is not None and p64[k].grad is not None, k
        g, g64 = p.grad.detach().numpy().reshape(-1), p64[k].grad.detach().numpy().reshape(-1)
        pos = RS.sample_positions(k, g64.size)
        out['gnorm.' + k] = np.float64(np.linalg.norm(g64))
        out['gmax.' + k] = np.float64(np.abs(g64).max())
        out['gsample.' + k] = g64[pos].copy()
        # (for the 2-norm: the relative 2-norm of the whole difference, which bounds | |g32| - |g64| | by the triangle inequality.  The
        # signed difference of the two norms itself is ONE draw of a quantity whose errors cancel -- 3.7e-8 on the latent codes, under
        # one fp32 rounding -- and 4 x such a draw is no bar)
        out['dev.gnorm.' + k] = np.float64(np.linalg.norm(g.astype(np.float64) - g64) / max(np.linalg.norm(g64), 1e-300))
        out['dev.gsample.' + k] = np.float64(np.abs(g[pos] - g64[pos]).max() / max(np.abs(g64).max(), 1e-300))
    # running statistics after the step
    sd, sd64 = net.state_dict(), net64.state_dict()
    for k in keys:
        if k.endswith('running_mean') or k.endswith('running_var'):
            out['stat.' + k] = sd64[k].numpy()
            out['dev.stat.' + k] = np.float64(rel(sd[k].numpy(), sd64[k].numpy()))
    # ReLU kinks
    shares = []
    for y in ref64['bn_out']:
        shares.append(float((y.abs() < 2.0 ** -20 * y.abs().max()).double().mean()))
    out['kink_share'] = np.array(shares)
    assert max(shares) < 0.02, shares
    print('features dev %s, raw %.2e, rgb %.2e, loss %.6g (dev %.2e), worst kink share %.2e' % (
        ['%.2e' % out['dev.features.%d' % l] for l in range(1, 5)], out['dev.raw'], out['dev.rgb'], out['loss'], out['dev.loss'], max(shares)))
    gd = {k[len('dev.gsample.'):]: float(v) for k, v in out.items() if k.startswith('dev.gsample.')}
    worst = max(gd, key=gd.get)
    print('gradient dev: latent codes %.2e, worst %s %.2e' % (gd['smpl_conv.latent_codes.weight'], worst, gd[worst]))
    path = os.path.join(HERE, 'ref_neuralbody.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
