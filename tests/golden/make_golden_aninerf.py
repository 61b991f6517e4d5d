"""Generates tests/golden/ref_aninerf.npz from the REFERENCE'S OWN Animatable-NeRF code
(configs/animatable_nerf/an_h36m_s9_train_pose.py), in the build container only:  python tests/golden/make_golden_aninerf.py

Imported unmodified through tests/golden/ref_import.py::load_mip() plus the leaf modules models/networks/utils/aninerf.py,
models/mlps/aninerf_mlp.py, models/networks/neuralbody.py and models/networks/aninerf.py; NerfRender is the reference's.

`pytorch3d.ops.knn.knn_points` (external, absent here; the reference's only use is K = 1) is STUBBED by its float32 restatement:
d2 = (dx dx + dy dy) + dz dz per pair, the smallest d2 and the first index that has it (tests/aninerf_restatement.py d2_matrix) --
as the KiloNeRF fixture stands in for `kilonerf_cuda`.  The stub also records every query's float64 margins.

Parameters: 2 M of them (the AN_* widths are hard-wired to 256), so none is stored: every state-dict entry is
aninerf_restatement.formula_tensor(key, shape, SEED), which the tests evaluate too.  Per parameter tensor the fixture keeps the
2-norm of its gradient and its entries at aninerf_restatement.sample_positions(key, numel).

  train_pose step   32 rays x 16 samples of xrnerf_amd.aninerf.synthetic_body(257, 5): DeformField.forward, TPoseHuman.forward,
                    filter_and_format_prediction, NerfRender.forward, img2mse + smooth_l1_loss (the lines of AniNeRFNetwork.forward /
                    train_pose_stage, taken one by one so that pind, tpose, tpose_dirs, pbw, tbw, raw and rgb can be stored)
  novel_pose step   NovelPoseTraining.calculate_bounds / wpts_to_ppts / ppts_to_tpose / tpose_to_ppts and the two smooth_l1 losses
                    on 512 + 512 stored uniform draws: calculate_loss itself draws 3 x 65 536 numbers per space inside
                    get_sampling_points, whose one line ((max - min) * vals + min) is applied here to the stored draws

Discrete decisions are made unambiguous, and that is asserted: a query (a ray sample, or a draw) is replaced by a fresh one when, in
the reference's own float64 run, a nearest-vertex d2 gap is below 1e-5, |dist - threshold| < 1e-5, a canonical-bounds margin is below
1e-5 or |alpha| < 1e-4.  More than 5 % replaced queries is a failure.
"""
import copy
import importlib
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402
import aninerf_restatement as RS  # noqa: E402

SEED = 11
V, N_RAYS, N_S, N_DRAWS = 257, 32, 16, 512
GAP, TH_MARGIN, BOUND_MARGIN, ALPHA_MARGIN = 1e-5, 1e-5, 1e-5, 1e-4
QUERIES = []            # one record per knn_points call of the current run


def knn_points(src, ref, K=1):
    assert K == 1 and src.shape[0] == 1 and ref.shape[0] == 1
    dd = RS.d2_matrix(src[0], ref[0])
    m = dd.min(1)[0]
    idx = (dd == m[:, None]).to(torch.uint8).argmax(1)
    s = torch.sort(dd.detach().double(), dim=1)[0]
    QUERIES.append({'gap': (s[:, 1] - s[:, 0]).numpy(), 'dist': s[:, 0].sqrt().numpy(), 'idx': idx.numpy()})
    return types.SimpleNamespace(dists=m[None, :, None], idx=idx[None, :, None])


def load_ref():
    ns = ref_import.load_mip()
    for name in ('pytorch3d', 'pytorch3d.ops', 'pytorch3d.ops.knn'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['pytorch3d.ops.knn'].knn_points = knn_points
    utils = sys.modules['xrnerf.models.networks.utils']
    ani = importlib.import_module('xrnerf.models.networks.utils.aninerf')
    tr = importlib.import_module('xrnerf.models.networks.utils.transforms')
    for mod, names in ((ani, [n for n in vars(ani) if not n.startswith('_') and n not in ('np', 'torch', 'F')]), (tr, ['nb_recover_shape'])):
        for n in names:
            setattr(utils, n, getattr(mod, n))
    utils.__all__ = [n for n in vars(utils) if not n.startswith('_')]
    ns.ani = ani
    ns.mlp = importlib.import_module('xrnerf.models.mlps.aninerf_mlp')
    importlib.import_module('xrnerf.models.networks.neuralbody')
    ns.AniNeRFNetwork = importlib.import_module('xrnerf.models.networks.aninerf').AniNeRFNetwork
    return ns


def to_cfg(d):
    return ref_import.Cfg({k: to_cfg(v) for k, v in d.items()}) if isinstance(d, dict) else d


def cast(datas, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in datas.items()}


def train_pose_lines(net, datas):
    """AniNeRFNetwork.forward + train_pose_stage, line by line"""
    deform_ret = net.deform_field(datas)
    raw = net.tpose_human(deform_ret, datas)
    alpha_before = raw[:, 3].detach().clone()
    datas, tpose_ret = net.tpose_human.filter_and_format_prediction(raw, deform_ret, datas)
    datas, ret = net.render(datas, False)
    img_loss = torch.mean((ret['rgb'] - datas['target_s']) ** 2)
    bw_loss = F.smooth_l1_loss(tpose_ret['pbw'], tpose_ret['tbw'])
    alpha = raw[:, 3].detach()
    chosen = alpha > 0
    chosen[alpha.argmax()] = True
    return dict(deform=deform_ret, raw=datas['raw'], rgb=ret['rgb'], img_loss=img_loss, bw_loss=bw_loss, chosen=chosen,
                alpha_before=alpha_before)


def bound_margin(tpose, verts):
    lo, hi = verts.min(0)[0] - 0.05, verts.max(0)[0] + 0.05
    return torch.minimum((tpose - lo).abs(), (tpose - hi).abs()).min(1)[0].detach().numpy()


def train_pose_failures(net64, datas, th):
    """indices into the [R*S] samples whose decisions are within the margins, in the float64 run"""
    QUERIES.clear()
    out = train_pose_lines(net64, cast(datas, torch.float64))
    q_all, q_sel, q_canon = QUERIES[0], QUERIES[1], QUERIES[2]
    pind = out['deform']['pind'][0].numpy()
    sel = np.flatnonzero(pind)
    bad = np.zeros(pind.shape, bool)
    bad |= np.abs(q_all['dist'] - th) < TH_MARGIN
    bad[sel] |= q_sel['gap'] < GAP
    bad[sel] |= q_canon['gap'] < GAP
    inside_margin = bound_margin(out['deform']['tpose'], datas['canonical_smpl_verts'].double())
    bad[sel] |= inside_margin < BOUND_MARGIN
    bad[sel] |= np.abs(out['alpha_before'].numpy()) < ALPHA_MARGIN
    return np.flatnonzero(bad), out


def sampled_grads(net, prefix, out):
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach().numpy().reshape(-1)
        out[prefix + 'gnorm.' + k] = np.float64(np.linalg.norm(g.astype(np.float64)))
        out[prefix + 'gsample.' + k] = g[RS.sample_positions(k, g.size)].copy()


def novel_lines(ns, net, datas, draws):
    """NovelPoseTraining.calculate_loss with get_sampling_points' line applied to the stored draws; the calculate_alpha calls are
    recorded (tpose and alpha of both directions)"""
    NP = ns.ani.NovelPoseTraining
    rec = []
    orig = net.tpose_human.calculate_alpha

    def recording(tpose):
        a = orig(tpose)
        rec.append((tpose[0].detach().clone(), a[0, 0].detach().clone()))
        return a
    net.tpose_human.calculate_alpha = recording
    try:
        world_bounds = NP.calculate_bounds(datas['smpl_verts'])
        canonical_bounds = NP.calculate_bounds(datas['canonical_smpl_verts'])
        pts = lambda b, vals: (b[:, 1] - b[:, 0])[:, None] * vals + b[:, 0][:, None]
        world_points = pts(world_bounds, draws[0].to(world_bounds.dtype))
        posed_points = NP.wpts_to_ppts(world_points, datas)
        canonical_points = pts(canonical_bounds, draws[1].to(world_bounds.dtype))
        pbw0, tbw0 = NP.ppts_to_tpose(net, posed_points, datas, canonical_bounds)
        pbw1, tbw1 = NP.tpose_to_ppts(net, canonical_points, datas)
    finally:
        del net.tpose_human.calculate_alpha
    l0, l1 = F.smooth_l1_loss(pbw0, tbw0), F.smooth_l1_loss(pbw1, tbw1)
    return dict(pbw0=pbw0, tbw0=tbw0, pbw1=pbw1, tbw1=tbw1, loss0=l0, loss1=l1, rec=rec)


def novel_failures(ns, net64, datas, draws, th):
    QUERIES.clear()
    out = novel_lines(ns, net64, cast(datas, torch.float64), draws)
    q0p, q0t, q1t, q1p = QUERIES                   # ppts_to_tpose: posed, canonical; tpose_to_ppts: canonical, posed
    (tpose0, alpha0), (tpose1, alpha1) = out['rec']
    verts = datas['canonical_smpl_verts'].double()
    bad0 = (q0p['gap'] < GAP) | (np.abs(q0p['dist'] - th) < TH_MARGIN) | (q0t['gap'] < GAP) | (bound_margin(tpose0, verts) < BOUND_MARGIN)
    live0 = (q0p['dist'] < th) & (bound_margin(tpose0, verts) >= BOUND_MARGIN)
    bad0 |= live0 & (np.abs(alpha0.numpy()) < ALPHA_MARGIN)
    bad1 = (q1t['gap'] < GAP) | (np.abs(q1t['dist'] - th) < TH_MARGIN) | (q1p['gap'] < GAP)
    bad1 |= (q1t['dist'] <= th) & (np.abs(alpha1.numpy()) < ALPHA_MARGIN)
    return np.flatnonzero(bad0), np.flatnonzero(bad1), out


def main():
    assert ref_import.available(), 'needs /root/reference (run in the build container)'
    ns = load_ref()
    from xrnerf_amd.aninerf import synthetic_body
    model = json.load(open(os.path.join(HERE, 'aninerf_model_cfg.json')))['model']
    th = model['cfg']['deform_field']['smpl_threshold']
    torch.manual_seed(0)
    net = ns.AniNeRFNetwork(to_cfg(copy.deepcopy(model['cfg'])), render=model['render'])
    keys = list(net.state_dict().keys())
    shapes = [tuple(v.shape) for v in net.state_dict().values()]
    net.load_state_dict(RS.formula_state_dict(keys, shapes, SEED), strict=True)
    net64 = ns.AniNeRFNetwork(to_cfg(copy.deepcopy(model['cfg'])), render=model['render'])        # (weight norm does not deep-copy)
    net64.load_state_dict(RS.formula_state_dict(keys, shapes, SEED), strict=True)
    net64 = net64.double()
    out = {'seed': np.int64(SEED), 'sd_keys': np.array(keys), 'sd_shapes': np.array([json.dumps(s) for s in shapes])}
    rng = np.random.default_rng(SEED)

    # ------------------------------------------------------------------ train_pose
    datas = synthetic_body(V, 5, N_RAYS, N_S)
    replaced = set()
    for _ in range(20):
        bad, _ = train_pose_failures(net64, datas, th)
        if not bad.size:
            break
        replaced |= set(bad.tolist())
        z = datas['z_vals'].numpy().copy()
        for i in bad:
            r, s = divmod(int(i), N_S)
            lo = 0.5 * (z[r, s - 1] + z[r, s]) if s > 0 else z[r, s] - 0.02
            hi = 0.5 * (z[r, s] + z[r, s + 1]) if s + 1 < N_S else z[r, s] + 0.02
            z[r, s] = rng.uniform(lo, hi)
        datas['z_vals'] = torch.as_tensor(z)
        datas['pts'] = datas['rays_o'][:, None, :] + datas['rays_d'][:, None, :] * datas['z_vals'][..., None]
    else:
        raise AssertionError('the train_pose queries stay ambiguous')
    print('train_pose: %d of %d queries replaced' % (len(replaced), N_RAYS * N_S))
    assert len(replaced) <= 0.05 * N_RAYS * N_S
    _, ref64 = train_pose_failures(net64, datas, th)
    q64 = list(QUERIES)
    net.get_params()
    net.zero_grad()
    QUERIES.clear()
    res = train_pose_lines(net, {k: v.clone() for k, v in datas.items()})
    (res['img_loss'] + res['bw_loss']).backward()
    d, d64 = res['deform'], ref64['deform']
    assert torch.equal(d['pind'], d64['pind']) and torch.equal(res['chosen'], ref64['chosen'])
    assert len(QUERIES) == 3 and all(np.array_equal(a['idx'], b['idx']) for a, b in zip(QUERIES[1:], q64[1:]))
    for k in datas:
        out['tp_in.' + k] = datas[k].numpy()
    out.update({'tp.pind': d['pind'][0].numpy(), 'tp.tpose': d['tpose'].detach().numpy(), 'tp.tpose_dirs': d['tpose_dirs'].detach().numpy(),
                'tp.pbw': d['pbw'][0].t().detach().numpy(), 'tp.tbw': d['tbw'][0].t().detach().numpy(), 'tp.raw': res['raw'].detach().numpy(),
                'tp.rgb': res['rgb'].detach().numpy(), 'tp.chosen': res['chosen'].numpy(), 'tp.img_loss': np.float64(res['img_loss'].item()),
                'tp.bw_loss': np.float64(res['bw_loss'].item()), 'tp.idx_posed': QUERIES[1]['idx'], 'tp.idx_canonical': QUERIES[2]['idx']})
    sampled_grads(net, 'tp.', out)
    print('train_pose: %d of %d samples near the body, %d rows chosen, img loss %.6g, bw loss %.6g' % (
        int(d['pind'].sum()), N_RAYS * N_S, int(res['chosen'].sum()), out['tp.img_loss'], out['tp.bw_loss']))

    # ------------------------------------------------------------------ novel_pose (same parameters, the other phase's freezing)
    for n in (net, net64):
        n.cfg['phase'] = 'novel_pose'
        for p in n.parameters():
            p.requires_grad = True                    # (each phase is a run of its own in the reference)
    draws = [torch.as_tensor(rng.uniform(0, 1, (1, N_DRAWS, 3)).astype(np.float32)) for _ in range(2)]
    replaced = 0
    for _ in range(20):
        b0, b1, _ = novel_failures(ns, net64, datas, draws, th)
        if not b0.size and not b1.size:
            break
        replaced += b0.size + b1.size
        for dr, b in ((draws[0], b0), (draws[1], b1)):
            if b.size:
                dr[0, torch.as_tensor(b)] = torch.as_tensor(rng.uniform(0, 1, (b.size, 3)).astype(np.float32))
    else:
        raise AssertionError('the novel_pose draws stay ambiguous')
    print('novel_pose: %d of %d draws replaced' % (replaced, 2 * N_DRAWS))
    assert replaced <= 0.05 * 2 * N_DRAWS
    _, _, n64 = novel_failures(ns, net64, datas, draws, th)
    q64 = list(QUERIES)
    params = net.get_params()
    net.zero_grad()
    QUERIES.clear()
    nres = novel_lines(ns, net, {k: v.clone() for k, v in datas.items()}, draws)
    (nres['loss0'] + nres['loss1']).backward()
    assert nres['pbw0'].shape == n64['pbw0'].shape and nres['pbw1'].shape == n64['pbw1'].shape
    assert len(QUERIES) == 4 and all(np.array_equal(a['idx'], b['idx']) for a, b in zip(QUERIES, q64))
    assert all(p.grad is not None for p in params)
    out.update({'np.draws_world': draws[0].numpy(), 'np.draws_canonical': draws[1].numpy(),
                'np.pbw0': nres['pbw0'].detach().numpy(), 'np.tbw0': nres['tbw0'].detach().numpy(), 'np.pbw1': nres['pbw1'].detach().numpy(),
                'np.tbw1': nres['tbw1'].detach().numpy(), 'np.loss0': np.float64(nres['loss0'].item()),
                'np.loss1': np.float64(nres['loss1'].item()),
                'np.trainable': np.array([k for k, p in net.named_parameters() if p.requires_grad])})
    sampled_grads(net, 'np.', out)
    print('novel_pose: %d + %d rows chosen, losses %.6g %.6g' % (nres['pbw0'].shape[0], nres['pbw1'].shape[0], out['np.loss0'], out['np.loss1']))
    path = os.path.join(HERE, 'ref_aninerf.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
