"""Generates tests/golden/ref_bodydata.npz, the fixture of the ZJU-MoCap / H36M human-data tests:
    python tests/golden/make_golden_bodydata.py

Needs the reference tree (tests/golden/ref_import.py).  Run unmodified, in this process: the reference's NBGetRays, ToTensor, GetZvals and
GetPts (datasets/pipelines/create.py, compose.py), NBSelectRays with its sample_rays, select_all_rays and get_near_far and PerturbZvals
(augment.py), CalculateSkelTransf and AninerfIdxConversion (transforms.py) and datasets/utils/aninerf.py, on the generated scenes of
tests/bodydata_cases.py.  Stubs live in this process only: `cv2` is absent here, so a stand-in module is installed whose fillPoly is the
exact integer fill of tests/bodydata_restatement.py (fill_one); `imageio` is an empty module (LoadImageAndCamera cannot run here and is
not run).  numpy's randint is wrapped: it records every call, and for the 'two' case it places pixels whose rays miss the box at the
head of round 0's draws, so that the reference needs a second round; torch is re-seeded before PerturbZvals and the same draw stored.

Stored: per training case the draws re-derived as a [8, sel_n] table, t_rand and the item; per scene the whole frame; the skeleton
transforms.  Asserted here, element by element: the float64 restatement rounds to the reference's fp32 value for every ray of every
case; every ray has |near - far| >= 1e-9 max(|near|, |far|) and no direction component within 1e-12 of a clamp threshold -- so no ray is
left out of any comparison; the reference needed >= 2 rounds for 'two'."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import bodydata_cases as K  # noqa: E402
import bodydata_restatement as RS  # noqa: E402
import ref_import  # noqa: E402


def stand_in_cv2():
    cv2 = types.ModuleType('cv2')

    def fillPoly(mask, polys, value):
        for pts in polys:
            mask[RS.fill_one(pts, mask.shape[0], mask.shape[1])] = value
        return mask
    cv2.fillPoly = fillPoly
    sys.modules['cv2'] = cv2


def reference():
    stand_in_cv2()
    ref_import.load_mip()                                   # create.py with the mmcv stub, imported unmodified
    utils = types.ModuleType('xrnerf.datasets.utils')
    utils.__path__ = [os.path.join(ref_import.REF, 'xrnerf', 'datasets', 'utils')]
    sys.modules['xrnerf.datasets.utils'] = utils
    ani = importlib.import_module('xrnerf.datasets.utils.aninerf')
    utils.get_rigid_transformation = ani.get_rigid_transformation
    ns = types.SimpleNamespace(ani=ani)
    ns.create = importlib.import_module('xrnerf.datasets.pipelines.create')
    ns.augment = importlib.import_module('xrnerf.datasets.pipelines.augment')
    ns.transforms = importlib.import_module('xrnerf.datasets.pipelines.transforms')
    ns.compose = importlib.import_module('xrnerf.datasets.pipelines.compose')
    return ns


class Recorder:
    """np.random.randint, recorded; `head`: {call number: indices placed at the head of that call's result}"""

    def __init__(self, head=None):
        self.calls, self.head, self.real = [], head or {}, np.random.randint

    def __call__(self, low, high=None, size=None):
        out = self.real(low, high, size)
        h = self.head.get(len(self.calls))
        if h is not None:
            out[:len(h)] = h[:len(out)]
        self.calls.append((int(high), np.array(out)))
        return out


def results_of(s, mode):
    cfg = types.SimpleNamespace(mode=mode)
    return dict(cfg=cfg, img=s['img'].copy(), msk=s['msk'].copy(), cam_K=s['K'].copy(), cam_R=s['R'].copy(), cam_T=s['T'].copy(), smpl_verts=s['verts'].copy())


def assert_margins(name, s, pix):
    o, d = RS.rays(s['K'], s['R'], s['T'], pix, s['W'])
    near, far, hit = RS.box(s['bounds'], o[None], d)
    gap = np.abs(near - far) / np.maximum(np.abs(near), np.abs(far))
    assert gap.min() >= 1e-9, (name, gap.min())
    assert RS.clamp_margin(d) >= 1e-12, (name, RS.clamp_margin(d))
    return gap.min(), RS.clamp_margin(d)


def main():
    ref = reference()
    out = {}
    to_t = lambda keys: ref.compose.ToTensor(keys=keys)
    # ---- frames
    for name in K.SCENES + ('miss',):
        s = K.scene(name)
        res = ref.create.NBGetRays()(results_of(s, 'test'))
        res = ref.augment.NBSelectRays(sel_all=True)(res)
        res = to_t(['rays_o', 'rays_d', 'target_s', 'near', 'far', 'mask_at_box'])(res)
        res = ref.create.GetPts()(ref.create.GetZvals(lindisp=False, N_samples=K.S)(res))
        want = RS.frame(s['K'], s['R'], s['T'], s['H'], s['W'], s['bounds'], s['img'])
        gap, margin = assert_margins(name, s, np.arange(s['H'] * s['W']))
        for k in K.RAY_KEYS + ('mask_at_box', 'z_vals', 'pts'):
            v = res[k].numpy()
            if k in want:
                assert v.dtype == want[k].dtype and v.shape == want[k].shape and (v.view(np.uint8) == want[k].view(np.uint8)).all(), (name, k)
            out['frame.%s.%s' % (name, k)] = v
        assert res['src_shape'].tolist() == [s['H'], s['W'], 3]
        print('frame %-8s %3d of %3d rays hit, smallest relative |near - far| %.2e, clamp margin %.2e' % (name, int(want['mask_at_box'].sum()), s['H'] * s['W'], gap, margin))
    assert out['frame.miss.mask_at_box'].sum() == 0 and out['frame.axis.mask_at_box'].sum() > 0
    # ---- training items
    for i, (case, (name, n)) in enumerate(K.TRAIN.items()):
        s = K.scene(name)
        c = K.corners(s)
        bound_list, body_list = RS.lists(s['msk'], c)
        head = {}
        if case == 'two':                                   # round 0: pixels of each list whose rays miss the box, first
            for call, lst in ((0, body_list), (1, bound_list)):
                o, d = RS.rays(s['K'], s['R'], s['T'], lst, s['W'])
                head[call] = np.flatnonzero(~RS.box(s['bounds'], o[None], d)[2])[:5]
                assert len(head[call]) >= 3
        rec = Recorder(head)
        np.random.seed(100 + i)
        np.random.randint = rec
        try:
            res = ref.create.NBGetRays()(results_of(s, 'train'))
            res = ref.augment.NBSelectRays(sel_n=n)(res)
        finally:
            np.random.randint = rec.real
        rounds = len(rec.calls) // 2
        assert len(rec.calls) == 2 * rounds and 1 <= rounds <= RS.ROUNDS and (case != 'two' or rounds >= 2), (case, rounds)
        draws = np.zeros((RS.ROUNDS, n), np.int64)
        for r in range(rounds):
            (hb, ib), (hr, ir) = rec.calls[2 * r], rec.calls[2 * r + 1]
            assert hb == len(body_list) and hr == len(bound_list)
            draws[r, :len(ib)] = ib
            draws[r, len(ib):len(ib) + len(ir)] = ir
        res = to_t(['rays_o', 'rays_d', 'target_s', 'near', 'far'])(res)
        res = ref.create.GetZvals(lindisp=False, N_samples=K.S)(res)
        torch.manual_seed(200 + i)
        t_rand = torch.rand(res['z_vals'].shape)
        torch.manual_seed(200 + i)
        res = ref.create.GetPts()(ref.augment.PerturbZvals()(res))
        want, used, per_round = RS.sample(s['K'], s['R'], s['T'], s['W'], s['bounds'], s['img'], bound_list, body_list, draws, n)
        assert used == rounds and sum(per_round) == n, (case, used, rounds, per_round)
        pix = np.concatenate([np.concatenate([body_list[draws[r, :(n0 // 2)] % len(body_list)], bound_list[draws[r, (n0 // 2):n0] % len(bound_list)]])
                              for r, n0 in zip(range(rounds), [n - sum(per_round[:r]) for r in range(rounds)])])
        assert_margins(case, s, pix)
        for k in K.RAY_KEYS:
            v = res[k].numpy()
            assert v.dtype == np.float32 and v.shape == want[k].shape and (v.view(np.uint8) == want[k].view(np.uint8)).all(), (case, k)
            out['train.%s.%s' % (case, k)] = v
        out['train.%s.draws' % case], out['train.%s.t_rand' % case] = draws, t_rand.numpy()
        out['train.%s.z_vals' % case], out['train.%s.pts' % case] = res['z_vals'].numpy(), res['pts'].numpy()
        print('train %-8s sel_n %3d on %-8s: %d round(s), survivors %r' % (case, n, name, rounds, per_round))
    # ---- the skeleton transforms and the index conversion
    rng = np.random.default_rng(31)
    poses, joints = rng.normal(0, 0.3, (24, 3)).astype(np.float32), rng.uniform(-0.5, 0.5, (24, 3)).astype(np.float32)
    parents = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21])
    res = ref.transforms.CalculateSkelTransf()({'smpl_pose': poses.reshape(-1), 'joints': joints, 'parents': parents})
    out.update({'skel.poses': poses, 'skel.joints': joints, 'skel.parents': parents, 'skel.A': res['A']})
    res = ref.transforms.AninerfIdxConversion()({'latent_idx': np.array([5]), 'cfg': types.SimpleNamespace(phase='novel_pose')})
    out['idx.color_novel'] = res['color_latent_idx']
    assert res['bw_latent_idx'].tolist() == [5]
    np.savez_compressed(K.GOLD, **out)
    print('wrote %s: %d arrays, %d bytes' % (K.GOLD, len(out), os.path.getsize(K.GOLD)))


if __name__ == '__main__':
    main()
