"""The shared bodies of the BungeeNeRF / KiloNeRF data tests (xrnerf_amd/bungeedata.py, xrnerf_amd/kilodata.py,
xrnerf_amd/csrc/xr_bungeedata.hip).  Every check_* takes the device, so tests/test_gpu_scenedata.py runs it on the MI355X and
tests/test_emu_scenedata.py on the kernels' host build; tests/test_scenedata_host.py runs what needs no kernel.

Reference (tests/golden/ref_scenedata.npz, made by tests/golden/make_golden_scenedata.py): the reference's own load_google_data ->
load_data -> load_rays_bungee -> BungeeBatchSample -> GetViewdirs at stages 0, 1, 2 of the generated google-format directory, cast to
fp32; its load_nsvf_dataset / load_data on four variants of the generated NSVF directory, get_global_domain_min_and_max,
get_nodes_fixed_resolution and GetRays.

Bars.  Every output of xr_bgd_item is bit for bit the fixture (the float64 chain rounded once, tests/scenedata_restatement.py), and
near / far / z_vals are bit for bit ops.bungee_zvals of the item's own rays_o / viewdirs.  xr_bgd_frame is bit for bit bungee.pose_rays
evaluated on HOST tensors (the reference's arithmetic: true division, the 3-term sum in index order, torch.norm as an fma chain) and
ops.bungee_zvals of those rays.
The fused training item and the step-by-step one do different arithmetic by construction, so `the same dict` is checked in two parts:
  * the step-by-step list works on the fp32 item: GetViewdirs normalises the ROUNDED rays_d in fp32, the fused item rounds the float64
    quotient once (what the fixture holds).  Everything before viewdirs is bit for bit the same.  The step-by-step side is pinned on its
    own: its viewdirs are bit for bit the host fp32 normalisation of the fixture's fp32 rays_d (on the GPU, where torch.norm associates
    differently, within 4 x 2^-24), and its near / far / z_vals are bit for bit ops.bungee_zvals of its rays.  Both viewdirs are within
    0.5 + 2.5 ulp of the exact unit vector, so the two are compared at 4 x 2^-24 absolute
  * near / far / z_vals of the two items are compared with each other at BOUNDS_BAR.  The sphere root is t = (-2b - sqrt(delta)) / (2 |v|^2)
    with b = (o - c) . v of magnitude R = (6371011 + 250) s, while t itself is of the camera's height h: the fp32 roundings of b, of b^2
    and of |o - c|^2 - r^2 (each a few eps R in absolute terms, eps = 2^-24) and the viewdirs difference (|o - c| |dv| <= sqrt(3) 4 eps R)
    land on t undivided -- the r / h amplification of xr_bungee.hip's header.  Counting them: <= 10 eps R of rounding in each path and
    <= 7 eps R from dv, under 34 eps R for near / 0.9 and far / 1.1; the bar is 64 eps R absolute for near and far.  An edge is
    1 / ((1 - t) / near + t / far) or linear between an edge and far, so |dz| <= (z / near)^2 |dnear| + |dfar| <= (1 + (far / near)^2) bar,
    and a perturbed edge lies between two such edges
  * on the GPU the tensor-op path of a frame is torch's device arithmetic (division by a host scalar is a multiplication by its
    reciprocal there, torch.sum and torch.norm associate differently: tests/pipeline_cases.py's header); rays_d, viewdirs and radii of
    that path are compared at 4 ulp of the largest magnitude of the row, everything on host tensors bit for bit.
Measured beside these tests (tools/microbench_scenedata.py): at 360 x 640 the radii of pose_rays evaluated on the
GPU machine's host differ in the last bit from xr_bgd_frame's (and xr_pipe_ray_front's) in 1963 of 230400 rays.  The kernels' radii equal
the same lines in numpy (IEEE square root and division) in every bit; it is torch.sqrt on host tensors that is not correctly rounded on
that machine.  The frames used here hold no such argument on either machine; if one ever does, the numpy lines are the arbiter."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
if ROOT not in sys.path:
    sys.path.insert(1, ROOT)
G = os.path.join(ROOT, 'tests', 'golden')

H, W, N_PER, CITY_SEED = 4, 5, 2, 3
HOLDOUT, N_RAND, STAGES, PERM_SEED = 4, 16, (0, 1, 2), 11
RAY_KEYS = ['rays_o', 'rays_d', 'target_s', 'radii', 'scale_code', 'viewdirs']
ITEM_KEYS = RAY_KEYS + ['near', 'far', 'z_vals']
N_TRAIN = {0: 1, 1: 3, 2: 4}                    # train images per stage at holdout 4
NSVF_VARIANTS = {'A': dict(intrinsics='matrix4', near_far=True, traj=False, testskip=1), 'B': dict(intrinsics='line', near_far=False, traj=True, testskip=2),
                 'C': dict(intrinsics='matrix3', near_far=False, traj=False, testskip=2), 'D': dict(intrinsics='line', near_far=True, traj=True, testskip=1)}
NSVF_H, NSVF_W, NSVF_NAMES = 6, 8, ['0_0000', '0_0001', '0_0002', '1_0000', '1_0001', '2_0000', '2_0001']
NSVF_BOX = [-1.25, -1.0, -0.75, 1.5, 1.0, 1.25]
# every `type=` under `data` of every file of the reference's configs/ (collected once from the config files)
CONFIG_DATASETS = ['AniNeRFDataset', 'BungeeDataset', 'GeneBodyDataset', 'HashNerfDataset', 'KiloNerfDataset', 'KiloNerfNodeDataset', 'MipMultiScaleDataset',
                   'NeuralBodyDataset', 'SceneBaseDataset']
CONFIG_PIPELINES = ['AninerfIdxConversion', 'BatchSample', 'BungeeBatchSample', 'BungeeGetBounds', 'BungeeGetZvals', 'CalculateSkelTransf', 'DeleteUseless',
                    'ExampleSample', 'FlattenRays', 'GetBounds', 'GetPts', 'GetRays', 'GetViewdirs', 'GetZvals', 'HashBatchSample', 'HashGetRays', 'HashSetImgids',
                    'KilonerfGetRays', 'LoadImageAndCamera', 'LoadSmplParam', 'MipMultiScaleSample', 'NBGetRays', 'NBSelectRays', 'PerturbZvals', 'RandomBGColor',
                    'Sample', 'SelectRays', 'ToNDC', 'ToTensor']

BOUNDS_BAR = 64 * 2.0 ** -24             # near / far of the fused and the step-by-step item, in units of the globe radius (header)

_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(os.path.join(G, 'ref_scenedata.npz')))
    return _gold


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    assert a.shape == b.shape and a.dtype == b.dtype, '%s: %r %s against %r %s' % (what, a.shape, a.dtype, b.shape, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), '%s: the bits differ (max |a - b| %.3e)' % (what, np.abs(a.astype(np.float64) - b).max())


def within(a, b, bar, what):
    a, b = host(a).astype(np.float64), host(b).astype(np.float64)
    assert a.shape == b.shape, what
    err = np.abs(a - b).max() if a.size else 0.
    assert err <= bar, '%s: max |a - b| %.3e above %.3e' % (what, err, bar)


class Calls:
    """counts the calls of the named ops"""

    def __init__(self, *names):
        self.names = names

    def __enter__(self):
        from xrnerf_amd import ops
        self.ops, self.saved, self.n = ops, {k: getattr(ops, k) for k in self.names}, {k: 0 for k in self.names}
        for k in self.names:
            def counted(*a, _k=k, **kw):
                self.n[_k] += 1
                return self.saved[_k](*a, **kw)
            setattr(ops, k, counted)
        return self

    def __exit__(self, *exc):
        for k, f in self.saved.items():
            setattr(self.ops, k, f)
        return False


# ------------------------------------------------------------------------------------------ the generated directories
def city():
    from xrnerf_amd import bungee
    return bungee.synthetic_city(H=H, W=W, n_per_scale=N_PER, seed=CITY_SEED)


def write_google(root):
    """synthetic_city as a google-format directory: images/%03d.png (8 bits) and poses_enu.json"""
    from PIL import Image
    c = city()
    os.makedirs(os.path.join(root, 'images'), exist_ok=True)
    rows = []
    for i, (pose, img) in enumerate(zip(c['poses'], c['images'])):
        Image.fromarray(np.clip(np.rint(img * 255.), 0, 255).astype(np.uint8)).save(os.path.join(root, 'images', '%03d.png' % i))
        p = np.concatenate([pose[:3, :4], np.array([[H], [W], [c['focal']]], np.float64)], 1)
        rows.append(p.reshape(-1).tolist() + [0.5, 100.0])
    with open(os.path.join(root, 'poses_enu.json'), 'w') as fh:
        json.dump({'poses': rows, 'scene_scale': c['scene_scale'], 'scene_origin': c['scene_origin'].tolist(), 'scale_split': c['scale_split']}, fh)
    return root


def google_cfg(root, stage, mode='train', n_rand=N_RAND):
    return dict(dataset_type='mutiscale_google', datadir=root, white_bkgd=False, factor=1, N_rand_per_sampler=n_rand, mode=mode, cur_stage=stage,
                holdout=HOLDOUT, is_batching=True)


def bungee_lists(n_rand=N_RAND, S=17, ray_nearfar='sphere', perturb=False):
    """train_pipeline / test_pipeline of configs/bungeenerf/bungeenerf_multiscale_google.py"""
    tail = [dict(type='GetViewdirs', enable=True), dict(type='BungeeGetBounds', enable=True, ray_nearfar=ray_nearfar),
            dict(type='BungeeGetZvals', enable=True, lindisp=False, N_samples=S)]
    train = [dict(type='BungeeBatchSample', enable=True, N_rand=n_rand), dict(type='DeleteUseless', keys=['rays_rgb', 'idx']),
             dict(type='ToTensor', enable=True, keys=['rays_o', 'rays_d', 'target_s', 'scale_code'])] + tail + \
            [dict(type='PerturbZvals', enable=perturb), dict(type='DeleteUseless', enable=True, keys=['pose', 'iter_n'])]
    test = [dict(type='ToTensor', enable=True, keys=['pose']), dict(type='GetRays', include_radius=True, enable=True),
            dict(type='FlattenRays', include_radius=True, enable=True)] + tail + \
           [dict(type='PerturbZvals', enable=False), dict(type='DeleteUseless', enable=True, keys=['pose'])]
    return train, test


def bungee_dataset(dev, root, stage, mode='train', **kw):
    from xrnerf_amd import pipelines
    train, test = bungee_lists(**kw)
    return pipelines.build_dataset(dict(type='BungeeDataset', cfg=google_cfg(root, stage, mode), pipeline=train if mode == 'train' else test),
                                   dict(device=dev, seed=PERM_SEED))


def nsvf_poses():
    """seven non-axis-aligned camera-to-world matrices looking at the box from a tilted orbit, and two more for test_traj.txt"""
    rng = np.random.default_rng(7)
    out = []
    for k in range(len(NSVF_NAMES) + 2):
        a, e = 0.9 * k + 0.3, 0.35 + 0.1 * np.sin(1.7 * k)
        pos = 3.2 * np.array([np.cos(a) * np.cos(e), np.sin(a) * np.cos(e), np.sin(e)]) + rng.uniform(-.2, .2, 3)
        fwd = -pos / np.linalg.norm(pos)
        right = np.cross(fwd, [0.1, 0.2, 1.]); right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        m = np.eye(4)
        m[:3, :4] = np.stack([right, -up, fwd, pos], 1)            # NSVF's convention: load_nsvf_dataset negates columns 1-2
        out.append(m)
    return out


def write_nsvf(root, variant):
    """7 RGBA images of 6 x 8 (3 train, 2 val, 2 test), pose/*.txt, intrinsics.txt in the variant's layout, bbox.txt and the optional files"""
    from PIL import Image
    v = NSVF_VARIANTS[variant]
    rng = np.random.default_rng(5)
    for d in ('rgb', 'pose'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    poses = nsvf_poses()
    for name, m in zip(NSVF_NAMES, poses):
        Image.fromarray(rng.integers(0, 256, (NSVF_H, NSVF_W, 4), dtype=np.uint8)).save(os.path.join(root, 'rgb', name + '.png'))
        np.savetxt(os.path.join(root, 'pose', name + '.txt'), m, fmt='%.9f')
    f, cx, cy = 9.5, 4.25, 2.75
    with open(os.path.join(root, 'intrinsics.txt'), 'w') as fh:
        if v['intrinsics'] == 'matrix4':
            fh.write('%r 0.0 %r 0.0\n0.0 %r %r 0.0\n0.0 0.0 1.0 0.0\n0.0 0.0 0.0 1.0\n' % (f, cx, f + 0.25, cy))
        elif v['intrinsics'] == 'matrix3':
            fh.write('%r 0.0 %r\n0.0 %r %r\n0.0 0.0 1.0\n' % (f, cx, f + 0.25, cy))
        else:
            fh.write('%r %r %r 0.\n0. 0. 0.\n1.\n%d %d\n' % (f, cx, cy, NSVF_H, NSVF_W))
    with open(os.path.join(root, 'bbox.txt'), 'w') as fh:
        fh.write(' '.join(repr(x) for x in NSVF_BOX) + ' 0.25\n')
    if v['near_far']:
        with open(os.path.join(root, 'near_and_far.txt'), 'w') as fh:
            fh.write('0.75 6.5\n')
    if v['traj']:
        np.savetxt(os.path.join(root, 'test_traj.txt'), np.concatenate(poses[-2:], 0), fmt='%.9f')
    return root


def nsvf_cfg(root, variant, mode='train', **kw):
    return dict(dict(dataset_type='nsvf', datadir=root, half_res=False, testskip=NSVF_VARIANTS[variant]['testskip'], white_bkgd=True, is_batching=False,
                     render_test=not NSVF_VARIANTS[variant]['traj'], mode=mode), **kw)


def finetune_lists(sel_n=16, S=5, precrop_iters=0):
    """train_pipeline / test_pipeline of configs/kilonerf/kilonerf_finetune_*.py; with precrop_iters = 10000 the train list is
    kilonerf_pretrain_*.py's"""
    tail = [dict(type='GetViewdirs', enable=True), dict(type='ToNDC', enable=False), dict(type='GetBounds', enable=True),
            dict(type='GetZvals', enable=True, lindisp=False, N_samples=S)]
    train = [dict(type='Sample'), dict(type='DeleteUseless', keys=['images', 'poses', 'i_data', 'idx']), dict(type='ToTensor', enable=True, keys=['pose', 'target_s']),
             dict(type='GetRays', enable=True), dict(type='SelectRays', enable=True, sel_n=sel_n, precrop_iters=precrop_iters, precrop_frac=0.5)] + tail + \
            [dict(type='PerturbZvals', enable=False), dict(type='GetPts', enable=True), dict(type='DeleteUseless', enable=True, keys=['pose', 'iter_n'])]
    test = [dict(type='ToTensor', enable=True, keys=['pose']), dict(type='KilonerfGetRays', enable=True, expand_origin=True), dict(type='FlattenRays', enable=True)] + tail + \
           [dict(type='PerturbZvals', enable=False), dict(type='GetPts', enable=True), dict(type='DeleteUseless', enable=True, keys=['pose'])]
    return train, test


# ------------------------------------------------------------------------------------------ host tier
def check_symbols(loaded=True):
    """the header, the ctypes table, the source and the build recipe name the same xr_bgd_* entry points; no other table holds one"""
    import re
    from xrnerf_amd import _lib, build, ops
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_bungeedata.h')).read()
    declared = set(re.findall(r'^int (xr_bgd_\w+)\(', header, re.M))
    assert declared == set(_lib.BUNGEEDATA_SIGNATURES) == {'xr_bgd_item', 'xr_bgd_frame'}
    for name, (res, args) in _lib.BUNGEEDATA_SIGNATURES.items():
        text = header[header.index('int %s(' % name):]
        assert text[:text.index(');')].count(',') + 1 == len(args), name
    others = [v for k, v in vars(_lib).items() if k.endswith('SIGNATURES') and k != 'BUNGEEDATA_SIGNATURES']
    assert len(others) >= 15 and not any(k.startswith('xr_bgd_') for t in others for k in t)
    assert 'xr_bgd_' not in open(os.path.join(ROOT, 'include', 'xrnerf_mi355.h')).read()
    assert build.SOURCES['xr_bungeedata.hip'] == ['-ffp-contract=off'] and build.SOURCES['xr_bungee.hip'] == ['-ffp-contract=off']
    source = open(os.path.join(ROOT, 'xrnerf_amd', 'csrc', 'xr_bungeedata.hip')).read()
    assert set(re.findall(r'extern "C" int (xr_\w+)\(', source)) == declared
    for src in ('xr_bungee.hip', 'xr_bungeedata.hip'):              # one copy of the bounds and the edges
        text = open(os.path.join(ROOT, 'xrnerf_amd', 'csrc', src)).read()
        assert '#include "xr_bungee_zvals.h"' in text and 'bg_sphere_dist(const' not in text
    for macro, value in (('CAM_DOUBLES', ops.BGD_CAM_DOUBLES), ('MAX_SAMPLES', ops.BGD_MAX_SAMPLES)):
        assert int(re.search(r'#define XR_BGD_%s (\d+)u' % macro, header).group(1)) == value
    if loaded:
        lib = _lib.load()
        assert all(hasattr(lib, name) for name in declared) and ops.bungeedata_kernels_available()


def check_registries():
    from xrnerf_amd import pipelines
    assert [n for n in CONFIG_DATASETS if n not in pipelines.DATASETS] == [] and [n for n in CONFIG_PIPELINES if n not in pipelines.PIPELINES] == []
    check_hash_steps()


def check_hash_steps(dev=None):
    """the instant-ngp transforms: the slices, the composite and the ids on plain tensors; with a device, HashGetRays against
    get_rays_np_hash (get_rays.py:35-60) restated in float64"""
    from xrnerf_amd import pipelines
    build = lambda **kw: pipelines.PIPELINES.build(kw)
    table = torch.arange(7 * 11, dtype=torch.float32).view(7, 11) / 100.
    sample = build(type='HashBatchSample', N_rand=3)
    a, b, c = sample({'rays_rgb': table}), sample({'rays_rgb': table}), sample({'rays_rgb': table})
    assert torch.equal(a['rays_o'], table[:3, :3]) and torch.equal(b['target_s'], table[3:6, 6:9]) and torch.equal(c['img_ids'], table[:3, 10:])      # the cursor wraps
    assert tuple(a['alpha'].shape) == (3, 1) and sample({'rays_rgb': table, 'N_rand': 2})['rays_d'].shape[0] == 2
    bg = torch.full((3, 3), 0.5)
    out = build(type='RandomBGColor')(dict(a, bg_color=bg))
    assert torch.equal(out['target_s'], a['target_s'] * a['alpha'] + bg * (1 - a['alpha'])) and out['bg_color'].dtype == torch.float32
    drawn = build(type='RandomBGColor')({'alpha': torch.zeros(4, 1), 'target_s': torch.zeros(4, 3)})
    assert torch.equal(drawn['target_s'], drawn['bg_color']) and bool((drawn['bg_color'] >= 0).all()) and bool((drawn['bg_color'] < 1).all())
    ids = build(type='HashSetImgids')({'rays_o': torch.zeros(6, 3), 'idx': 4})['img_ids']
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (6, 1) and ids.unique().tolist() == [4]
    if dev is None:
        return
    hh, ww, K = 5, 7, np.array([[9., 0, 3.5], [0, 9., 2.5], [0, 0, 1]])
    pose = np.concatenate([np.linalg.qr(np.random.default_rng(3).normal(size=(3, 3)))[0], [[0.4, 0.5, 0.6]]], 0)                  # [4, 3]
    got = build(type='HashGetRays', H=hh, W=ww, K=K)({'pose': torch.tensor(pose, dtype=torch.float32, device=dev)})
    sync()
    i, j = np.meshgrid(np.arange(ww) + 0.5, np.arange(hh) + 0.5, indexing='xy')
    d = np.stack([(i - K[0][2]) / K[0][0], (j - K[1][2]) / K[1][1], np.ones_like(i)], -1) @ pose[:3, :3]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    assert tuple(got['rays_d'].shape) == (hh, ww, 3) and got['rays_d'].device.type == dev.type
    within(got['rays_d'], d, 1e-6, 'HashGetRays rays_d')
    within(got['rays_o'], np.broadcast_to(pose[3], d.shape), 1e-7, 'HashGetRays rays_o')


def check_plans():
    """the two Bungee lists plan to BungeeRun, the finetune lists to _FusedRun, the existing lists as before"""
    import bodydata_cases as BK
    from xrnerf_amd import bungeedata, pipelines
    BK.check_plans()                                               # pipeline_cases, multiscale_cases and bodydata_cases lists
    info = dict(H=H, W=W, K=np.array([[6., 0, 2.5], [0, 6., 2.], [0, 0, 1]]), scene_origin=[0., 0., -6371011.], scene_scaling_factor=0.0025, near=2., far=6.)
    compose = lambda steps: pipelines.Compose([dict(s, **info) for s in steps])
    train, test = bungee_lists()
    c = compose(train)
    assert type(c.fused) is bungeedata.BungeeRun and (c.fused.start, c.fused.end) == (0, 5) and c.fused.sample is not None and not c.fused.perturb
    c = compose(bungee_lists(perturb=True)[0])
    assert type(c.fused) is bungeedata.BungeeRun and (c.fused.start, c.fused.end) == (0, 6) and c.fused.perturb
    c = compose(test)
    assert type(c.fused) is bungeedata.BungeeRun and (c.fused.start, c.fused.end) == (1, 5) and c.fused.rays is not None
    assert compose(train[:4]).fused is None and compose(train[1:]).fused is None                      # no z-values; no sample
    assert compose([s for s in train if s['type'] != 'GetViewdirs']).fused is None                    # the bounds need viewdirs
    assert compose([dict(s, include_radius=False) if s['type'] == 'GetRays' else s for s in test]).fused is None
    assert compose(test[:5] + [dict(type='PerturbZvals', enable=True)]).fused is None                  # a perturbed frame: step by step
    assert compose(train[:1] + [dict(type='DeleteUseless', keys=['rays_o'])] + train[1:]).fused is None
    ftrain, ftest = finetune_lists()
    c = compose(ftest)
    assert type(c.fused) is pipelines._FusedRun and type(c.transforms[c.fused.start]) is pipelines.KilonerfGetRays and type(c.transforms[c.fused.end]) is pipelines.GetPts
    plain = compose([dict(s, type='GetRays') if s['type'] == 'KilonerfGetRays' else s for s in ftest])
    assert (plain.fused.start, plain.fused.end) == (c.fused.start, c.fused.end)                       # wherever GetRays plans
    assert type(compose(ftrain).fused) is pipelines._FusedRun
    assert repr(pipelines.PIPELINES.build(dict(type='BungeeBatchSample'))) == 'BungeeBatchSample:sample a batch of rays from all rays'
    assert repr(pipelines.PIPELINES.build(dict(type='ExampleSample'))) == 'ExampleSample:slice a batch of examples from all examples'


def check_refusals_host(tmp):
    """what is refused before any kernel is asked: H < 3, a scale_split that disagrees with the image count, expand_origin=False when fused"""
    import pytest
    from xrnerf_amd import bungeedata, ops, pipelines
    cpu = torch.device('cpu')
    with pytest.raises(ValueError):
        ops.bgd_frame(torch.zeros(3, 4), 2, 5, np.eye(3), S=4)
    with pytest.raises(ValueError):
        ops.bgd_item(torch.zeros(1, 12, dtype=torch.float64), None, None, None, 2, 5, 6.0, None, 0, 4)
    with pytest.raises(ValueError):
        bungeedata.BungeeState(2, 5, 6.0, np.zeros((2, 3, 4)), np.zeros((2, 2, 5, 3), np.float32), [0, 0], [1], cpu)
    with pytest.raises(ValueError):
        bungeedata.scale_codes(3, 6, [4, 2, 0], 0)                 # stage 0 of 6 images split at 4 holds 2 images, not 3
    assert bungeedata.scale_codes(4, 6, [4, 2, 0], 1).tolist() == [0, 0, 1, 1]
    root = write_google(os.path.join(tmp, 'google_bad'))
    meta = json.load(open(os.path.join(root, 'poses_enu.json')))
    meta['scale_split'] = [7, 2, 0]                               # more images above the first split than the directory holds
    json.dump(meta, open(os.path.join(root, 'poses_enu.json'), 'w'))
    with pytest.raises(ValueError):
        pipelines.build_dataset(dict(type='BungeeDataset', cfg=google_cfg(root, 1, 'val'), pipeline=[]), dict(device=cpu))
    with pytest.raises(ValueError):
        bungeedata.BungeeState(4, 5, 6.0, np.zeros((2, 3, 4)), np.zeros((2, 4, 5, 3), np.float32), [0, 0], [1], cpu, perm=np.zeros(20, np.int64))
    with pytest.raises(ValueError):
        pipelines.PIPELINES.build(dict(type='BungeeGetBounds', ray_nearfar='cube'))
    info = dict(H=6, W=8, K=np.array([[9.5, 0, 4.], [0, 9.5, 3.], [0, 0, 1]]), near=2., far=6.)
    ftest = [dict(s, expand_origin=False) if s['type'] == 'KilonerfGetRays' else s for s in finetune_lists()[1]]
    comp = pipelines.Compose([dict(s, **info) for s in ftest[:2]])
    assert pipelines.Compose([dict(s, **info) for s in ftest]).fused is None            # the fused run is declined
    out = comp({'pose': torch.eye(4)[:3]})
    assert tuple(out['rays_o'].shape) == (3,) and tuple(out['rays_d'].shape) == (6, 8, 3)
    for name in ('deepvoxels', 'LINEMOD'):
        with pytest.raises(NotImplementedError):
            pipelines.build_dataset(dict(type='SceneBaseDataset', cfg=dict(dataset_type=name, datadir=tmp), pipeline=[]), dict(device=cpu))


def check_nsvf_loader(tmp):
    """load_nsvf_dataset and SceneBaseDataset._load_data reproduce the fixture on the generated directory, for each variant"""
    from xrnerf_amd import builder, kilodata, pipelines
    g = gold()
    for name, v in NSVF_VARIANTS.items():
        root = write_nsvf(os.path.join(tmp, 'nsvf_' + name), name)
        rgbs, poses, intr, near, far, bg, render_poses, i_split = kilodata.load_nsvf_dataset(root, v['testskip'])
        pre = 'nsvf.%s.' % name
        same_bits(rgbs, g[pre + 'rgbs'], name + ' rgbs')
        same_bits(poses, g[pre + 'poses'], name + ' poses')
        same_bits(np.asarray(render_poses), g[pre + 'traj'], name + ' test_traj')
        assert [intr.H, intr.W] == [NSVF_H, NSVF_W] and np.array_equal(np.array([intr.fx, intr.fy, intr.cx, intr.cy], np.float64), g[pre + 'intrinsics'])
        assert np.array_equal(np.array([near, far], np.float64), g[pre + 'near_far']) and bg is None
        for a, k in zip(i_split, ('i_train', 'i_val', 'i_test')):
            assert np.array_equal(a, g[pre + 'split.' + k]), (name, k)
        ds = pipelines.SceneBaseDataset.__new__(pipelines.SceneBaseDataset)
        ds.cfg = builder.ConfigDict.wrap(nsvf_cfg(root, name))
        images, poses, render_poses, hwf, K, near, far, i_train, i_val, i_test = ds._load_data()
        same_bits(images, g[pre + 'images'], name + ' images')
        same_bits(np.asarray(render_poses), g[pre + 'render_poses'], name + ' render_poses')
        assert hwf[:2] == [NSVF_H, NSVF_W] and np.array_equal(np.asarray(K, np.float64), g[pre + 'K']) and np.float64(hwf[2]) == g[pre + 'K'][0, 0]
        assert np.array_equal(np.array([near, far], np.float64), g[pre + 'near_far'])
        for a, k in zip((i_train, i_val, i_test), ('i_train', 'i_val', 'i_test')):
            assert np.array_equal(a, g[pre + k]), (name, k)
    gmin, gmax = kilodata.get_global_domain_min_and_max(builder.ConfigDict.wrap(nsvf_cfg(root, 'D')))
    same_bits(gmin, g['nsvf.gmin'], 'global_domain_min')
    same_bits(gmax, g['nsvf.gmax'], 'global_domain_max')
    t = kilodata.get_global_domain_min_and_max(dict(global_domain_min=[0., 1., 2.], global_domain_max=[3., 4., 5.]), torch.device('cpu'))
    assert t[0].dtype == torch.float32 and t[1].tolist() == [3., 4., 5.]


def batching_list(n_rand=16, S=5):
    """the batching train list of configs/nerf/nerf_blender_base01.py, which a KiloNerfDataset with is_batching=True takes"""
    return [dict(type='BatchSample', enable=True, N_rand=n_rand), dict(type='DeleteUseless', keys=['rays_rgb', 'idx']),
            dict(type='ToTensor', enable=True, keys=['rays_o', 'rays_d', 'target_s']), dict(type='GetViewdirs', enable=True), dict(type='ToNDC', enable=False),
            dict(type='GetBounds', enable=True), dict(type='GetZvals', enable=True, lindisp=False, N_samples=S), dict(type='PerturbZvals', enable=False),
            dict(type='GetPts', enable=True), dict(type='DeleteUseless', enable=True, keys=['pose', 'iter_n'])]


def node_cfg(root, work_dir, mode='train', **kw):
    return dict(dict(dataset_type='nsvf', datadir=root, mode=mode, batch_index=0, work_dir=work_dir, num_examples_per_network=96 if mode == 'train' else 40,
                     max_num_networks=3, train_batch_size=32, outputs='color_and_density', is_batching=False, fixed_resolution=[2, 1, 2]), **kw)


def distill_lists():
    train = [dict(type='ExampleSample', enable=True, train_batch_size=32), dict(type='ToTensor', enable=True, keys=['domain_mins', 'domain_maxs']),
             dict(type='DeleteUseless', enable=True, keys=['all_examples'])]
    return train, [dict(type='ToTensor', enable=True, keys=['domain_mins', 'domain_maxs'])]


def check_node_cp(tmp):
    """the checkpoint dict and the node boxes of batch_index 0 equal the fixture (no kernel: an empty val set is never generated)"""
    from xrnerf_amd import kilodata, pipelines
    g = gold()
    root = write_nsvf(os.path.join(tmp, 'nsvf_cp'), 'A')
    build = lambda **kw: pipelines.build_dataset(dict(type='KiloNerfNodeDataset', cfg=node_cfg(root, os.path.join(tmp, 'work'), **kw), pipeline=distill_lists()[0]),
                                                 dict(device=torch.device('cpu')))
    ds = build()
    assert sorted(ds.cp) == sorted(kilodata.KiloNerfNodeDataset.CP_KEYS) and ds.cp['phase'] == 'discovery' and ds.cp['fitted_volume'] == 0 == ds.cp['num_networks_fitted']
    assert len(ds.cp['root_nodes']) == 4 and len(ds.node_batch) == 3 and len(ds.cp['nodes_to_process']) == 1 and len(ds.cp['saturated_nodes_to_process']) == 0
    same_bits(np.array([n.domain_min for n in ds.cp['root_nodes']], np.float32), g['nodes.mins'].astype(np.float32), 'node mins')
    same_bits(np.array([n.domain_max for n in ds.cp['root_nodes']], np.float32), g['nodes.maxs'].astype(np.float32), 'node maxs')
    assert np.float32(ds.cp['total_volume']) == np.float32(g['nodes.total_volume']) and not ds.processing_saturated_nodes
    assert sorted(ds.get_info()) == ['cp', 'node_batch', 'processing_saturated_nodes'] and len(ds) == 3
    assert [n.domain_min for n in ds.node_batch] == ds.domain_mins and ds.node_batch[0] is ds.cp['root_nodes'][0]
    ds.save_cp()
    nxt = build(batch_index=1)                                     # the next batch: the one box left
    assert len(nxt.node_batch) == 1 and nxt.node_batch[0].domain_min == ds.cp['root_nodes'][3].domain_min and len(nxt.cp['nodes_to_process']) == 0
    one = pipelines.build_dataset(dict(type='KiloNerfNodeDataset', cfg={k: v for k, v in node_cfg(root, tmp).items() if k != 'fixed_resolution'}, pipeline=[]),
                                  dict(device=torch.device('cpu')))
    assert len(one.cp['root_nodes']) == 1 and len(one.node_batch) == 1
    same_bits(np.asarray(one.node_batch[0].domain_min), g['nsvf.gmin'], 'the root box')
    ex = torch.arange(2 * 7 * 10, dtype=torch.float32).view(2, 7, 10)
    out = pipelines.Compose(distill_lists()[0])({'all_examples': ex, 'example_indices': [5, 0, 5], 'domain_mins': [[0., 0, 0]], 'domain_maxs': [[1., 1, 1]]})
    assert torch.equal(out['batch_examples'], ex[:, [5, 0, 5]]) and 'all_examples' not in out and out['domain_mins'].dtype == torch.float32
    out = pipelines.PIPELINES.build(dict(type='ExampleSample', train_batch_size=4))({'all_examples': ex})
    assert tuple(out['batch_examples'].shape) == (2, 4, 10)


# ------------------------------------------------------------------------------------------ kernel tiers
def zvals_of(item, ds_or_info, S, ray_nearfar):
    from xrnerf_amd import ops
    info = ds_or_info if isinstance(ds_or_info, dict) else ds_or_info.get_info()
    return ops.bungee_zvals(item['rays_o'].contiguous(), item['viewdirs'].contiguous(), None, None, S, ray_nearfar,
                            tuple(float(v) for v in info['scene_origin']), float(info['scene_scaling_factor']))


def check_items(dev, tmp):
    """every item of the train split at stages 0, 1, 2, the short last slice included: the fixture's bits; near / far / z_vals: the bits of
    ops.bungee_zvals of the item's rays, for both bounds and two sample counts; the default draw is the reference's permutation"""
    g = gold()
    root = write_google(os.path.join(tmp, 'google'))
    for stage in STAGES:
        total = N_TRAIN[stage] * H * W
        for ray_nearfar, S in (('sphere', 17), ('flat', 8), ('sphere', 8), ('flat', 17)):
            ds = bungee_dataset(dev, root, stage, S=S, ray_nearfar=ray_nearfar)
            assert len(ds) == total // N_RAND and len(ds.state) == total and ds.n_images == 6 and ds.cur_stage == stage
            same_bits(ds.state.perm, g['bungee.s%d.perm' % stage], 'stage %d: the default draw' % stage)
            assert ds.i_train.tolist() == g['bungee.s%d.i_train' % stage].tolist() and ds.i_test.tolist() == g['bungee.s%d.i_test' % stage].tolist()
            items = [ds[i] for i in range(-(-total // N_RAND))]
            sync()
            assert all(sorted(it) == sorted(ITEM_KEYS) for it in items) and items[-1]['rays_o'].shape[0] == total - N_RAND * (len(items) - 1)
            for k in RAY_KEYS:
                same_bits(torch.cat([it[k] for it in items], 0), g['bungee.s%d.%s' % (stage, k)], 'stage %d %s %d: %s' % (stage, ray_nearfar, S, k))
            for i, it in enumerate(items):
                near, far, z = zvals_of(it, ds, S, ray_nearfar)
                for k, v in (('near', near), ('far', far), ('z_vals', z)):
                    same_bits(it[k], v, 'stage %d %s %d item %d: %s' % (stage, ray_nearfar, S, i, k))
                assert tuple(it['z_vals'].shape) == (it['rays_o'].shape[0], S) and bool((it['z_vals'][:, 1:] >= it['z_vals'][:, :-1]).all())
                assert bool((it['near'] > 0).all()) and bool((it['far'] > it['near']).all())
        info = ds.get_info()
        assert sorted(info) == sorted(['H', 'W', 'focal', 'K', 'render_poses', 'hwf', 'cur_stage', 'scene_origin', 'scene_scaling_factor', 'scale_split'])
        assert np.array_equal(np.asarray(info['K'], np.float64), g['bungee.K']) and info['scale_split'] == [4, 2, 0] and info['hwf'][:2] == [H, W]
        assert ds.state.bytes_per_ray() < 88 / 2.                   # 20 a ray plus the per-image tables, which weigh at 20 rays an image


def check_compose(dev, tmp):
    """the training list: ONE xr_bgd_item launch when fused; step by step it is the sample's launch and tensor ops (see the bars in this
    file's header); over the materialised tables no item launch at all; PerturbZvals with a given t_rand is pipelines._perturb"""
    from xrnerf_amd import pipelines
    g = gold()
    root = write_google(os.path.join(tmp, 'google'))
    S = 17
    ds = bungee_dataset(dev, root, 2, S=S, perturb=True)
    assert type(ds.pipeline.fused).__name__ == 'BungeeRun'
    tables = ds.state.materialise()
    assert tuple(tables['rays_rgb'].shape) == (80, 3, 3) and tables['scale_code'].dtype == torch.int64
    for idx in (0, 4):
        n = 16
        t_rand = torch.rand((n, S), generator=torch.Generator().manual_seed(idx)).to(dev)
        outs = {}
        for mode in ('fused', 'steps', 'tables'):
            ds.pipeline.fuse = mode == 'fused'
            data = ds._fetch_train_data(idx)
            if mode == 'tables':
                data = dict(tables, idx=idx, iter_n=0)
            with Calls('bgd_item', 'bungee_zvals') as calls:
                outs[mode] = ds.pipeline(dict(data, t_rand=t_rand.clone()))
            sync()
            assert calls.n == {'fused': dict(bgd_item=1, bungee_zvals=0), 'steps': dict(bgd_item=1, bungee_zvals=2), 'tables': dict(bgd_item=0, bungee_zvals=2)}[mode], (mode, calls.n)
            assert sorted(outs[mode]) == sorted(ITEM_KEYS), (mode, sorted(outs[mode]))
        ds.pipeline.fuse = True
        f, s, t = outs['fused'], outs['steps'], outs['tables']
        for k in ITEM_KEYS:
            assert f[k].dtype == s[k].dtype == t[k].dtype and f[k].shape == s[k].shape == t[k].shape and f[k].device.type == dev.type, k
            same_bits(s[k], t[k], 'step by step against the materialised tables: %s' % k)
        for k in ('rays_o', 'rays_d', 'target_s', 'radii', 'scale_code'):
            same_bits(f[k], s[k], 'fused against step by step: %s' % k)
        within(f['viewdirs'], s['viewdirs'], 4 * 2.0 ** -24, 'fused against step by step: viewdirs')
        # the step-by-step side, pinned: GetViewdirs' fp32 normalisation of the FIXTURE's fp32 rays_d, evaluated on host tensors
        d32 = torch.from_numpy(g['bungee.s2.rays_d'][idx * N_RAND:idx * N_RAND + n])
        pinned = (d32 / torch.norm(d32, dim=-1, keepdim=True)).reshape(-1, 3).float()
        if dev.type == 'cpu':
            same_bits(s['viewdirs'], pinned, 'step by step viewdirs against the host normalisation of the fixture rays_d')
        else:                                                      # torch.norm on the device associates differently: one ulp of the norm
            within(s['viewdirs'], pinned, 4 * 2.0 ** -24, 'step by step viewdirs against the host normalisation of the fixture rays_d')
        unperturbed = {}
        for name, it in (('fused', f), ('steps', s)):
            near, far, z = zvals_of(it, ds, S, 'sphere')
            same_bits(it['near'], near, name + ' near')
            same_bits(it['far'], far, name + ' far')
            same_bits(it['z_vals'], pipelines._perturb(z, t_rand), name + ' perturbed z_vals')
            unperturbed[name] = z
        # the two paths against each other, at BOUNDS_BAR (this file's header)
        info = ds.get_info()
        bar = BOUNDS_BAR * (6371011. + 250.) * float(info['scene_scaling_factor'])
        zbar = bar * (1. + float((f['far'] / f['near']).max()) ** 2)
        figures = {k: float((f[k].double() - s[k].double()).abs().max()) for k in ('near', 'far', 'z_vals')}
        print('item %d: max |fused - step by step| near %.3e far %.3e (bar %.3e) z_vals %.3e (bar %.3e)' % (idx, figures['near'], figures['far'], bar, figures['z_vals'], zbar))
        within(f['near'], s['near'], bar, 'fused against step by step: near')
        within(f['far'], s['far'], bar, 'fused against step by step: far')
        within(f['z_vals'], s['z_vals'], zbar, 'fused against step by step: z_vals')
        within(unperturbed['fused'], unperturbed['steps'], zbar, 'fused against step by step: un-perturbed z_vals')
    drawn = ds[1]                                                  # without t_rand: the draw is made on the device, inside the bins
    near, far, z = zvals_of(drawn, ds, S, 'sphere')
    sync()
    assert bool((drawn['z_vals'] >= z[:, :1]).all()) and bool((drawn['z_vals'] <= z[:, -1:]).all()) and not torch.equal(drawn['z_vals'], z)


def check_frame(dev, tmp):
    """a validation frame: xr_bgd_frame is bungee.pose_rays on host tensors + ops.bungee_zvals in every bit, the last image row (whose
    radius repeats dx[H-3]) included; the test list is ONE launch"""
    from xrnerf_amd import bungee, ops
    root = write_google(os.path.join(tmp, 'google'))
    for ray_nearfar, S in (('sphere', 17), ('flat', 8)):
        ds = bungee_dataset(dev, root, 2, mode='val', S=S, ray_nearfar=ray_nearfar)
        assert len(ds) == 1 and type(ds.pipeline.fused).__name__ == 'BungeeRun'
        val = ds[0]
        assert sorted(val) == ['images', 'poses', 'spiral_poses'] and tuple(val['poses'].shape) == (2, 3, 4) and tuple(val['images'].shape) == (2, H, W, 3)
        info = ds.get_info()
        for pose in val['poses']:
            with Calls('bgd_frame', 'bungee_zvals') as calls:
                got = ds.pipeline({'pose': pose})
            assert calls.n == dict(bgd_frame=1, bungee_zvals=0) and sorted(got) == sorted(['rays_o', 'rays_d', 'radii', 'viewdirs', 'near', 'far', 'z_vals', 'src_shape'])
            ref = bungee.pose_rays(pose.cpu(), H, W, info['K'])
            for k in ('rays_o', 'rays_d', 'radii', 'viewdirs'):
                same_bits(got[k], ref[k], 'frame %s %s' % (ray_nearfar, k))
            assert got['src_shape'].tolist() == [H, W, 3] and ref['src_shape'].tolist() == [H, W, 3]
            near, far, z = zvals_of(got, ds, S, ray_nearfar)
            for k, v in (('near', near), ('far', far), ('z_vals', z)):
                same_bits(got[k], v, 'frame %s %s' % (ray_nearfar, k))
            same_bits(got['radii'][-W:], got['radii'][-3 * W:-2 * W], 'the last row repeats dx[H-3]')
            ds.pipeline.fuse = False
            with Calls('bgd_frame', 'bungee_zvals') as calls:
                steps = ds.pipeline({'pose': pose})
            ds.pipeline.fuse = True
            sync()
            assert calls.n == dict(bgd_frame=0, bungee_zvals=2) and sorted(steps) == sorted(got)
            for k in ('rays_o', 'rays_d', 'radii', 'viewdirs'):
                assert steps[k].dtype == got[k].dtype and steps[k].shape == got[k].shape
                if dev.type == 'cpu':
                    same_bits(steps[k], got[k], 'frame step by step %s' % k)
                else:
                    within(steps[k], got[k], 4 * 2.0 ** -23 * float(got[k].abs().max()), 'frame step by step %s' % k)
            part = ops.bgd_frame(pose[:3, :4], H, W, info['K'], want=('radii', 'rays_d'))
            assert sorted(part) == ['radii', 'rays_d']
            same_bits(part['radii'], got['radii'], 'a subset of the outputs')
    test = bungee_dataset(dev, root, 2, mode='test')
    assert len(test) == 2 and sorted(test[1]) == ['idx', 'image', 'pose'] and test[1]['idx'] == 1
    same_bits(test[1]['pose'], val['poses'][1], 'the test pose')


def check_out_of_range(dev, tmp):
    """an index outside the table: NaN rays, code -1, nothing read; the neighbours untouched.  A slice past the table: the short batch."""
    from xrnerf_amd import ops
    root = write_google(os.path.join(tmp, 'google'))
    st = bungee_dataset(dev, root, 1).state
    bad = st.perm.clone()
    bad[3], bad[17], bad[40] = -1, len(st), 2 ** 40
    args = (st.cams, st.codes, st.images, st.i_train, H, W, st.focal)
    kw = dict(S=8, scaling=0.0025, scene_origin=(0., 0., -6371011.))
    got, full = ops.bgd_item(*args, bad, 0, 48, **kw), ops.bgd_item(*args, st.perm, 0, 48, **kw)
    sync()
    ok = [i for i in range(48) if i not in (3, 17, 40)]
    for k in got:
        if k == 'scale_code':
            assert got[k][[3, 17, 40]].reshape(-1).tolist() == [-1, -1, -1]
        else:
            assert bool(torch.isnan(got[k][[3, 17, 40]]).all()), k
        same_bits(got[k][ok], full[k][ok], 'rays beside an out-of-range index: %s' % k)
    wild = st.i_train.clone()
    wild[1] = 99                                                    # an image slot that names no image
    got = ops.bgd_item(st.cams, st.codes, st.images, wild, H, W, st.focal, st.perm, 0, 60, want=('rays_d', 'scale_code'))
    sync()
    hit = ((st.perm // (H * W)) == 1).cpu()
    assert bool(torch.isnan(got['rays_d'].cpu()[hit]).all()) and not bool(torch.isnan(got['rays_d'].cpu()[~hit]).any())
    tail = ops.bgd_item(*args, st.perm, 48, 16, **kw)
    none = ops.bgd_item(*args, st.perm, 64, 16, **kw)
    assert tail['rays_o'].shape[0] == 12 and tail['z_vals'].shape == (12, 8) and none['rays_o'].shape[0] == 0 and none['scale_code'].dtype == torch.int64
    same_bits(tail['rays_d'], ops.bgd_item(*args, st.perm, 0, 60, want=('rays_d',))['rays_d'][48:], 'the short batch')
    big = ops.bgd_item(*args, st.perm, 0, 60, S=300, t_rand=torch.rand((60, 300), generator=torch.Generator().manual_seed(1)).to(dev), **{k: v for k, v in kw.items() if k != 'S'})
    near, far, z = ops.bungee_zvals(big['rays_o'], big['viewdirs'], None, None, 300, 'sphere', kw['scene_origin'], kw['scaling'])
    sync()
    assert bool((big['z_vals'][:, 1:] >= big['z_vals'][:, :-1]).all()) and bool((big['z_vals'] >= z[:, :1]).all()) and bool((big['z_vals'] <= z[:, -1:]).all())
    same_bits(ops.bgd_item(*args, st.perm, 0, 60, S=300, want=('z_vals',), **{k: v for k, v in kw.items() if k != 'S'})['z_vals'], z, 'a row longer than the workgroup')


def check_sort(dev):
    """rows the reference's sort really reorders: far below near (the whole row reversed) and NaN bounds (NaN last) -- through the
    kernels' own rays, against ops.bungee_zvals, whose insertion sort is the other statement of the same order"""
    from xrnerf_amd import ops
    n, hw = 2, 12
    cams = torch.zeros((n, 12), dtype=torch.float64)
    cams[:, 0], cams[:, 5], cams[:, 10] = 1., 1., 1.
    cams[0, 11], cams[1, 11] = 0.5, -0.5                           # a camera above the near plane, and one below the ground: far < near
    args = (cams.to(dev), torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros((n, 3, 4, 3), device=dev), torch.tensor([0, 1], dtype=torch.int32, device=dev), 3, 4, 5.0)
    perm = torch.arange(2 * hw, dtype=torch.int64, device=dev)
    got = ops.bgd_item(*args, perm, 0, 2 * hw, S=9, ray_nearfar='flat', scaling=0.001)
    near, far, z = ops.bungee_zvals(got['rays_o'], got['viewdirs'], None, None, 9, 'flat', (0., 0., 0.), 0.001)
    sync()
    same_bits(got['z_vals'], z, 'rows the sort reorders')
    same_bits(got['near'], near, 'near')
    assert bool((got['far'][hw:] < got['near'][hw:]).all()) and bool((got['z_vals'][:, 1:] >= got['z_vals'][:, :-1]).all())


def check_host_tensors_raise(dev):
    import pytest
    from xrnerf_amd import _lib, ops
    with pytest.raises(_lib.XrError):
        ops.bgd_frame(torch.eye(4)[:3], H, W, np.eye(3), S=4)
    with pytest.raises(_lib.XrError):
        ops.bgd_item(torch.zeros((1, 12), dtype=torch.float64), torch.zeros(1, dtype=torch.int64), torch.zeros((1, H, W, 3)), torch.zeros(1, dtype=torch.int32), H, W, 6.0,
                     torch.arange(20), 0, 4)
    with pytest.raises(_lib.XrError):
        ops.bgd_frame(torch.eye(4, device=dev)[:3], H, W, np.eye(3), S=1)          # one edge is no interval
    with pytest.raises(_lib.XrError):
        ops.bgd_frame(torch.eye(4, device=dev)[:3], H, W, np.eye(3), S=4, ray_nearfar=None)


def check_set_stage(dev, tmp):
    """set_stage(k) gives the items, the info and the length of a freshly built dataset of stage k"""
    root = write_google(os.path.join(tmp, 'google'))
    ds = bungee_dataset(dev, root, 0)
    for stage in (2, 1, 0):
        ds.set_stage(stage)
        fresh = bungee_dataset(dev, root, stage)
        assert len(ds) == len(fresh) and ds.cur_stage == stage and ds.get_info()['cur_stage'] == stage and ds.i_train.tolist() == fresh.i_train.tolist()
        same_bits(ds.get_info()['render_poses'], fresh.get_info()['render_poses'], 'render_poses')
        for idx in range(len(fresh) + 1):
            a, b = ds[idx], fresh[idx]
            sync()
            for k in ITEM_KEYS:
                same_bits(a[k], b[k], 'set_stage(%d) item %d %s' % (stage, idx, k))


def check_kilo_dataset(dev, tmp):
    """KiloNerfDataset over the NSVF directory: train, val and test items through the fused run equal the step-by-step path and the
    fixture's GetRays"""
    from xrnerf_amd import pipelines
    g = gold()
    root = write_nsvf(os.path.join(tmp, 'nsvf_A'), 'A')
    train_list, test_list = finetune_lists()
    sets = {m: pipelines.build_dataset(dict(type='KiloNerfDataset', cfg=nsvf_cfg(root, 'A', m), pipeline=train_list if m == 'train' else test_list), dict(device=dev))
            for m in ('train', 'val', 'test')}
    tr, va, te = sets['train'], sets['val'], sets['test']
    assert len(tr) == 3 and len(va) == 1 and len(te) == 2 and type(va.pipeline.fused) is pipelines._FusedRun and type(tr.pipeline.fused) is pipelines._FusedRun
    same_bits(tr.global_domain_min, g['nsvf.gmin'], 'global_domain_min')
    same_bits(tr.images, g['nsvf.A.images'], 'resident images')
    close = (lambda a, b, what: same_bits(a, b, what)) if dev.type == 'cpu' else (lambda a, b, what: within(a, b, 4 * 2.0 ** -23 * max(1., float(b.abs().max())), what))
    sel = torch.randperm(NSVF_H * NSVF_W, generator=torch.Generator().manual_seed(2))[:16]
    for idx in range(3):
        outs = []
        for fuse in (True, False):
            tr.pipeline.fuse = fuse
            outs.append(tr.pipeline(dict(tr._fetch_train_data(idx), select_inds=sel.clone())))
        tr.pipeline.fuse = True
        sync()
        assert sorted(outs[0]) == sorted(outs[1]) and 'global_domain_min' in outs[0] and outs[0]['global_domain_max'].device.type == dev.type
        for k in ('target_s', 'near', 'far', 'z_vals', 'rays_o'):
            same_bits(outs[0][k], outs[1][k], 'train item %d %s' % (idx, k))
        for k in ('rays_d', 'viewdirs', 'pts'):
            close(outs[1][k], outs[0][k], 'train item %d %s' % (idx, k))
    data = te[0]
    assert sorted(data) == ['global_domain_max', 'global_domain_min', 'idx', 'image', 'pose']
    pose = te.poses[int(te.i_test[0])]
    got = te.pipeline({'pose': pose})
    te.pipeline.fuse = False
    steps = te.pipeline({'pose': pose})
    te.pipeline.fuse = True
    sync()
    same_bits(got['rays_d'], g['nsvf.getrays.rays_d'].reshape(-1, 3), 'KilonerfGetRays against the reference GetRays: rays_d')
    same_bits(got['rays_o'], g['nsvf.getrays.rays_o'].reshape(-1, 3), 'KilonerfGetRays against the reference GetRays: rays_o')
    assert sorted(got) == sorted(steps) and got['src_shape'].tolist() == [NSVF_H, NSVF_W, 3]
    for k in ('rays_o', 'near', 'far', 'z_vals'):
        same_bits(got[k], steps[k], 'test frame %s' % k)
    for k in ('rays_d', 'viewdirs', 'pts'):
        close(steps[k], got[k], 'test frame %s' % k)
    # the pretrain configs' train list (the centre window during the first 10000 iterations) and a batching split over the same directory
    pre = pipelines.build_dataset(dict(type='KiloNerfDataset', cfg=nsvf_cfg(root, 'A'), pipeline=finetune_lists(sel_n=4, precrop_iters=10000)[0]), dict(device=dev))
    assert type(pre.pipeline.fused) is pipelines._FusedRun and len(pre) == 3
    win = torch.tensor([3, 0, 2, 1])                               # of the 2 x 4 centre window of a 6 x 8 frame: rows 2..3, columns 2..5
    outs = []
    for fuse in (True, False):
        pre.pipeline.fuse = fuse
        outs.append(pre.pipeline(dict(pre._fetch_train_data(1), select_inds=win.clone())))
    pre.pipeline.fuse = True
    sync()
    same_bits(outs[0]['target_s'], pre.images[int(pre.i_train[1])][[2, 2, 2, 2], [5, 2, 4, 3]], 'pretrain item: the window pixels')
    for k in ('target_s', 'near', 'far', 'z_vals', 'rays_o'):
        same_bits(outs[0][k], outs[1][k], 'pretrain item %s' % k)
    for k in ('rays_d', 'viewdirs', 'pts'):
        close(outs[1][k], outs[0][k], 'pretrain item %s' % k)
    pre.set_iter(10000)                                            # past the precrop: the whole frame
    assert tuple(pre[0]['rays_o'].shape) == (4, 3)
    bat = pipelines.build_dataset(dict(type='KiloNerfDataset', cfg=nsvf_cfg(root, 'A', is_batching=True, N_rand_per_sampler=16), pipeline=batching_list()), dict(device=dev))
    assert type(bat.pipeline.fused) is pipelines._FusedRun and len(bat) == 3 * NSVF_H * NSVF_W // 16 and tuple(bat.rays_rgb.shape) == (144, 3, 3)
    n = 0
    for idx in range(len(bat)):
        fused = bat[idx]
        bat.pipeline.fuse = False
        steps = bat[idx]
        bat.pipeline.fuse = True
        sync()
        assert sorted(fused) == sorted(steps) and 'global_domain_min' not in fused and tuple(fused['pts'].shape) == (16, 5, 3)
        for k in ('rays_o', 'rays_d', 'target_s', 'near', 'far', 'z_vals'):
            same_bits(fused[k], steps[k], 'batching item %d %s' % (idx, k))
        for k in ('viewdirs', 'pts'):
            close(steps[k], fused[k], 'batching item %d %s' % (idx, k))
        n += 1
    assert n == 9
    v = va[0]
    assert sorted(v) == ['global_domain_max', 'global_domain_min', 'images', 'poses', 'spiral_poses'] and tuple(v['poses'].shape) == (2, 4, 4)
    same_bits(v['spiral_poses'], g['nsvf.A.render_poses'], 'render_test selects the test poses')


def check_node_dataset(dev, tmp):
    """KiloNerfNodeDataset items are distill_examples of (seed, idx): inside their boxes, unit directions; the val set is generated once"""
    from xrnerf_amd import kilo_distill, pipelines
    root = write_nsvf(os.path.join(tmp, 'nsvf_A'), 'A')
    train_list, test_list = distill_lists()
    ds = pipelines.build_dataset(dict(type='KiloNerfNodeDataset', cfg=node_cfg(root, os.path.join(tmp, 'work')), pipeline=train_list), dict(device=dev, seed=9))
    assert len(ds) == 3 and ds.all_examples is None
    mins, maxs = ds._mins, ds._maxs
    for idx in range(len(ds)):
        item = ds[idx]
        ref = kilo_distill.distill_examples(mins, maxs, 32, 9, idx, pool_size=96)
        sync()
        assert sorted(item) == ['batch_examples', 'domain_maxs', 'domain_mins'] and tuple(item['batch_examples'].shape) == (3, 32, 6)
        same_bits(item['batch_examples'], ref, 'item %d' % idx)
        same_bits(item['domain_mins'], mins, 'domain_mins')
        ex = item['batch_examples']
        assert bool((ex[..., :3] >= mins[:, None]).all()) and bool((ex[..., :3] <= maxs[:, None]).all())
        within(ex[..., 3:].norm(dim=-1), torch.ones(3, 32), 4 * 2.0 ** -24, 'unit directions')
    assert not torch.equal(ds[0]['batch_examples'], ds[1]['batch_examples'])
    same_bits(ds[1]['batch_examples'], ds[1]['batch_examples'], 'an item is a function of (seed, idx)')
    val = pipelines.build_dataset(dict(type='KiloNerfNodeDataset', cfg=node_cfg(root, os.path.join(tmp, 'work'), 'val'), pipeline=test_list), dict(device=dev, seed=9))
    a, b = val[0], val[0]
    assert len(val) == 1 and tuple(a['batch_examples'].shape) == (3, 40, 6) and a['batch_examples'] is b['batch_examples']
    assert bool((a['batch_examples'][..., :3] >= mins[:, None]).all()) and bool((a['batch_examples'][..., :3] <= maxs[:, None]).all())


def check_end_to_end(dev, tmp):
    """BungeeNerfNetwork fed only by build_dataset + iterate on the generated directory: two training iterations and a validation frame"""
    import copy
    import xrnerf_amd
    from xrnerf_amd import bungee, pipelines
    root = write_google(os.path.join(tmp, 'google'))
    torch.manual_seed(3)
    cfg = copy.deepcopy(json.load(open(os.path.join(G, 'bungee_model_cfg.json')))['model'])
    cfg['mlp']['netwidth'], cfg['mlp']['cur_stage'], cfg['cfg']['N_importance'] = 32, 2, 9
    net = xrnerf_amd.build_network(cfg).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    train = bungee_dataset(dev, root, 2, S=9)
    val = bungee_dataset(dev, root, 2, mode='val', S=9)
    pipelines.SetValPipelineHook(valset=val).before_run(type('R', (), {'model': net})())
    n = 0
    for batch in pipelines.iterate(train):
        if n == 2:
            break
        assert tuple(batch['rays_o'].shape) == (1, N_RAND, 3) and batch['scale_code'].dtype == torch.int64
        outs = bungee.train_iteration(net, batch, opt)
        assert len(outs) == int(batch['scale_code'].max()) + 1 and all(np.isfinite(o['log_vars']['loss']) for o in outs)
        n += 1
    assert n == 2
    out = net.val_step(next(iter(pipelines.iterate(val))))
    assert len(out['rgbs']) == 2 and out['rgbs'][0].shape == (H, W, 3) and np.isfinite(out['rgbs'][0]).all() and len(out['spiral_rgbs']) == 2
