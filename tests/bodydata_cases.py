"""The bodies of the human-data tests (xrnerf_amd/bodydata.py over xrnerf_amd/csrc/xr_bodydata.hip), shared by the three tiers:
tests/test_bodydata_host.py (no GPU), tests/test_emu_bodydata.py (the host build of the kernels) and tests/test_gpu_bodydata.py (the MI355X).
Also the generated scenes the fixture tests/golden/ref_bodydata.npz is made of (tests/golden/make_golden_bodydata.py imports them)."""
import ctypes as C
import os
import re

import numpy as np
import torch

import bodydata_restatement as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'ref_bodydata.npz')
S = 6                                   # samples per ray in the z_vals / pts cases
SCENES = ('oblique', 'axis', 'small')
# name -> (scene, sel_n).  300 crosses the sweep of 256; 'two' has stored draws whose first round holds rays that miss the box
TRAIN = {'t64': ('oblique', 64), 't300': ('oblique', 300), 'two': ('oblique', 48), 't1': ('axis', 1), 'small16': ('small', 16)}
RAY_KEYS = ('rays_o', 'rays_d', 'near', 'far', 'target_s')
_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(GOLD))
    return _gold


def BD():
    from xrnerf_amd import bodydata
    return bodydata


def _rot(axis, ang):
    axis = np.asarray(axis, float)
    axis = axis / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * (k @ k)


def scene(name):
    """a camera, a 40-vertex body, a prepared image and a mask.  'oblique': 24 x 32, a rotated camera; 'axis': R = I and an integer cx, so
    the centre column's x component is exactly 0 and takes the 1e-5 clamp; 'small': a 7 x 5 image of another size; 'miss': 'small' with the
    body moved out of view (no ray hits its box)"""
    base = 'small' if name == 'miss' else name
    rng = np.random.default_rng({'oblique': 3, 'axis': 4, 'small': 5}[base])
    verts = rng.uniform([-0.3, -0.5, -0.2], [0.3, 0.5, 0.2], (40, 3)).astype(np.float32)
    if base == 'oblique':
        H, W, R, K = 24, 32, _rot([0.3, 1.0, 0.2], 0.7), np.array([[40., 0, 15.3], [0, 41., 11.7], [0, 0, 1]])
    elif base == 'axis':
        H, W, R, K = 16, 20, np.eye(3), np.array([[30., 0, 10.], [0, 30., 8.], [0, 0, 1]])
    else:
        H, W, R, K = 7, 5, _rot([1.0, 0.2, -0.4], -0.5), np.array([[9., 0, 2.4], [0, 9.5, 3.3], [0, 0, 1]])
    if name == 'miss':
        verts = verts + np.float32(5.0) * np.array([1, 0, 0], np.float32)
    T = np.array([[0.05], [-0.03], [2.2]])
    img = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    msk = np.ones((H, W), np.uint8)
    msk[H // 3:H // 2, W // 3:W // 2] = 0
    msk[H // 2, W // 2] = 0                                              # the body list is a proper subset of the bound list
    img[msk == 0] = 0
    bounds = np.stack([np.min(verts, axis=0) - 0.05, np.max(verts, axis=0) + 0.05], axis=0)
    return dict(name=name, H=H, W=W, K=K, R=R, T=T, verts=verts, img=img, msk=msk, bounds=bounds)


def corners(s):
    return BD().box_corners_2d(s['bounds'], s['K'], np.concatenate([s['R'], s['T']], axis=1))


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    assert a.shape == b.shape and a.dtype == b.dtype, '%s: %r %s against %r %s' % (what, a.shape, a.dtype, b.shape, b.dtype)
    eq = (a.view(np.uint8) == b.view(np.uint8))
    assert eq.all(), '%s: the bits differ in %d of %d bytes' % (what, int((~eq).sum()), eq.size)


def to_dev(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def picture(dev, s):
    """the scene as a PreparedPicture on `dev` (the fixture's image and mask are prepared pictures already)"""
    up = to_dev(dev)
    return BD().PreparedPicture(up(s['img']), up(s['msk']), s['K'], s['R'], s['T'], img_path=s['name'])


def short_counter(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


class Calls:
    """counts the launches the fused run makes: ops.body_sample / body_points / body_frame / body_masks calls"""
    NAMES = ('body_sample', 'body_points', 'body_frame', 'body_masks', 'body_prepare')

    def __enter__(self):
        from xrnerf_amd import ops
        self.ops, self.saved, self.n = ops, {k: getattr(ops, k) for k in self.NAMES}, {k: 0 for k in self.NAMES}
        for k in self.NAMES:
            setattr(ops, k, self._counted(k))
        return self

    def _counted(self, k):
        def f(*a, **kw):
            self.n[k] += 1
            return self.saved[k](*a, **kw)
        return f

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(self.ops, k, v)
        return False


# ------------------------------------------------------------------------------------------ the prepared picture
def raw_picture():
    rng = np.random.default_rng(11)
    img8 = rng.integers(0, 256, (12, 16, 3), dtype=np.uint8)
    msk8 = (rng.uniform(0, 1, (6, 8)) > 0.3).astype(np.uint8) * 255       # another size: resized to the image by nearest
    K = np.array([[14., 0, 7.6], [0, 13., 6.2], [0, 0, 1]])
    return img8, msk8, K, np.array([-0.25, 0.08, 0.004, -0.003, 0.01])


def check_prepare(dev):
    """identity D copies bits; nonzero D, ratio 0.5, white_bkgd on and off against the float64 specification within DEPTH 2^-24 (values
    lie in [0, 1]); masks exactly; two runs give identical bytes"""
    from xrnerf_amd import ops
    img8, msk8, K, D = raw_picture()
    up = to_dev(dev)
    img, msk = ops.body_prepare(up(img8), up(msk8), K, np.zeros(5), 1, False)
    sync()
    want, wmsk = RS.prepare(img8, msk8, K, np.zeros(5), 1, False)
    exact = img8.astype(np.float32) / np.float32(255)
    exact[wmsk == 0] = 0
    same_bits(img, exact, 'identity image')
    same_bits(msk, wmsk, 'identity mask')
    tol = RS.PREPARE_DEPTH * 2.0 ** -24
    for ratio, white in ((0.5, False), (0.5, True), (1, True)):
        a, am = ops.body_prepare(up(img8), up(msk8), K, D, ratio, white)
        b, bm = ops.body_prepare(up(img8), up(msk8), K, D, ratio, white)
        sync()
        want, wmsk = RS.prepare(img8, msk8, K, D, int(round(1 / ratio)), white)
        same_bits(am, wmsk, 'mask %r' % ((ratio, white),))
        err = np.abs(host(a).astype(np.float64) - want).max()
        print('prepare ratio %s white %s: max error %.3e (bar %.3e)' % (ratio, white, err, tol))
        assert err <= tol, (ratio, white, err, tol)
        same_bits(a, b, 'second run image')
        same_bits(am, bm, 'second run mask')
        assert 0 < int(wmsk.sum()) < wmsk.size and (host(a)[wmsk == 0] == (1.0 if white else 0.0)).all()
        hp, hm = BD().host_prepare(img8, msk8, K, D, ratio, white)          # the path without the library: the same arithmetic in numpy
        same_bits(hm, wmsk, 'host mask')
        assert np.abs(hp.astype(np.float64) - want).max() <= tol
    for bad in (0.3, 0.75, 2):
        try:
            ops.body_prepare(up(img8), up(msk8), K, D, bad, False)
        except NotImplementedError as e:
            assert repr(bad) in str(e)
        else:
            raise AssertionError('ratio %r was not refused' % bad)


def check_host_prepare():
    img8, msk8, K, D = raw_picture()
    tol = RS.PREPARE_DEPTH * 2.0 ** -24
    for ratio, white, d in ((0.5, False, D), (0.5, True, D), (1, False, np.zeros(5))):
        hp, hm = BD().host_prepare(img8, msk8, K, d, ratio, white)
        want, wmsk = RS.prepare(img8, msk8, K, d, int(round(1 / ratio)), white)
        same_bits(hm, wmsk, 'host mask')
        assert hp.dtype == np.float32 and np.abs(hp.astype(np.float64) - want).max() <= (tol if d.any() else 2.0 ** -24)


def check_lists(dev):
    """mask bytes and both candidate lists equal the specification's exactly, twice"""
    from xrnerf_amd import ops
    for name in SCENES:
        s = scene(name)
        c = corners(s)
        same_bits(BD().bound_mask(c, s['H'], s['W']), RS.fill(c, s['H'], s['W']), 'host fill %s' % name)
        wb, wh = RS.lists(s['msk'], c)
        for _ in range(2):
            bound, body = ops.body_masks(to_dev(dev)(s['msk']), c)
            sync()
            same_bits(bound, wb, 'bound list %s' % name)
            same_bits(body, wh, 'body list %s' % name)
        assert 0 < len(wh) < len(wb) < s['H'] * s['W']
    # more than one workgroup per scan sweep row and a silhouette that leaves the picture
    s = scene('oblique')
    big = np.ones((40, 50), np.uint8)
    c = corners(s) * 2 - 7
    bound, body = ops.body_masks(to_dev(dev)(big), c)
    sync()
    wb, wh = RS.lists(big, c)
    same_bits(bound, wb, 'bound list 40 x 50')
    same_bits(body, wh, 'body list 40 x 50')


def train_args(dev, case):
    g, (name, n) = gold(), TRAIN[case]
    s = scene(name)
    pic = picture(dev, s)
    return s, pic, to_dev(dev)(g['train.%s.draws' % case]), n


def check_train(dev):
    """every training case: the kernel's outputs are the reference's, bit for bit, with z_vals / pts from the second launch and from
    the sampling workgroup itself; two runs give identical bytes; nothing ran short"""
    from xrnerf_amd import ops
    g = gold()
    for case in TRAIN:
        s, pic, draws, n = train_args(dev, case)
        bound, body = pic.lists(s['bounds'])
        cam, short = pic.cam(s['bounds']), short_counter(dev)
        t_rand = to_dev(dev)(g['train.%s.t_rand' % case])
        outs = [ops.body_sample(cam, pic.H, pic.W, pic.img, body, bound, draws, short, S=S, t_rand=t_rand, fused_points=f) for f in (False, True, False)]
        sync()
        for out in outs:
            assert sorted(out) == sorted(RAY_KEYS + ('z_vals', 'pts'))
            for k in RAY_KEYS + ('z_vals', 'pts'):
                same_bits(out[k], g['train.%s.%s' % (case, k)], 'train %s %s' % (case, k))
        plain = ops.body_sample(cam, pic.H, pic.W, pic.img, body, bound, draws, short)
        sync()
        assert sorted(plain) == sorted(RAY_KEYS) and int(short.item()) == 0
        same_bits(plain['near'], g['train.%s.near' % case], 'train %s near without samples' % case)


def short_case(dev):
    """the 'oblique' picture with an all-ones mask and draws that, after round 0's second half, point only at silhouette pixels whose
    rays miss the box"""
    s = scene('oblique')
    s['msk'] = np.ones_like(s['msk'])
    c = corners(s)
    wb, wh = RS.lists(s['msk'], c)
    o, d = RS.rays(s['K'], s['R'], s['T'], wb, s['W'])
    hit = RS.box(s['bounds'], o[None], d)[2]
    miss, hits = np.flatnonzero(~hit), np.flatnonzero(hit)
    assert len(miss) >= 4 and (wb == wh).all()
    n = 40
    draws = np.tile(miss[np.arange(n) % len(miss)], (RS.ROUNDS, 1)).astype(np.int64)
    draws[0, n // 2:] = hits[(7 * np.arange(n - n // 2)) % len(hits)] + 3 * len(wb)       # (mod len: the same entries)
    return s, wb, wh, draws, n


def check_short(dev):
    """an item that exhausts eight rounds: the survivors of round 0, a NaN tail, short_items == 1 (2 after the second item)"""
    from xrnerf_amd import ops
    s, wb, wh, draws, n = short_case(dev)
    want, rounds, per_round = RS.sample(s['K'], s['R'], s['T'], s['W'], s['bounds'], s['img'], wb, wh, draws, n)
    assert rounds == RS.ROUNDS and per_round == [n - n // 2] + [0] * 7
    pic, short = picture(dev, s), short_counter(dev)
    bound, body = pic.lists(s['bounds'])
    for i in (1, 2):
        out = ops.body_sample(pic.cam(s['bounds']), pic.H, pic.W, pic.img, body, bound, to_dev(dev)(draws), short, S=S, fused_points=(i == 2))
        sync()
        for k in RAY_KEYS:
            same_bits(out[k], want[k], 'short item %s' % k)
        assert int(short.item()) == i and np.isnan(host(out['z_vals'])[n - n // 2:]).all() and np.isnan(host(out['pts'])[n - n // 2:]).all()
        assert np.isfinite(host(out['pts'])[:n - n // 2]).all()
    # the host path handed the same table gives the same item
    sel = BD().NBSelectRays(sel_n=n)
    res = sel(BD().NBGetRays()(host_results(s, ray_draws=draws)))
    for k in RAY_KEYS:
        same_bits(res[k], want[k], 'short item on the host %s' % k)


def check_empty(dev):
    """an empty body list: ValueError before launch from the wrapper and from the fused run; the kernel itself refuses with -22 and
    leaves the outputs untouched"""
    from xrnerf_amd import _lib, ops
    s = scene('small')
    s['msk'] = np.zeros_like(s['msk'])
    pic, short = picture(dev, s), short_counter(dev)
    bound, body = pic.lists(s['bounds'])
    sync()
    assert body.numel() == 0 and bound.numel() > 0
    draws = torch.zeros((8, 4), dtype=torch.int64, device=dev)
    for call in (lambda: ops.body_sample(pic.cam(s['bounds']), pic.H, pic.W, pic.img, body, bound, draws, short),
                 lambda: compose(train_list(4))(fused_results(dev, s, pic, short, ray_draws=draws))):
        with Calls() as calls:
            try:
                call()
            except ValueError as e:
                assert 'empty candidate list' in str(e)
            else:
                raise AssertionError('an empty body list was not refused')
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    outs = [torch.full((4, w), 7.0, device=dev) for w in (3, 3, 1, 1, 3)]
    lib, cam = _lib.load(), pic.cam(s['bounds'])
    for lb, ln, seln in ((0, int(bound.numel()), 4), (int(bound.numel()), 0, 4), (1, 1, 0), (1, 1, ops.BODY_MAX_SEL + 1)):
        rc = lib.xr_body_sample(p(cam), pic.H, pic.W, p(pic.img), p(bound), lb, p(bound), ln, p(draws), seln, 0, None, *[p(o) for o in outs], None, None,
                                p(short), None)
        assert rc == -22, (lb, ln, seln, rc)
    # H W beyond int32 is refused by every entry point that indexes pixels with 32 bits
    mask, total, ws = torch.zeros(16, dtype=torch.uint8, device=dev), torch.full((1,), 7, dtype=torch.int32, device=dev), torch.zeros(64, dtype=torch.uint8, device=dev)
    assert lib.xr_body_frame_count(p(cam), 65536, 65536, p(mask), p(total), p(ws), 64, None) == -22
    assert lib.xr_body_sample(p(cam), 65536, 65536, p(pic.img), p(bound), 1, p(bound), 1, p(draws), 4, 0, None, *[p(o) for o in outs], None, None, p(short), None) == -22
    assert lib.xr_body_frame_count(p(cam), pic.H, pic.W, p(mask), p(total), p(ws), 0, None) == -12          # a workspace too small
    sync()
    assert all(bool((o == 7.0).all()) for o in outs) and int(short.item()) == 0 and int(total.item()) == 7


# ------------------------------------------------------------------------------------------ frames
def check_frames(dev):
    """every scene's whole frame: mask_at_box and the compacted survivors are the reference's select_all_rays, bit for bit; a frame no
    ray hits; without the colours; two runs identical"""
    from xrnerf_amd import ops
    g = gold()
    for name in SCENES + ('miss',):
        s = scene(name)
        pic = picture(dev, s)
        a = ops.body_frame(pic.cam(s['bounds']), pic.H, pic.W, pic.img)
        b = ops.body_frame(pic.cam(s['bounds']), pic.H, pic.W, pic.img)
        sync()
        assert a['mask_at_box'].dtype == torch.bool and tuple(a['mask_at_box'].shape) == (s['H'] * s['W'],)
        for k in RAY_KEYS + ('mask_at_box',):
            same_bits(a[k], g['frame.%s.%s' % (name, k)], 'frame %s %s' % (name, k))
            same_bits(a[k], b[k], 'frame %s %s, second run' % (name, k))
        M = int(g['frame.%s.mask_at_box' % name].sum())
        assert (M == 0) == (name == 'miss') and tuple(a['rays_o'].shape) == (M, 3)
        nc = ops.body_frame(pic.cam(s['bounds']), pic.H, pic.W)
        assert 'target_s' not in nc
        same_bits(nc['far'], g['frame.%s.far' % name], 'frame %s far without colours' % name)
        if M:
            zp = ops.body_points(a['rays_o'], a['rays_d'], a['near'], a['far'], S)
            sync()
            for k in ('z_vals', 'pts'):
                same_bits(zp[k], g['frame.%s.%s' % (name, k)], 'frame %s %s' % (name, k))


# ------------------------------------------------------------------------------------------ Compose
def cfg_of(mode='train', **kw):
    from xrnerf_amd import builder
    return builder.ConfigDict(dict(mode=mode, phase='train_pose', **kw))


def train_list(sel_n, perturb=True, pts=True):
    return [dict(type='NBGetRays', enable=True), dict(type='NBSelectRays', enable=True, sel_n=sel_n),
            dict(type='ToTensor', enable=True, keys=['rays_o', 'rays_d', 'target_s', 'near', 'far']),
            dict(type='GetZvals', enable=True, lindisp=False, N_samples=S), dict(type='PerturbZvals', enable=perturb), dict(type='GetPts', enable=pts),
            dict(type='DeleteUseless', enable=True, keys=['iter_n', 'cams', 'cam_inds', 'ims', 'cfg', 'data_root', 'idx', 'img_path', 'num_cams'])]


def test_list(sel_rgb=True):
    keys = ['rays_o', 'rays_d', 'near', 'far', 'mask_at_box'] + (['target_s'] if sel_rgb else [])
    return [dict(type='NBGetRays', enable=True), dict(type='NBSelectRays', enable=True, sel_all=True, sel_rgb=sel_rgb),
            dict(type='ToTensor', enable=True, keys=keys), dict(type='GetZvals', enable=True, lindisp=False, N_samples=S),
            dict(type='PerturbZvals', enable=False), dict(type='GetPts', enable=True),
            dict(type='DeleteUseless', enable=True, keys=['iter_n', 'cams', 'cam_inds', 'ims', 'cfg', 'data_root', 'idx', 'img_path', 'num_cams'])]


def compose(steps):
    from xrnerf_amd import pipelines
    return pipelines.Compose(steps)


def host_results(s, mode='train', **kw):
    """what LoadImageAndCamera + LoadSmplParam leave on the host path"""
    return dict(cfg=cfg_of(mode), img=s['img'].copy(), msk=s['msk'].copy(), cam_K=s['K'].copy(), cam_R=s['R'].copy(), cam_T=s['T'].copy(),
                smpl_verts=s['verts'].copy(), **kw)


def fused_results(dev, s, pic, short, mode='train', **kw):
    """what they leave with the frame store on the device"""
    return dict(cfg=cfg_of(mode), img=pic.img, msk=pic.msk, cam_K=s['K'].copy(), cam_R=s['R'].copy(), cam_T=s['T'].copy(), smpl_verts=s['verts'].copy(),
                body_picture=pic, short_items=short, **kw)


def check_compose(dev):
    """NBGetRays .. GetPts over a prepared picture plans as a BodyRun: two launches for a training item (one with fused_points), the
    fixture's bits; a frame is the count, the write and the points; fuse = False (numpy on the host) gives the same bits"""
    BDm, g = BD(), gold()
    case = 't300'
    s, pic, draws, n = train_args(dev, case)
    pic.lists(s['bounds'])                                                    # (made once per picture: not part of an item)
    t_rand = to_dev(dev)(g['train.%s.t_rand' % case])
    for fuse, fused_points in ((True, False), (True, True), (False, False)):
        comp = compose(train_list(n))
        assert type(comp.fused) is BDm.BodyRun and (comp.fused.start, comp.fused.end) == (0, 5)
        comp.fuse, comp.fused.fused_points = fuse, fused_points
        short = short_counter(dev)
        with Calls() as calls:
            out = comp(fused_results(dev, s, pic, short, ray_draws=draws.clone(), t_rand=t_rand.clone(), iter_n=0, idx=0))
        sync()
        want_calls = dict(body_sample=1 if fuse else 0, body_points=0, body_frame=0, body_masks=0, body_prepare=0)
        assert calls.n == want_calls, (fuse, calls.n)            # (body_sample makes its own second launch unless fused_points)
        assert 'cfg' not in out and 'idx' not in out and 'ray_draws' not in out and 't_rand' not in out
        for k in RAY_KEYS + ('z_vals', 'pts'):
            assert isinstance(out[k], torch.Tensor) and out[k].dtype == torch.float32
            same_bits(out[k], g['train.%s.%s' % (case, k)], 'compose fuse=%s %s' % (fuse, k))
    # the default draw: inside the lists, another one per item, nothing short
    comp, short = compose(train_list(50)), short_counter(dev)
    a = comp(fused_results(dev, s, pic, short))
    b = comp(fused_results(dev, s, pic, short))
    sync()
    assert tuple(a['pts'].shape) == (50, S, 3) and not bool(torch.isnan(a['pts']).any()) and not torch.equal(a['target_s'], b['target_s'])
    assert int(short.item()) == 0 and bool((a['z_vals'] >= a['near']).all()) and bool((a['z_vals'] <= a['far']).all())
    # frames
    for name, sel_rgb in (('oblique', True), ('small', False), ('miss', True)):
        s = scene(name)
        pic = picture(dev, s)
        for fuse in (True, False):
            comp = compose(test_list(sel_rgb))
            assert type(comp.fused) is BDm.BodyRun
            comp.fuse = fuse
            with Calls() as calls:
                out = comp(fused_results(dev, s, pic, short_counter(dev), mode='test'))
            sync()
            M = int(g['frame.%s.mask_at_box' % name].sum())
            if fuse:
                assert calls.n['body_frame'] == 1 and calls.n['body_points'] == 1 and calls.n['body_sample'] == 0
            assert ('target_s' in out) == sel_rgb and out['src_shape'].tolist() == [s['H'], s['W'], 3]
            for k in RAY_KEYS + ('mask_at_box',) + (('z_vals', 'pts') if M else ()):
                if k == 'target_s' and not sel_rgb:
                    continue
                assert isinstance(out[k], torch.Tensor)
                same_bits(out[k], g['frame.%s.%s' % (name, k)], 'frame compose fuse=%s %s %s' % (fuse, name, k))
            assert tuple(out['pts'].shape) == (M, S, 3)


def check_host_path():
    """the transforms on their own (numpy on the host) give the fixture: NBGetRays + NBSelectRays with the stored draws, every case and
    every frame; the skeleton transforms and the index conversion"""
    BDm, g = BD(), gold()
    for case, (name, n) in TRAIN.items():
        s = scene(name)
        comp = compose(train_list(n))
        comp.fuse = False
        out = comp(host_results(s, ray_draws=g['train.%s.draws' % case], t_rand=torch.from_numpy(g['train.%s.t_rand' % case]), iter_n=0))
        for k in RAY_KEYS + ('z_vals', 'pts'):
            same_bits(out[k], g['train.%s.%s' % (case, k)], 'host %s %s' % (case, k))
    for name in SCENES + ('miss',):
        s = scene(name)
        out = compose(test_list())(host_results(s, mode='test'))
        for k in RAY_KEYS + ('mask_at_box',):
            same_bits(out[k], g['frame.%s.%s' % (name, k)], 'host frame %s %s' % (name, k))
    same_bits(BDm.get_rigid_transformation(g['skel.poses'], g['skel.joints'], g['skel.parents']), g['skel.A'], 'get_rigid_transformation')
    res = BDm.CalculateSkelTransf()({'smpl_pose': g['skel.poses'].reshape(-1), 'joints': g['skel.joints'], 'parents': g['skel.parents']})
    same_bits(res['A'], g['skel.A'], 'CalculateSkelTransf')
    for phase, colour in (('train_pose', 5), ('novel_pose', 0)):
        res = BDm.AninerfIdxConversion()({'latent_idx': np.array([5]), 'cfg': _phase_cfg(phase)})
        assert res['bw_latent_idx'].tolist() == [5] and res['color_latent_idx'].tolist() == [colour] and res['latent_idx'].tolist() == [5]
    same_bits(g['idx.color_novel'], np.array([0]), 'the reference zeroes the colour index in novel_pose')


def _phase_cfg(phase):
    from xrnerf_amd import builder
    return builder.ConfigDict(dict(mode='train', phase=phase))


def check_plans():
    """the planner takes the config lists and nothing else; existing lists plan as before"""
    import multiscale_cases as MK
    BDm = BD()
    MK.check_existing_plans_unchanged()
    ani = [dict(type='CalculateSkelTransf', enable=True), dict(type='AninerfIdxConversion', enable=True)] + train_list(8)
    comp = compose([dict(type='LoadImageAndCamera', enable=True), dict(type='LoadSmplParam', enable=True)] + ani)
    assert type(comp.fused) is BDm.BodyRun and (comp.fused.start, comp.fused.end) == (4, 9)
    assert compose(train_list(8, perturb=False, pts=False)).fused.end == 3
    assert compose(train_list(8)[1:]).fused is None and compose(train_list(8)[:1]).fused is None
    assert compose([dict(type='NBGetRays'), dict(type='NBSelectRays'), dict(type='GetZvals', randomized=True)]).fused is None
    assert compose([dict(type='NBGetRays'), dict(type='NBSelectRays'), dict(type='GetZvals', lindisp=True)]).fused is None
    r = lambda t: repr(BDm.PIPELINES.build(dict(type=t)))
    assert r('LoadImageAndCamera') == 'LoadImageAndCamera:load the image and camera parameter'
    assert r('LoadSmplParam') == 'LoadSmplParam:load the SMPL parameter' and r('LoadCamAndSmplParam') == 'LoadCamAndSmplParam:load the Camera and SMPL parameters'
    assert r('CalculateSkelTransf') == 'CalculateSkelTransf:calculate the skeletal transformation' and r('AninerfIdxConversion') == 'AninerfIdxConversion:convert the aninerf index'
    assert r('NBGetRays') == "NBGetRays:get rays from pose and camera's params" and r('NBSelectRays') == 'NBSelectRays:random select rays when training'
    for name in ('NeuralBodyDataset', 'AniNeRFDataset'):
        assert name in BDm.DATASETS


# ------------------------------------------------------------------------------------------ a generated ZJU-shaped directory
N_FRAMES, N_CAMS, UNIT = 6, 3, 1.0


def img_path_to_smpl_idx(x):
    return int(os.path.basename(x).split('_')[1].split('.')[0])


def img_path_to_frame_idx(x):
    return int(os.path.basename(x).split('_')[1].split('.')[0]) - 1


def write_zju(root):
    """annots.npy, PNGs and masks via PIL, new_vertices, new_params and lbs: cameras 0..2 are the 'oblique', 'axis' and 'small' scenes
    (different picture sizes in one split); camera 1's mask folder is mask_cihp for frame 0"""
    from PIL import Image
    rng = np.random.default_rng(17)
    scenes = [scene(n) for n in SCENES]
    cams = {'K': [(s['K'] * np.array([[2.], [2.], [1.]])).tolist() for s in scenes],       # (halved again by ratio = 0.5)
            'R': [s['R'].tolist() for s in scenes], 'T': [(s['T'] * UNIT).tolist() for s in scenes],
            'D': [[[0.0]] * 5, [[-0.05], [0.01], [0.001], [-0.001], [0.0]], [[0.0]] * 5]}
    ims = []
    for f in range(N_FRAMES):
        names = []
        for c, s in enumerate(scenes):
            rel = os.path.join('Camera_%d' % c, 'f_%d.png' % (f + 1))
            names.append(rel)
            os.makedirs(os.path.join(root, 'Camera_%d' % c), exist_ok=True)
            Image.fromarray(rng.integers(0, 256, (s['H'] * 2, s['W'] * 2, 3), dtype=np.uint8)).save(os.path.join(root, rel))
            mdir = 'mask_cihp' if (c == 1 and f == 0) else 'mask'
            os.makedirs(os.path.join(root, mdir, 'Camera_%d' % c), exist_ok=True)
            m = np.ones((s['H'] * 2, s['W'] * 2), np.uint8) * 3
            m[:s['H'] // 2, :s['W'] // 2] = 0
            Image.fromarray(m).save(os.path.join(root, mdir, rel))
        ims.append({'ims': names})
    np.save(os.path.join(root, 'annots.npy'), {'cams': cams, 'ims': ims}, allow_pickle=True)
    for d in ('new_vertices', 'new_params', 'lbs'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    joints = rng.uniform([-0.3, -0.5, -0.15], [0.3, 0.5, 0.15], (24, 3)).astype(np.float32)
    for f in range(1, N_FRAMES + 1):
        np.save(os.path.join(root, 'new_vertices', '%d.npy' % f), scenes[0]['verts'] + np.float32(0.01 * f))
        np.save(os.path.join(root, 'new_params', '%d.npy' % f), {'Rh': rng.normal(0, 0.4, (1, 3)), 'Th': rng.normal(0, 0.1, (1, 3)),
                                                                  'poses': rng.normal(0, 0.2, (1, 72)), 'shapes': np.zeros((1, 10))}, allow_pickle=True)
    parents = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21])
    w = rng.uniform(0, 1, (40, 24)).astype(np.float32) ** 8
    np.save(os.path.join(root, 'lbs', 'joints.npy'), joints)
    np.save(os.path.join(root, 'lbs', 'parents.npy'), parents)
    np.save(os.path.join(root, 'lbs', 'weights.npy'), w / w.sum(1, keepdims=True))
    np.save(os.path.join(root, 'lbs', 'bigpose_vertices.npy'), scenes[0]['verts'])
    return root


def base_cfg(datadir, **kw):
    cfg = dict(dataset_type='blender', datadir=datadir, smpl_vertices_dir='new_vertices', smpl_params_dir='new_params', ratio=0.5, unit=UNIT,
               training_view=[0, 2], test_view=[1], num_train_frame=4, training_frame=[0, 4], frame_interval=1, val_frame_interval=2,
               white_bkgd=False, mode='train', img_path_to_smpl_idx=img_path_to_smpl_idx, img_path_to_frame_idx=img_path_to_frame_idx)
    cfg.update(kw)
    return cfg


def ani_lists(sel_n):
    extra = [dict(type='CalculateSkelTransf', enable=True), dict(type='AninerfIdxConversion', enable=True)]
    head = [dict(type='LoadImageAndCamera', enable=True), dict(type='LoadSmplParam', enable=True)]
    drop = ['iter_n', 'cams', 'cam_inds', 'ims', 'cfg', 'data_root', 'idx', 'img_path', 'num_cams', 'parents', 'joints']
    tr, te = train_list(sel_n), test_list()
    tr[-1] = te[-1] = dict(type='DeleteUseless', enable=True, keys=drop)
    return head + extra + tr, head + extra + te


def nb_lists(sel_n):
    head = [dict(type='LoadImageAndCamera', enable=True), dict(type='LoadSmplParam', enable=True)]
    return head + train_list(sel_n), head + test_list()


def check_dataset(dev, tmp):
    """build_dataset on the generated directory: selection, lengths, item keys and dtypes; on a device with the kernels the pictures are
    prepared once and the items come from the fused run; frames equal the host path's (rays bit for bit, colours within the bar)"""
    from xrnerf_amd import pipelines
    BDm = BD()
    root = write_zju(os.path.join(tmp, 'zju'))
    tr_list, te_list = nb_lists(20)
    train = pipelines.build_dataset(dict(type='NeuralBodyDataset', cfg=base_cfg(root), pipeline=tr_list), dict(device=dev, seed=3))
    test = pipelines.build_dataset(dict(type='NeuralBodyDataset', cfg=base_cfg(root, mode='test'), pipeline=te_list), dict(device=dev))
    assert len(train) == 8 and train.num_cams == 2 and train.cam_inds.tolist() == [0, 2] * 4 and train.ims[3] == os.path.join('Camera_2', 'f_2.png')
    assert len(test) == 2 and test.cam_inds.tolist() == [1, 1] and [os.path.basename(p) for p in test.ims] == ['f_1.png', 'f_3.png']
    novel = pipelines.build_dataset(dict(type='NeuralBodyDataset', cfg=base_cfg(root, phase='novel_pose', novel_pose_frame=[4, 6], test_view=[]), pipeline=tr_list),
                                    dict(device=dev))
    assert [os.path.basename(p) for p in novel.ims] == ['f_5.png'] * 2 + ['f_6.png'] * 2 and len(novel.spiral_poses) == 50
    native = train.store.native
    with Calls() as calls:
        items = [train[i] for i in (0, 1, 3, 1, 0)]
        train.set_iter(5)
    sync()
    if native:
        assert calls.n['body_prepare'] == 3 and calls.n['body_masks'] == 3 and calls.n['body_sample'] == 5 and train.store.prepared == 3
    keys = ['cam_K', 'cam_R', 'cam_T', 'far', 'latent_idx', 'near', 'pts', 'rays_d', 'rays_o', 'smpl_R', 'smpl_T', 'smpl_pose', 'smpl_verts', 'target_s', 'z_vals']
    for it, i in zip(items, (0, 1, 3, 1, 0)):
        assert sorted(it) == keys, sorted(it)
        assert all(isinstance(v, torch.Tensor) and v.device.type == dev.type for v in it.values())
        assert tuple(it['pts'].shape) == (20, S, 3) and it['latent_idx'].tolist() == [i // 2] and it['latent_idx'].dtype == torch.int64
        assert tuple(it['smpl_R'].shape) == (3, 3) and it['smpl_R'].dtype == torch.float32 and tuple(it['smpl_T'].shape) == (1, 3)
        assert bool(torch.isfinite(it['pts']).all()) and bool((it['near'] < it['far']).all())
    assert train.short_items == 0 and train.iter_n == 5
    Rm = host(items[0]['smpl_R']).astype(np.float64)
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(Rm) - 1) < 1e-6
    # val / test force idx = 0; the frame against the host path of the same directory (camera 1 has a nonzero D and a mask_cihp mask)
    cpu = pipelines.build_dataset(dict(type='NeuralBodyDataset', cfg=base_cfg(root, mode='test'), pipeline=te_list), dict(device='cpu'))
    a, b, c = test[1], test[0], cpu[0]
    sync()
    tol = RS.PREPARE_DEPTH * 2.0 ** -24
    for k in ('rays_o', 'rays_d', 'near', 'far', 'mask_at_box', 'z_vals', 'pts', 'smpl_verts', 'latent_idx'):
        same_bits(a[k], b[k], 'test item 1 is item 0: %s' % k)
        same_bits(a[k], c[k], 'frame against the host path: %s' % k)
    assert np.abs(host(a['target_s']).astype(np.float64) - host(c['target_s'])).max() <= tol and a['src_shape'].tolist() == [16, 20, 3]
    assert a['mask_at_box'].dtype == torch.bool and 0 < int(a['mask_at_box'].sum()) == a['rays_o'].shape[0]
    # the byte budget: one picture's worth keeps the newest only
    small = pipelines.build_dataset(dict(type='NeuralBodyDataset', cfg=base_cfg(root, cache_bytes=1), pipeline=tr_list), dict(device=dev))
    if native:
        small[0], small[1], small[0]
        assert len(small.store.entries) == 1 and small.store.prepared == 3
    for bad in (0.3, 0.75):
        try:
            pipelines.build_dataset(dict(type='NeuralBodyDataset', cfg=base_cfg(root, ratio=bad), pipeline=tr_list), dict(device=dev))
        except NotImplementedError as e:
            assert repr(bad) in str(e)
        else:
            raise AssertionError('ratio %r was not refused' % bad)
    # Animatable NeRF: the five extra keys
    atr, ate = ani_lists(12)
    ani = pipelines.build_dataset(dict(type='AniNeRFDataset', cfg=base_cfg(root, phase='train_pose'), pipeline=atr), dict(device=dev))
    it = ani[2]
    assert sorted(it) == sorted(keys + ['A', 'big_A', 'canonical_smpl_verts', 'smpl_bw', 'bw_latent_idx', 'color_latent_idx'])
    assert tuple(it['A'].shape) == (24, 4, 4) and it['A'].dtype == torch.float32 and tuple(it['big_A'].shape) == (24, 4, 4) and tuple(it['smpl_bw'].shape) == (40, 24)
    same_bits(it['big_A'], BDm.get_rigid_transformation(_bigpose(), ani.joints, ani.parents), 'big_A')
    np.save(os.path.join(root, 'lbs', 'template_pose.npy'), np.full(72, 0.1))
    ani2 = pipelines.build_dataset(dict(type='AniNeRFDataset', cfg=base_cfg(root, phase='novel_pose', novel_pose_frame=[4, 6], mode='test'), pipeline=ate), dict(device=dev))
    same_bits(ani2.big_A, BDm.get_rigid_transformation(np.full((24, 3), 0.1), ani2.joints, ani2.parents), 'big_A from template_pose.npy')
    os.remove(os.path.join(root, 'lbs', 'template_pose.npy'))
    it = ani2[0]
    assert it['color_latent_idx'].tolist() == [0] and it['bw_latent_idx'].tolist() == [0] and 'mask_at_box' in it
    # render mode: the spiral camera, no picture
    rcfg = base_cfg(root, mode='render', render_H=6, render_W=8, frame_idx=2, num_render_views=4, frame_idx_to_smpl_idx=lambda x: x + 1,
                    frame_idx_to_latent_idx=lambda x: x)
    rlist = [dict(type='LoadCamAndSmplParam', enable=True)] + test_list(sel_rgb=False)
    rlist[-1] = dict(type='DeleteUseless', enable=True, keys=['iter_n', 'cfg', 'data_root', 'idx', 'spiral_poses', 'K'])
    render = pipelines.build_dataset(dict(type='NeuralBodyDataset', cfg=rcfg, pipeline=rlist), dict(device=dev))
    it = render[1]
    assert len(render) == 4 and it['src_shape'].tolist() == [6, 8, 3] and 'target_s' not in it and it['latent_idx'].tolist() == [2]
    assert tuple(it['mask_at_box'].shape) == (48,) and it['rays_o'].shape[0] == int(it['mask_at_box'].sum()) and it['pts'].shape[1:] == (S, 3)
    return dict(train=train, test=test, ani=ani, root=root)


def _bigpose():
    p = np.zeros(72, np.float32)
    p[5], p[8] = np.deg2rad(30), np.deg2rad(-30)
    return p.reshape(-1, 3)


def check_end_to_end(dev, tmp):
    """build_dataset -> iterate -> NeuralBodyNetwork.train_step + val_step and AniNeRFNetwork.train_step at tiny sizes: finite losses"""
    import copy
    import json
    import xrnerf_amd
    from xrnerf_amd import pipelines
    root = write_zju(os.path.join(tmp, 'zju_e2e'))
    G = os.path.join(ROOT, 'tests', 'golden')
    torch.manual_seed(4)
    cfg = json.load(open(os.path.join(G, 'neuralbody_model_cfg.json')))['model']
    cfg['cfg']['smpl_embedder']['voxel_size'] = [0.05] * 3
    net = xrnerf_amd.build_network(copy.deepcopy(cfg)).to(dev)
    tr_list, te_list = nb_lists(16)
    train = pipelines.build_dataset(dict(type='NeuralBodyDataset', cfg=base_cfg(root, training_view=[2], training_frame=[0, 2]), pipeline=tr_list), dict(device=dev))
    val = pipelines.build_dataset(dict(type='NeuralBodyDataset', cfg=base_cfg(root, mode='val', test_view=[2]), pipeline=te_list), dict(device=dev))
    n = 0
    for item in pipelines.iterate(train):
        out = net.train_step(item, None)
        out['loss'].backward()
        assert np.isfinite(out['log_vars']['loss']) and out['num_samples'] == 16
        n += 1
    assert n == 2
    item = next(iter(pipelines.iterate(val)))
    out = net.val_step(item)
    assert out['rgb'].shape == (7, 5, 3) and np.isfinite(out['rgb']).all() and out['gt_img'].shape == (7, 5, 3)
    acfg = json.load(open(os.path.join(G, 'aninerf_model_cfg.json')))['model']
    anet = xrnerf_amd.build_network(copy.deepcopy(acfg)).to(dev)
    atr, _ = ani_lists(16)
    atrain = pipelines.build_dataset(dict(type='AniNeRFDataset', cfg=base_cfg(root, training_view=[2], training_frame=[0, 1], phase='train_pose'), pipeline=atr),
                                     dict(device=dev))
    out = anet.train_step(next(iter(pipelines.iterate(atrain))), None)
    out['loss'].backward()
    assert bool(torch.isfinite(out['loss']))


# ------------------------------------------------------------------------------------------ the header, the table, the recipe
def check_symbols(loaded=True):
    """the header, the ctypes table, the source and the build recipe name the same xr_body_* entry points; the table is disjoint from
    every other and the pinned families are untouched"""
    from xrnerf_amd import _lib, build, ops
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_bodydata.h')).read()
    declared = set(re.findall(r'^(?:int|size_t) (xr_body_\w+)\(', header, re.M))
    assert declared == set(_lib.BODYDATA_SIGNATURES) and len(declared) == 8
    for name, (res, args) in _lib.BODYDATA_SIGNATURES.items():
        text = header[header.index(' %s(' % name):]
        assert text[:text.index(');')].count(',') + 1 == len(args), name
    others = [v for k, v in vars(_lib).items() if k.endswith('SIGNATURES') and k != 'BODYDATA_SIGNATURES']
    assert len(others) >= 13 and not any(k.startswith('xr_body_') for t in others for k in t)
    assert set(_lib.PIPELINE_SIGNATURES) == {'xr_pipe_ray_front'} and set(_lib.MULTISCALE_SIGNATURES) == {'xr_ms_rays', 'xr_ms_pyramid'}
    for h in ('xrnerf_mi355.h', 'xrnerf_mi355_pipeline.h', 'xrnerf_mi355_multiscale.h'):
        assert 'xr_body_' not in open(os.path.join(ROOT, 'include', h)).read()
    for src in ('xr_pipeline.hip', 'xr_multiscale.hip'):
        assert 'xr_body_' not in open(os.path.join(ROOT, 'xrnerf_amd', 'csrc', src)).read()
    assert build.SOURCES['xr_bodydata.hip'] == ['-ffp-contract=off']
    source = open(os.path.join(ROOT, 'xrnerf_amd', 'csrc', 'xr_bodydata.hip')).read()
    assert set(re.findall(r'extern "C" (?:int|size_t) (xr_\w+)\(', source)) == declared
    for macro, value in (('CAM_DOUBLES', ops.BODY_CAM_DOUBLES), ('ROUNDS', ops.BODY_ROUNDS), ('MAX_SEL', ops.BODY_MAX_SEL), ('MAX_SHRINK', ops.BODY_MAX_SHRINK)):
        assert int(re.search(r'#define XR_BODY_%s (\d+)u' % macro, header).group(1)) == value
    if loaded:
        lib = _lib.load()
        assert all(hasattr(lib, name) for name in declared) and ops.bodydata_kernels_available()
