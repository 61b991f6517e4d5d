"""The shared bodies of the Mip-NeRF multiscale data tests (xrnerf_amd/multiscale.py, xrnerf_amd/csrc/xr_multiscale.hip).  Every check_*
takes the device, so tests/test_gpu_multiscale.py runs it on the MI355X and tests/test_emu_multiscale.py on the kernels' host build;
tests/test_multiscale_host.py runs the tensor and host paths.

Reference (tests/golden/ref_multiscale.npz, made by tests/golden/make_golden_multiscale.py): the reference's own load_rays_multiscale,
flatten, load_multiscale_data, MipMultiScaleSample and GetZvals, and the down2 / save / pix2cam lines of tools/convert_blender_data.py,
run on the scene generated here:
  * base_views(): three RGBA views of 12 x 16 with every alpha value from 0 to 255 among them, n_down = 3 (12 x 16, 6 x 8, 3 x 4: H = 3 is
    the smallest legal height), cameras with non-axis-aligned rotations;
  * fixture_meta(): the converter's metadata of those nine images with distinct near, far and lossmult per level, plus one 5 x 7 entry with
    an off-centre pix2cam of its own (an H / W swap cannot pass).
Bars: every ray output of the kernel and of the fused Compose equals the fixture bit for bit in fp32 (the generator asserts that the
float64 restatement tests/multiscale_restatement.py rounds to the same fp32 as the reference, element by element); every pyramid byte
and every packed fp32 pixel equals the reference's; metadata.json parses to == values."""
import ctypes as C
import copy
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')

import multiscale_restatement as RS  # noqa: E402

H0, W0, N_VIEWS, N_DOWN = 12, 16, 3, 3
N_SPLIT = {'train': 3, 'val': 1, 'test': 2}                 # the splits share the first views
ANGLE_X = 0.6911112070083618
N_DRAW, S_DRAW = 64, 5
RAY_KEYS = list(RS.RAY_KEYS)
ALL_KEYS = ['target_s'] + RAY_KEYS
EXTRA = dict(height=5, width=7, focal=9.3, cx=3.2, cy=2.9, label=3, near=1.7, far=5.3, lossmult=2.5)


# ------------------------------------------------------------------------------------------ the generated scene
def base_views():
    """[3, 12, 16, 4] uint8; the alpha plane of view 0 runs through 0 .. 191 and view 1's through 64 .. 255"""
    rng = np.random.default_rng(7)
    v = rng.integers(0, 256, (N_VIEWS, H0, W0, 4), dtype=np.uint8)
    v[0, :, :, 3] = np.arange(H0 * W0, dtype=np.uint8).reshape(H0, W0)
    v[1, :, :, 3] = (np.arange(H0 * W0) + 64).astype(np.uint8).reshape(H0, W0)
    return v


def cameras(n=N_VIEWS + 1):
    """[n, 4, 4] float64 camera-to-world matrices: a random rotation (QR of a normal matrix), the camera about 4 from the origin"""
    rng = np.random.default_rng(11)
    out = np.zeros((n, 4, 4))
    for m in out:
        q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
        m[:3, :3], m[:3, 3], m[3, 3] = q, 4.0 * q[:, 2] + rng.normal(0, 0.1, 3), 1.0
    return out


def extra_view():
    return np.random.default_rng(13).integers(0, 256, (EXTRA['height'], EXTRA['width'], 4), dtype=np.uint8)


def write_blender(root, views=None):
    """the base views (or `views`, one per split) as a Blender scene: transforms_{train,val,test}.json over ./train/r_<i>.png"""
    from PIL import Image
    os.makedirs(os.path.join(root, 'train'), exist_ok=True)
    cams = cameras()
    for i, v in enumerate(base_views() if views is None else views):
        Image.fromarray(v, 'RGBA').save(os.path.join(root, 'train', 'r_%d.png' % i))
    for split, n in N_SPLIT.items() if views is None else [(s, len(views)) for s in N_SPLIT]:
        frames = [{'file_path': './train/r_%d' % i, 'transform_matrix': cams[i].tolist()} for i in range(n)]
        with open(os.path.join(root, 'transforms_%s.json' % split), 'w') as fp:
            json.dump({'camera_angle_x': ANGLE_X, 'frames': frames}, fp)
    return root


def fixture_meta(conv_meta, zero_lossmult_level=None):
    """the rays fixture's metadata: the converter's train split with distinct per-level scalars, plus the 5 x 7 entry"""
    m = copy.deepcopy({k: list(v) for k, v in conv_meta.items()})
    for i, j in enumerate(m['label']):
        m['near'][i], m['far'][i], m['lossmult'][i] = 2.0 + 0.125 * j + 0.01 * (i // N_DOWN), 6.0 - 0.25 * j, 4.0 ** j + 0.5 * j
    e = EXTRA
    m['file_path'].append('images_train/extra.png')
    m['cam2world'].append(cameras()[N_VIEWS].tolist())
    for k in ('width', 'height', 'focal', 'label', 'near', 'far', 'lossmult'):
        m[k].append(e[k])
    m['pix2cam'].append([[1. / e['focal'], 0., -e['cx'] / e['focal']], [0., -1. / e['focal'], e['cy'] / e['focal']], [0., 0., -1.]])
    if zero_lossmult_level is not None:
        m['lossmult'] = [0.0 if j == zero_lossmult_level else v for v, j in zip(m['lossmult'], m['label'])]
    return m


_cache = {}


def gold():
    if 'gold' not in _cache:
        _cache['gold'] = np.load(os.path.join(G, 'ref_multiscale.npz'))
    return _cache['gold']


def conv_meta(split='train'):
    """the reference converter's metadata.json, parsed"""
    return json.loads(str(gold()['metadata_json']))[split]


def level_sizes():
    return [(H0 >> j, W0 >> j) for j in range(N_DOWN)]


def write_fixture_scene(root, zero_lossmult_level=None):
    """the multiscale scene the rays fixture was made on, from the stored converter bytes: all three splits hold the ten images"""
    from PIL import Image
    os.makedirs(os.path.join(root, 'images_train'), exist_ok=True)
    meta = fixture_meta(conv_meta(), zero_lossmult_level)
    saved, at = gold()['pyramid.bytes'], 0
    for name, h, w in list(zip(meta['file_path'], meta['height'], meta['width']))[:-1]:
        Image.fromarray(saved[at:at + h * w].reshape(h, w, 4), 'RGBA').save(os.path.join(root, name))
        at += h * w
    Image.fromarray(extra_view(), 'RGBA').save(os.path.join(root, meta['file_path'][-1]))
    with open(os.path.join(root, 'metadata.json'), 'w') as fp:
        json.dump({s: meta for s in ('train', 'val', 'test')}, fp, ensure_ascii=False, indent=4)
    return meta


def data_cfg(root, n_rand=16, num_samples=8):
    """the `data` dict of configs/mipnerf/mipnerf_multiscale.py with datadir pointed at `root` and N_rand / num_samples reduced"""
    base = dict(dataset_type='multiscale', datadir=root, white_bkgd=True, mode='train', N_rand_per_sampler=n_rand)
    train_pipeline = [dict(type='MipMultiScaleSample', keys=['target_s'] + RAY_KEYS, N_rand=n_rand),
                      dict(type='GetZvals', enable=True, lindisp=False, N_samples=num_samples + 1, randomized=True),
                      dict(type='ToTensor', keys=['target_s'] + RAY_KEYS)]
    test_pipeline = [dict(type='GetZvals', enable=True, lindisp=False, N_samples=num_samples + 1, randomized=False),
                     dict(type='ToTensor', keys=['image'] + RAY_KEYS)]
    return dict(train_loader=dict(batch_size=1, num_workers=1), train=dict(type='MipMultiScaleDataset', cfg=dict(base), pipeline=train_pipeline),
                val_loader=dict(batch_size=1, num_workers=0), val=dict(type='MipMultiScaleDataset', cfg=dict(base, mode='val'), pipeline=test_pipeline),
                test_loader=dict(batch_size=1, num_workers=0), test=dict(type='MipMultiScaleDataset', cfg=dict(base, mode='test'), pipeline=test_pipeline))


# ------------------------------------------------------------------------------------------ helpers
def MS():
    from xrnerf_amd import multiscale
    return multiscale


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    assert a.shape == b.shape and a.dtype == b.dtype, '%s: %r %s against %r %s' % (what, a.shape, a.dtype, b.shape, b.dtype)
    eq = (a.view(np.uint8) == b.view(np.uint8))
    assert eq.all(), '%s: the bits differ in %d of %d bytes (max |a - b| %.3e)' % (what, int((~eq).sum()), eq.size, np.nanmax(np.abs(a.astype(np.float64) - b)))


def to_dev(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def table_of(dev, meta=None):
    """the CameraTable of the fixture scene, from the fixture's own packed pixels"""
    meta = fixture_meta(conv_meta()) if meta is None else meta
    return MS().CameraTable({k: np.array(v) for k, v in meta.items()}, to_dev(dev)(gold()['table.target_s']), dev)


class Calls:
    """counts ops.ms_rays calls"""

    def __enter__(self):
        from xrnerf_amd import ops
        self.ops, self.saved, self.n = ops, ops.ms_rays, 0

        def counted(*a, **k):
            self.n += 1
            return self.saved(*a, **k)
        ops.ms_rays = counted
        return self

    def __exit__(self, *exc):
        self.ops.ms_rays = self.saved
        return False


# ------------------------------------------------------------------------------------------ rays
def check_frames(dev):
    """every full frame through the kernel's range selection, whole and in pieces: the reference's flattened tables, bit for bit"""
    from xrnerf_amd import ops
    g, t = gold(), table_of(dev)
    assert t.total == 3 * (192 + 48 + 12) + 35 and len(t) == 10
    for i, (h, w) in enumerate(t.sizes):
        lo, hi = int(t.offsets[i]), int(t.offsets[i + 1])
        whole = t.frame(i, want=ALL_KEYS)
        parts = [ops.ms_rays(t.cams, t.hw, t.prefix, t.sizes, images=t.images, image=i, first_pixel=p0, R=n)
                 for p0, n in ((0, 1), (1, w + 2), (w + 3, h * w - w - 3))]
        sync()
        for k in ALL_KEYS:
            assert tuple(whole[k].shape[:2]) == (h, w)
            same_bits(whole[k].reshape(h * w, -1), g['table.' + k][lo:hi], 'frame %d %s' % (i, k))
            same_bits(torch.cat([p[k] for p in parts], 0), g['table.' + k][lo:hi], 'frame %d in pieces %s' % (i, k))
        same_bits(t.z_row(i, S_DRAW, False).expand(h * w, S_DRAW), g['table.z_vals'][lo:hi], 'frame %d z row' % i)
        same_bits(t.image(i).reshape(-1, 3), g['table.target_s'][lo:hi], 'frame %d image view' % i)


def draw_args(dev):
    g = gold()
    return to_dev(dev)(g['draw'].astype(np.int64)), to_dev(dev)(g['t_rand'])


def check_draw(dev):
    """the training draw (first and last pixel of every image, rows H-2 and H-1, a duplicate) with and without randomised z_vals; a
    second call gives the same bits"""
    g, t = gold(), table_of(dev)
    idx, t_rand = draw_args(dev)
    d = g['draw']
    for i in range(len(t)):
        assert int(t.offsets[i]) in d and int(t.offsets[i + 1]) - 1 in d, 'the draw misses the first or last pixel of image %d' % i
    assert len(set(d.tolist())) < len(d), 'the draw holds no duplicate'
    plain = t.rays(idx)
    assert sorted(plain) == sorted(ALL_KEYS)
    got, again = t.rays(idx, S=S_DRAW, t_rand=t_rand), t.rays(idx, S=S_DRAW, t_rand=t_rand)
    det = t.rays(idx, S=S_DRAW, want=('z_vals',))
    sync()
    assert sorted(got) == sorted(ALL_KEYS + ['z_vals']) and sorted(det) == ['z_vals']
    for k in ALL_KEYS:
        assert tuple(got[k].shape) == (N_DRAW, g['train.' + k].shape[1])
        same_bits(plain[k], g['train.' + k], 'draw %s' % k)
        same_bits(got[k], g['train.' + k], 'draw with z %s' % k)
    same_bits(got['z_vals'], g['train.z_vals'], 'draw z_vals')
    same_bits(det['z_vals'], g['table.z_vals'][d], 'draw un-randomised z_vals')
    for k in got:
        same_bits(got[k], again[k], 'second run %s' % k)
    lin = t.rays(idx, S=S_DRAW, lindisp=True, want=('z_vals', 'near', 'far'))
    ref = RS.z_vals(host(lin['near']), host(lin['far']), S_DRAW, lindisp=True)
    assert np.abs(host(lin['z_vals']).astype(np.float64) - ref).max() <= 2 ** -22 * 6.0          # 1 / (..): a few fp32 roundings at z <= 6


def check_out_of_range(dev):
    """an index outside [0, total): that ray is NaN in every output, its neighbours are untouched"""
    g, t = gold(), table_of(dev)
    idx, t_rand = draw_args(dev)
    bad = idx.clone()
    bad[3], bad[17], bad[40] = -1, t.total, 2 ** 40
    got, full = t.rays(bad, S=S_DRAW, t_rand=t_rand), t.rays(idx, S=S_DRAW, t_rand=t_rand)
    sync()
    ok = [i for i in range(N_DRAW) if i not in (3, 17, 40)]
    for k in got:
        assert bool(torch.isnan(got[k][[3, 17, 40]]).all()), k
        same_bits(got[k][ok], full[k][ok], 'rays beside an out-of-range index: %s' % k)


def compose_list(n_rand=N_DRAW, S=S_DRAW, randomized=True):
    return [dict(type='MipMultiScaleSample', keys=['target_s'] + RAY_KEYS, N_rand=n_rand),
            dict(type='GetZvals', enable=True, lindisp=False, N_samples=S, randomized=randomized), dict(type='ToTensor', keys=['target_s'] + RAY_KEYS)]


def check_compose(dev):
    """[MipMultiScaleSample, GetZvals, ToTensor] over a camera table is ONE launch and the fixture's bits; fuse = False gives the same
    item from the sample's launch and GetZvals' tensor ops; the default draw stays inside the set and changes from item to item"""
    from xrnerf_amd import pipelines
    g, t = gold(), table_of(dev)
    idx, t_rand = draw_args(dev)
    for fuse in (True, False):
        comp = pipelines.Compose(compose_list())
        assert type(comp.fused).__name__ == 'MultiscaleRun' and (comp.fused.start, comp.fused.end) == (0, 2)
        comp.fuse = fuse
        with Calls() as calls:
            out = comp({'camera_table': t, 'ray_indices': idx.clone(), 't_rand': t_rand.clone()})
        sync()
        assert calls.n == 1 and sorted(out) == sorted(ALL_KEYS + ['z_vals']), (fuse, calls.n, sorted(out))
        for k in ALL_KEYS + ['z_vals']:
            assert isinstance(out[k], torch.Tensor) and out[k].dtype == torch.float32 and out[k].device.type == dev.type
            same_bits(out[k], g['train.' + k], 'compose fuse=%s %s' % (fuse, k))
    comp = pipelines.Compose(compose_list(n_rand=40, S=4))
    a, b = comp({'camera_table': t}), comp({'camera_table': t})
    sync()
    assert tuple(a['rays_o'].shape) == (40, 3) and tuple(a['z_vals'].shape) == (40, 4) and not bool(torch.isnan(a['rays_d']).any())
    assert not torch.equal(a['target_s'], b['target_s']) and bool((a['z_vals'][:, 1:] >= a['z_vals'][:, :-1]).all())
    assert bool((a['z_vals'] >= a['near']).all()) and bool((a['z_vals'] <= a['far']).all())


def check_tensor_sample(dev):
    """handed plain tensors, MipMultiScaleSample indexes every key with one draw, as the reference does"""
    g = gold()
    idx, t_rand = draw_args(dev)
    comp = MS().pipelines.Compose(compose_list())
    data = {k: to_dev(dev)(g['table.' + k]) for k in ALL_KEYS}
    with Calls() as calls:
        out = comp(dict(data, ray_indices=idx, t_rand=t_rand))
    sync()
    assert calls.n == 0 and sorted(out) == sorted(ALL_KEYS + ['z_vals'])
    for k in ALL_KEYS + ['z_vals']:
        same_bits(out[k], g['train.' + k], 'tensor sample %s' % k)


def check_existing_plans_unchanged():
    """every list of tests/pipeline_cases.py still plans as a _FusedRun with the same span; the second planner only takes what the first
    leaves"""
    import pipeline_cases as K
    from xrnerf_amd import pipelines
    for name, c in K.CASES.items():
        comp = pipelines.Compose([dict(s, **K.datainfo(c)) for s in K.pipeline_list(c)])
        assert type(comp.fused) is pipelines._FusedRun, name
        assert type(comp.transforms[comp.fused.start]).__name__ in ('GetRays', 'BatchSample'), name
        assert type(comp.transforms[comp.fused.end]).__name__ == ('GetZvals' if c['radius'] or not c['pts'] else 'GetPts'), name
        assert comp.fused is not None and pipelines._FusedRun.plan(comp.transforms).end == comp.fused.end
    assert pipelines.Compose([dict(type='DeleteUseless', keys=['a'])]).fused is None
    assert pipelines.Compose([dict(type='GetZvals', randomized=True)]).fused is None                    # a randomised test list is not a frame run
    assert pipelines.Compose(compose_list()[:1]).fused is None                                            # the sample without GetZvals
    assert pipelines.Compose([dict(type='MipMultiScaleSample', keys=['rays_o', 'pts'])] + compose_list()[1:]).fused is None


# ------------------------------------------------------------------------------------------ refusals
def check_refusals(dev):
    """-22 with a message, nothing launched, outputs untouched; R = 0 launches nothing; the wrapper's own refusals"""
    from xrnerf_amd import _lib, ops
    lib, t = _lib.load(), table_of(dev)
    idx, t_rand = draw_args(dev)
    out = {k: torch.full((N_DRAW, n), 7.0, device=dev) for k, n in (('rays_o', 3), ('rays_d', 3), ('viewdirs', 3), ('radii', 1), ('lossmult', 1), ('near', 1),
                                                                    ('far', 1), ('z_vals', S_DRAW), ('target_s', 3))}
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    base = dict(cams=p(t.cams), hw=p(t.hw), prefix=p(t.prefix), n=len(t), total=t.total, images=p(t.images), idx=p(idx), image=0, first=0, R=N_DRAW, S=S_DRAW,
                t_rand=p(t_rand), **{k: p(v) for k, v in out.items()})

    def call(**over):
        a = dict(base, **over)
        return lib.xr_ms_rays(a['cams'], a['hw'], a['prefix'], a['n'], a['total'], a['images'], a['idx'], a['image'], a['first'], a['R'], a['S'], 0, a['t_rand'],
                              *[a[k] for k in ops.MS_OUTPUTS], None)
    assert call(cams=None) == -22 and call(hw=None) == -22 and call(prefix=None) == -22
    msg = lib.last_errors() if hasattr(lib, 'last_errors') else lib.xr_last_error().decode()
    assert 'cams, hw and prefix are required' in msg, msg
    assert call(n=0) == -22 and call(total=0) == -22 and call(images=None) == -22
    assert call(idx=None, image=10) == -22 and call(idx=None, first=t.total - 3) == -22
    assert call(S=0) == -22 and call(S=0, z_vals=None) == -22                                     # t_rand still asks for S
    assert call(R=0) == 0
    sync()
    assert all(bool((v == 7).all()) for v in out.values()), 'a refused call wrote an output'
    assert call() == 0 and call(S=0, z_vals=None, t_rand=None) == 0 and call(images=None, target_s=None) == 0
    sync()
    assert all(not bool((v == 7).any()) for v in out.values())
    pyr = lambda base_t, N, H, W, Cn, nd, by, px: lib.xr_ms_pyramid(p(base_t), N, H, W, Cn, nd, 1, p(by), p(px), None)
    b = to_dev(dev)(base_views())
    by, px = torch.full((3 * 252, 4), 9, dtype=torch.uint8, device=dev), torch.full((3 * 252, 3), 7.0, device=dev)
    assert pyr(None, 3, 12, 16, 4, 3, by, px) == -22 and pyr(b, 3, 12, 16, 4, 3, None, None) == -22 and pyr(b, 0, 12, 16, 4, 3, by, px) == -22
    assert pyr(b, 3, 12, 16, 2, 3, by, px) == -22 and pyr(b, 3, 12, 16, 4, 0, by, px) == -22 and pyr(b, 3, 12, 16, 4, 9, by, px) == -22
    assert pyr(b, 3, 12, 16, 4, 4, by, px) == -22                                                  # 12 rows do not halve three times
    sync()
    assert bool((by == 9).all()) and bool((px == 7).all())
    # the wrapper
    empty = t.rays(idx[:0], S=S_DRAW, t_rand=t_rand[:0])
    assert tuple(empty['z_vals'].shape) == (0, S_DRAW) and tuple(empty['target_s'].shape) == (0, 3)
    for bad in (dict(idx=idx.int()), dict(idx=idx, image=0), dict(idx=None), dict(idx=idx, t_rand=t_rand[:, :4], S=S_DRAW), dict(idx=idx, want=('pts',)),
                dict(idx=None, image=10), dict(idx=None, image=9, first_pixel=30, R=6), dict(idx=idx, images=t.images[:-1])):
        with pytest.raises(_lib.XrError):
            ops.ms_rays(t.cams, t.hw, t.prefix, t.sizes, **dict(dict(images=t.images), **bad))
    with pytest.raises(_lib.XrError):
        ops.ms_rays(t.cams.float(), t.hw, t.prefix, t.sizes, idx=idx)
    with pytest.raises(_lib.XrError):
        ops.ms_pyramid(b.float(), 3)


def check_h2_raises(dev):
    """H = 2: the reference returns fewer radii than rays; refused with ValueError at every layer"""
    from xrnerf_amd import ops
    meta = {k: np.array(v) for k, v in fixture_meta(conv_meta()).items()}
    meta['height'] = meta['height'].copy()
    meta['height'][2] = 2
    with pytest.raises(ValueError):
        MS().CameraTable(meta, torch.zeros((1, 3)), dev)
    t = table_of(dev)
    with pytest.raises(ValueError):
        ops.ms_rays(t.cams, t.hw, t.prefix, [(2, 16)] + t.sizes[1:], idx=draw_args(dev)[0])
    with pytest.raises(ValueError):
        RS.frame_rays(meta['pix2cam'][0], meta['cam2world'][0], 2, 16, 1., 2., 6.)
    with pytest.raises(ValueError):
        MS()._frame_rays(meta['pix2cam'][0], meta['cam2world'][0], 2, 16, 1., 2., 6.)


# ------------------------------------------------------------------------------------------ the pyramid and the converter
def check_pyramid(dev):
    """every level's bytes and packed pixels are the reference converter's and loader's; RGB input and no white background as well; an
    odd base size raises"""
    from xrnerf_amd import ops
    g, base = gold(), base_views()
    for white, key in ((True, 'pyramid.pixels'), (False, 'pyramid.pixels_plain')):
        got = ops.ms_pyramid(to_dev(dev)(base), N_DOWN, white)
        sync()
        same_bits(got['bytes'], g['pyramid.bytes'], 'pyramid bytes')
        same_bits(got['pixels'], g[key], 'pyramid pixels white_bkgd=%s' % white)
    rgb = np.ascontiguousarray(base[:2, :8, :12, :3])                              # C = 3 takes the LAST channel (blue) as alpha, as the loader does
    got = ops.ms_pyramid(to_dev(dev)(rgb), 3, True)
    only = ops.ms_pyramid(to_dev(dev)(rgb), 3, True, want=('pixels',))
    sync()
    saved, loaded = zip(*[RS.pyramid(v, 3, True) for v in rgb])
    same_bits(got['bytes'], np.concatenate([b.reshape(-1, 3) for s in saved for b in s], 0), 'RGB pyramid bytes')
    same_bits(got['pixels'], np.concatenate([p.reshape(-1, 3) for s in loaded for p in s], 0), 'RGB pyramid pixels')
    same_bits(only['pixels'], got['pixels'], 'pixels alone')
    assert sorted(only) == ['pixels']
    for shape in ((1, 12, 18, 4), (1, 10, 16, 4), (1, 13, 16, 4)):
        with pytest.raises(ValueError):
            ops.ms_pyramid(torch.zeros(shape, dtype=torch.uint8, device=dev), 3)
    with pytest.raises(ValueError):
        RS.pyramid(np.zeros((10, 16, 4), np.uint8), 3)


def items_equal(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert tuple(a[k].shape) == tuple(b[k].shape) and a[k].dtype == b[k].dtype, (what, k)
            same_bits(a[k], b[k], '%s %s' % (what, k))
        else:
            assert a[k] == b[k], (what, k)


def check_converter(dev, tmp):
    """convert_blender_scene writes the reference converter's PNG bytes and a metadata.json that parses to == values; the dataset built in
    memory (from_blender) and the one read back from the written scene give identical items"""
    from PIL import Image
    ms, g = MS(), gold()
    src, out = write_blender(os.path.join(tmp, 'blender')), os.path.join(tmp, 'multiscale')
    res = ms.convert_blender_scene(src, out, N_DOWN, dev)
    sync()
    want = json.loads(str(g['metadata_json']))
    assert json.load(open(os.path.join(out, 'metadata.json'))) == want
    assert list(res['train'][0]) == list(want['train']) == list(ms.META_KEYS)
    for split in N_SPLIT:
        meta, packed = res[split]
        assert json.loads(json.dumps(meta)) == want[split] and packed.device.type == dev.type
        n = N_SPLIT[split] * 252
        same_bits(packed, g['pyramid.pixels'][:n], 'packed %s' % split)
        at = 0
        for name, h, w in zip(meta['file_path'], meta['height'], meta['width']):
            same_bits(np.array(Image.open(os.path.join(out, name))).reshape(-1, 4), g['pyramid.bytes'][at:at + h * w], name)
            at += h * w
    nodisk = ms.convert_blender_scene(src, None, N_DOWN, dev, splits=('test',))
    assert sorted(nodisk) == ['test'] and sorted(os.listdir(tmp)) == ['blender', 'multiscale']
    data = data_cfg(out, n_rand=24, num_samples=4)
    for split in ('train', 'test'):
        a = ms.pipelines.build_dataset(dict(data[split], device=dev, seed=5))
        b = ms.MipMultiScaleDataset.from_blender(data[split]['cfg'], data[split]['pipeline'], src, n_down=N_DOWN, device=dev, seed=5)
        assert len(a) == len(b) == N_SPLIT[split] * N_DOWN
        for i in (0, 4):
            torch.manual_seed(3)
            x = a[i]
            torch.manual_seed(3)
            y = b[i]
            sync()
            items_equal(x, y, 'round trip %s item %d' % (split, i))
    with pytest.raises(ValueError):
        ms.convert_blender_scene(src, None, 4, dev)


# ------------------------------------------------------------------------------------------ the dataset
def check_dataset(dev, tmp):
    """MipMultiScaleDataset over the fixture scene: train items (pinned draw) and every test frame are the fixture's bits, with the
    reference's keys and shapes; __len__ is n_examples in every mode"""
    from xrnerf_amd import pipelines
    g = gold()
    meta = write_fixture_scene(tmp)
    data = data_cfg(tmp, n_rand=N_DRAW, num_samples=S_DRAW - 1)
    ds = {k: pipelines.build_dataset(dict(data[k], device=dev)) for k in ('train', 'val', 'test')}
    assert [len(ds[k]) for k in ('train', 'val', 'test')] == [10, 10, 10] and ds['train'].n_examples == 10
    assert all(np.array_equal(ds['train'].meta[k], np.array(meta[k])) for k in meta)
    idx, t_rand = draw_args(dev)
    tr = ds['train']
    item = tr.pipeline(dict(tr._fetch_train_data(0), ray_indices=idx, t_rand=t_rand))
    sync()
    assert sorted(item) == sorted(ALL_KEYS + ['z_vals'])
    for k in item:
        same_bits(item[k], g['train.' + k], 'train item %s' % k)
    free = tr[0]
    assert sorted(free) == sorted(item) and tuple(free['z_vals'].shape) == (N_DRAW, S_DRAW) and not bool(torch.isnan(free['rays_d']).any())
    offs = np.concatenate([[0], np.cumsum(np.array(meta['height']) * np.array(meta['width']))])
    for mode in ('val', 'test'):
        for i in (0, 2, 5, 9):
            fr = ds[mode][i]
            sync()
            h, w = meta['height'][i], meta['width'][i]
            assert sorted(fr) == sorted(['image', 'idx', 'z_vals'] + RAY_KEYS) and fr['idx'] == i, sorted(fr)
            for k in RAY_KEYS + ['image', 'z_vals']:
                ref = g['table.' + ('target_s' if k == 'image' else k)][offs[i]:offs[i + 1]]
                assert tuple(fr[k].shape) == (h, w, ref.shape[1]) and fr[k].dtype == torch.float32 and fr[k].device.type == dev.type, (mode, i, k, tuple(fr[k].shape))
                same_bits(fr[k].reshape(h * w, -1), ref, '%s frame %d %s' % (mode, i, k))
    batched = next(iter(pipelines.iterate(ds['test'])))
    assert batched['idx'].tolist() == [0] and tuple(batched['rays_o'].shape) == (1, H0, W0, 3) and tuple(batched['z_vals'].shape) == (1, H0, W0, S_DRAW)
    return ds


def model_cfg():
    """configs/mipnerf/mipnerf_multiscale.py's `model` (tests/golden/mip_model_cfg.json) with a 4 x 64 MLP"""
    model = copy.deepcopy(json.load(open(os.path.join(G, 'mip_model_cfg.json')))['model'])
    model['mlp'].update(netdepth=4, netwidth=64, skips=[2])
    return model


class Runner:
    def __init__(self, model=None, outputs=None):
        self.model, self.outputs, self.iter = model, outputs, 0


def check_end_to_end(dev, tmp):
    """build_dataset on the config's three data dicts -> iterate -> MipNerfNetwork.train_step (three steps, finite loss, gradients),
    the loss applies lossmult (zeroing level 0's in the metadata changes it), val_step on a 3 x 4 frame in both phases, and
    TestHook(ndown=3) files frame idx under scale idx % 3 (on a 28 x 28 view converted in memory: the hook's SSIM window needs 7 rows)"""
    import xrnerf_amd
    from xrnerf_amd import evaluate, pipelines
    roots = [os.path.join(tmp, 'a'), os.path.join(tmp, 'b')]
    write_fixture_scene(roots[0])
    write_fixture_scene(roots[1], zero_lossmult_level=0)
    n_rand, S = 16, 9
    data = [data_cfg(r, n_rand=n_rand, num_samples=S - 1) for r in roots]
    train = pipelines.build_dataset(dict(data[0]['train'], device=dev))
    torch.manual_seed(0)
    net = xrnerf_amd.build_network(model_cfg()).to(dev)
    state = copy.deepcopy(net.state_dict())
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    losses = []
    for it, item in enumerate(pipelines.iterate(train)):
        assert sorted(item) == sorted(ALL_KEYS + ['z_vals']) and all(isinstance(v, torch.Tensor) and v.shape[0] == 1 and v.device.type == dev.type for v in item.values())
        assert tuple(item['z_vals'].shape) == (1, n_rand, S) and tuple(item['lossmult'].shape) == (1, n_rand, 1)
        out = net.train_step(item, opt)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()
        losses.append(float(out['log_vars']['loss']))
        assert out['num_samples'] == n_rand
        if it == 2:
            break
    assert len(losses) == 3 and np.isfinite(losses).all(), losses
    assert any(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in net.parameters())
    # lossmult: the same rays, draws and weights through both scenes
    net.load_state_dict(state)
    rng = np.random.default_rng(2)
    pick = to_dev(dev)(rng.integers(0, 791, n_rand).astype(np.int64))
    t_rand = to_dev(dev)(rng.uniform(0, 1, (n_rand, S)).astype(np.float32))
    seen = []
    for d in data:
        ds = pipelines.build_dataset(dict(d['train'], device=dev))
        item = ds.pipeline(dict(ds._fetch_train_data(0), ray_indices=pick.clone(), t_rand=t_rand.clone()))
        torch.manual_seed(1)
        seen.append((float(net.train_step({k: v[None] for k, v in item.items()}, opt)['log_vars']['loss']), item))
    assert bool((seen[1][1]['lossmult'] == 0).any()) and bool((seen[0][1]['lossmult'] > 0).all())
    same_bits(seen[0][1]['rays_d'], seen[1][1]['rays_d'], 'the same rays in both scenes')
    print('MS %s losses %r, with level 0 zeroed %r against %r' % (dev.type, losses, seen[1][0], seen[0][0]))
    assert np.isfinite(seen[0][0]) and np.isfinite(seen[1][0]) and seen[0][0] != seen[1][0]
    # validation and test frames
    val, test = (pipelines.build_dataset(dict(data[0][k], device=dev)) for k in ('val', 'test'))
    frames = list(pipelines.iterate(val))
    assert len(frames) == 10 and tuple(frames[2]['image'].shape) == (1, 3, 4, 3)
    res = net.val_step(frames[2])
    assert res['rgbs'][0].shape == (3, 4, 3) and res['gt_imgs'][0].shape == (3, 4, 3) and np.isfinite(res['rgbs'][0]).all()
    net.phase = 'test'
    out = net.val_step({k: (v[None] if isinstance(v, torch.Tensor) else torch.tensor([v])) for k, v in test[5].items()})
    assert out['idx'] == 5 and out['rgb'].shape == (3, 4, 3) and out['gt_img'].shape == (3, 4, 3)
    # TestHook's SSIM window is 7 wide: a 28 x 28 view converted in memory gives 28, 14 and 7 rows, one frame per scale
    blender = write_blender(os.path.join(tmp, 'c'), np.random.default_rng(5).integers(0, 256, (1, 28, 28, 4), dtype=np.uint8))
    test = MS().MipMultiScaleDataset.from_blender(data[0]['test']['cfg'], data[0]['test']['pipeline'], blender, n_down=N_DOWN, device=dev)
    hook = evaluate.TestHook(ndown=N_DOWN)
    hook.before_val_epoch(Runner(net))
    for i, item in enumerate(pipelines.iterate(test)):
        out = net.val_step(item)
        assert out['idx'] == i and out['rgb'].shape == (28 >> i, 28 >> i, 3) and out['gt_img'].shape == (28 >> i, 28 >> i, 3)
        before = [len(hook.psnr[s]) for s in range(N_DOWN)]
        hook.after_val_iter(Runner(net, out))
        assert [len(hook.psnr[s]) - before[s] for s in range(N_DOWN)] == [int(s == i % N_DOWN) for s in range(N_DOWN)]
    assert [len(hook.mse[s]) for s in range(N_DOWN)] == [1, 1, 1] and all(np.isfinite(hook.mse[s]).all() and np.isfinite(hook.ssim[s]).all() for s in range(N_DOWN))


# ------------------------------------------------------------------------------------------ header, table, recipe
def check_symbols(loaded=True):
    """the header, the ctypes table, the source and the build recipe name the same xr_ms_* entry points; the table is disjoint from every
    other and the pinned families are untouched"""
    from xrnerf_amd import _lib, build, ops
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_multiscale.h')).read()
    declared = set(re.findall(r'^(?:int|size_t) (xr_ms_\w+)\(', header, re.M))
    assert declared == set(_lib.MULTISCALE_SIGNATURES) == {'xr_ms_rays', 'xr_ms_pyramid'}
    for name, (res, args) in _lib.MULTISCALE_SIGNATURES.items():
        text = header[header.index(' %s(' % name):]
        assert text[:text.index(');')].count(',') + 1 == len(args), name
    others = [v for k, v in vars(_lib).items() if k.endswith('SIGNATURES') and k != 'MULTISCALE_SIGNATURES']
    assert len(others) >= 12 and not any(k.startswith('xr_ms_') for t in others for k in t)
    assert set(_lib.PIPELINE_SIGNATURES) == {'xr_pipe_ray_front'}
    for h in ('xrnerf_mi355.h', 'xrnerf_mi355_pipeline.h'):
        assert 'xr_ms_' not in open(os.path.join(ROOT, 'include', h)).read()
    assert build.SOURCES['xr_multiscale.hip'] == ['-ffp-contract=off']
    source = open(os.path.join(ROOT, 'xrnerf_amd', 'csrc', 'xr_multiscale.hip')).read()
    assert set(re.findall(r'extern "C" int (xr_\w+)\(', source)) == declared
    assert int(re.search(r'#define XR_MS_CAM_DOUBLES (\d+)u', header).group(1)) == ops.MS_CAM_DOUBLES
    assert int(re.search(r'#define XR_MS_MAX_DOWN (\d+)u', header).group(1)) == ops.MS_MAX_DOWN
    if loaded:
        lib = _lib.load()
        assert all(hasattr(lib, name) for name in declared) and ops.multiscale_kernels_available()
