"""GNR's body depth maps on the MI355X (xrnerf_amd/csrc/xr_gnr_raster.hip behind xrnerf_amd/gnr_raster.py): the z-buffer rasteriser, the
vertex visibility, depth_maps and their wiring into GnrNetwork.prepare_data, GnrRenderer and synthetic_scene.  The check_* bodies take
the device, so tests/test_emu_gnr_raster.py runs them on the kernels' host build and tests/test_gnr_raster_host.py on the tensor-op path.

References: tests/golden/ref_gnr_raster.npz -- the reference's own render.h, run serially (tests/golden/make_golden_gnr_raster.py) -- and
tests/gnr_raster_restatement.py, a serial float32 numpy restatement that the maker holds equal to it bit for bit.  Every comparison
here is exact (== on the bits of the floats): the kernels restate the reference's fp32 operations in its order, so there is no
tolerance to choose."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')

import gnr_raster_cases as K  # noqa: E402
import gnr_raster_restatement as RS  # noqa: E402
from xrnerf_amd import gnr_raster  # noqa: E402,F401  (every check here, and in the two files that run these bodies, is about this module)

CASE_NAMES = ('quads', 'degenerate_persp', 'degenerate_ortho', 'big', 'icosahedron', 'body')
NO_BACK_FACES = ('degenerate_persp', 'degenerate_ortho', 'big')
WHAT = ('index', 'coeff', 'visual', 'depth')


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a if a.dtype == np.bool_ else np.ascontiguousarray(a).view(np.uint8)


def same(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, '%s: shape %r, expected %r' % (what, got.shape, want.shape)
    assert np.array_equal(got, want), '%s: %d of %d bytes differ' % (what, int((got != want).sum()), got.size)


_cache = {}


def gold():
    if 'gold' not in _cache:
        _cache['gold'] = np.load(os.path.join(G, 'ref_gnr_raster.npz'))
    return _cache['gold']


def cases():
    if 'cases' not in _cache:
        _cache['cases'] = {c[0]: c for c in K.cases()}
    return _cache['cases']


def restated(v, tri, h, w, persp, double_face=False):
    """the restatement's (index, coeff, visual, depth) of one view, computed once per input"""
    v, tri = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(tri, np.int64)
    key = hashlib.sha256(v.tobytes() + tri.tobytes() + repr((v.shape, tri.shape, h, w, persp, double_face)).encode()).hexdigest()
    if key not in _cache:
        index, coeff, vis, zbuf = RS.zbuffer_forward(v, tri, h, w, persp, K.EPS, double_face)
        _cache[key] = (index, coeff, vis, RS.depth_of(zbuf, index))
    return _cache[key]


# ------------------------------------------------------------------------------------------ the fixture
def check_fixture(dev, name):
    """every stored array of the case, bit for bit; render_forward (one view, three values) is the same call; with double_face a case
    without back faces keeps its bits"""
    from xrnerf_amd import gnr_raster as R
    g, case = gold(), cases()[name]
    _, v, tri, h, w, persp = case
    digest = hashlib.sha256(np.ascontiguousarray(v).tobytes() + np.ascontiguousarray(tri).tobytes() + bytes([h, w, int(persp)])).hexdigest()
    assert digest == str(g[name + '.inputs_sha256']), 'this machine generates other inputs than the fixture\'s maker did: %s' % name
    tv, tt, _, _, _ = K.tensors(case, dev)
    out = R.rasterize(tv, tt, h, w, persp, K.EPS)
    sync()
    assert out[0].dtype == torch.int64 and out[1].dtype == torch.float32 and out[2].dtype == torch.bool and out[3].dtype == torch.float32
    for view in range(v.shape[0]):
        index = g['%s.%d.index' % (name, view)]
        want = (index, g['%s.%d.coeff' % (name, view)], g['%s.%d.visual' % (name, view)], RS.depth_of(g['%s.%d.zbuf' % (name, view)], index))
        for got, ref, what in zip(out, want, WHAT):
            same(got[view], ref, '%s view %d %s' % (name, view, what))
    if v.shape[0] == 1:
        three = R.render_forward(tv[0], tt, h, w, persp, K.EPS)
        sync()
        assert len(three) == 3
        for got, ref, what in zip(three, out, WHAT):
            same(got, ref[0], '%s render_forward %s' % (name, what))
    if name in NO_BACK_FACES:
        both = R.rasterize(tv, tt, h, w, persp, K.EPS, double_face=True)
        sync()
        for got, ref, what in zip(both, out, WHAT):
            same(got, ref, '%s double_face %s' % (name, what))


# ------------------------------------------------------------------------------------------ shapes the fixture lacks
def random_mesh(seed, n, f, h, w, persp, views=1):
    """vertices scattered over and around an h x w image at depths 1 .. 3 (one at z = 0, one far outside), random faces"""
    rng = np.random.default_rng(seed)
    px, py = rng.uniform(-3, w + 3, (views, n)), rng.uniform(-3, h + 3, (views, n))
    z = rng.uniform(1, 3, (views, n))
    if n > 4:
        z[:, 1] = 0.0
        px[:, 2] = 1e6
    v = np.stack([px * z, py * z, z] if persp else [px, py, z], -1).astype(np.float32)
    tri = rng.integers(0, n, (f, 3)).astype(np.int64)
    return v, tri


def against_restatement(dev, v, tri, h, w, persp, double_face=False, what=''):
    from xrnerf_amd import gnr_raster as R
    out = R.rasterize(torch.from_numpy(v).to(dev), torch.from_numpy(tri).to(dev), h, w, persp, K.EPS, double_face)
    sync()
    for view in range(v.shape[0]):
        want = restated(v[view], tri, h, w, persp, double_face)
        for got, ref, name in zip(out, want, WHAT):
            same(got[view], ref, '%s view %d %s' % (what, view, name))
    return out


def check_small_shapes(dev):
    """a 1 x 1 image; an image with no face in it (no faces at all, and faces that all lie outside); one vertex; one face"""
    one = np.array([[K._pv(-1, -1, 2.0), K._pv(-1, 3, 2.0), K._pv(3, -1, 2.0), K._pv(0.5, 0.5, 3.0), K._pv(0.25, 0.75, 1.0)]], np.float32)
    out = against_restatement(dev, one, np.array([[0, 1, 2]], np.int64), 1, 1, True, what='1x1')
    assert int(out[0][0, 0, 0]) == 0 and out[2][0].tolist() == [False, False, False, False, True]
    v, _ = random_mesh(1, 9, 1, 7, 5, True)
    out = against_restatement(dev, v, np.zeros((0, 3), np.int64), 7, 5, True, what='no faces')
    assert bool((out[0] == -1).all()) and bool((out[3] == 0).all()) and bool((out[1] == 0).all())
    far = np.array([[K._pv(40, 40, 2.0), K._pv(50, 40, 2.0), K._pv(40, 50, 2.0), K._pv(3.5, 3.5, 2.0)]], np.float32)
    out = against_restatement(dev, far, np.array([[0, 2, 1], [0, 1, 2]], np.int64), 7, 5, True, what='faces outside')
    assert bool((out[0] == -1).all()) and out[2][0].tolist() == [False, False, False, True]
    for persp in (True, False):
        single = np.array([[K._pv(2, 3, 1.5) if persp else [2, 3, 1.5]]], np.float32)
        out = against_restatement(dev, single, np.array([[0, 0, 0]], np.int64), 6, 6, persp, what='N = 1')
        assert int((out[0] >= 0).sum()) == 1 and int(out[0][0, 3, 2]) == 0
        v, tri = random_mesh(2, 12, 1, 9, 11, persp)
        against_restatement(dev, v, np.array([[3, 5, 4]], np.int64), 9, 11, persp, double_face=True, what='F = 1')


def check_random_meshes(dev, persp):
    """random triangles over shared vertices on 23 x 17 (box strides that are no multiple of the wave, faces that overlap, vertices
    under faces, off the image, at z = 0), single- and double-faced"""
    for seed, double_face in ((3, False), (4, True)):
        v, tri = random_mesh(seed, 60, 40, 17, 23, persp)
        out = against_restatement(dev, v, tri, 17, 23, persp, double_face, what='random persp=%s double_face=%s' % (persp, double_face))
        assert int((out[0] >= 0).sum()) > 50 and 0 < int(out[2].sum()) < 60


def check_crowded_pixel(dev):
    """70 vertices in one pixel (more than a wave), in front of and behind a triangle; 300 spread over a second one"""
    rng = np.random.default_rng(5)
    crowd = [K._pv(4 + rng.uniform(0.05, 0.95), 3 + rng.uniform(0.05, 0.95), z) for z in rng.uniform(1.2, 2.8, 70)]
    spread = [K._pv(rng.uniform(0, 12), rng.uniform(0, 10), rng.uniform(1.2, 2.8)) for _ in range(300)]
    v = np.array([[K._pv(0, 0, 2.0), K._pv(0, 9, 2.0), K._pv(11, 0, 2.0), K._pv(11, 9, 2.2)] + crowd + spread], np.float32)
    out = against_restatement(dev, v, np.array([[0, 1, 2], [3, 2, 1]], np.int64), 10, 12, True, what='crowded pixel')
    vis = out[2][0].cpu().numpy()
    assert 0 < int(vis[4:74].sum()) < 70


def check_views_slices_and_repeat(dev):
    """V = 3 views in one call = three calls; outputs as slices of larger buffers, the rest untouched; a second run gives the same bits"""
    from xrnerf_amd import gnr_raster as R
    from xrnerf_amd import ops
    h, w, n = 13, 19, 40
    v, tri = random_mesh(6, n, 30, h, w, True, views=3)
    tv, tt = torch.from_numpy(v).to(dev), torch.from_numpy(tri).to(dev)
    out = R.rasterize(tv, tt, h, w, True, K.EPS)
    again = R.rasterize(tv, tt, h, w, True, K.EPS)
    sync()
    for a, b, what in zip(out, again, WHAT):
        same(a, b, 'second run %s' % what)
    for view in range(3):
        single = R.rasterize(tv[view], tt, h, w, True, K.EPS)
        sync()
        for a, b, what in zip(out, single, WHAT):
            same(a[view], b, 'view %d alone %s' % (view, what))
    if not ops._on_device(tv):
        return                                                      # (the tensor-op path has no `out`)
    big = (torch.full((5, h, w), 77, dtype=torch.int64, device=dev), torch.full((5, h, w, 3), 7.5, device=dev),
           torch.ones((5, n), dtype=torch.bool, device=dev), torch.full((5, h, w), 7.5, device=dev))
    big[2][0] = False
    ops.gnr_raster_forward(tv, tt.to(torch.int32), h, w, True, False, K.EPS, out=tuple(b[1:4] for b in big))
    sync()
    for b, a, what in zip(big, out, WHAT):
        same(b[1:4], a, 'slice %s' % what)
    assert bool((big[0][0] == 77).all()) and bool((big[0][4] == 77).all()) and bool((big[1][0] == 7.5).all()) and bool((big[1][4] == 7.5).all())
    assert not bool(big[2][0].any()) and bool(big[2][4].all()) and bool((big[3][0] == 7.5).all()) and bool((big[3][4] == 7.5).all())


# ------------------------------------------------------------------------------------------ depth_maps
def scene():
    if 'scene' not in _cache:
        from xrnerf_amd.gnr_render import synthetic_scene
        _cache['scene'] = synthetic_scene()
    return _cache['scene']


def check_depth_maps(dev):
    """on the generated scene (64 x 64, four views with lens distortion): fed the projected vertices the device produced, the maps are
    the restatement's on those vertices, bit for bit; they lie inside the scene's dilated mask; every in-image vertex has a covered
    pixel in its 3 x 3 neighbourhood; mirrored faces give the same covered set with double_face"""
    from xrnerf_amd import gnr_raster as R
    sc = scene()
    d = lambda t: t.to(dev)
    verts, faces, calibs, persps = d(sc['smpl']['verts']), d(sc['smpl']['faces']), d(sc['calibs']), d(sc['persps'])
    pv = R.projected_vertices(verts, calibs, persps)
    maps = R.depth_maps(verts, faces, calibs, persps, 64, 64)
    sync()
    assert tuple(maps.shape) == (4, 1, 64, 64) and maps.dtype == torch.float32 and tuple(pv.shape) == (4, verts.shape[0], 3)
    pvh, got = pv.cpu().numpy(), maps.cpu().numpy()
    tri = sc['smpl']['faces'].numpy().astype(np.int64)
    for view in range(4):
        index, _, _, depth = restated(pvh[view], tri, 64, 64, True, True)
        same(got[view, 0], depth, 'depth_maps view %d' % view)
        covered = got[view, 0] > 0
        assert covered.sum() > 300 and not (covered & ~(sc['masks'][view, 0].numpy() > 0)).any(), 'the map leaves the dilated mask in view %d' % view
        px, py = np.floor(pvh[view, :, 0] / pvh[view, :, 2]).astype(np.int64), np.floor(pvh[view, :, 1] / pvh[view, :, 2]).astype(np.int64)
        on = (px >= 0) & (px < 64) & (py >= 0) & (py < 64)
        assert on.sum() > 600
        pad = np.pad(covered, 1)
        near = np.zeros((64, 64), bool)
        for dy in range(3):
            for dx in range(3):
                near |= pad[dy:dy + 64, dx:dx + 64]
        assert near[py[on], px[on]].all(), 'a vertex of view %d has no covered pixel around it' % view
        zs = pvh[view, :, 2]
        assert zs.min() - 1e-3 <= got[view, 0][covered].min() and got[view, 0][covered].max() <= zs.max() + 1e-3
    mirrored = R.depth_maps(verts, faces[:, [0, 2, 1]].contiguous(), calibs, persps, 64, 64)
    sync()
    assert np.array_equal(mirrored.cpu().numpy() > 0, got > 0)
    single = R.depth_maps(verts, faces, calibs, persps, 64, 64, double_face=False)
    sync()
    assert 0 < int((single > 0).sum()) <= int((maps > 0).sum())


# ------------------------------------------------------------------------------------------ wiring
def loader_batch(with_depth=None):
    """the loader's batch of GnrNetwork.prepare_data (every entry behind a batch dimension of 1) from the generated scene"""
    sc = scene()
    one = lambda t: t[None]
    smpl = sc['smpl']
    data = {'img': one(torch.cat([sc['images'], sc['images'][:1]], 0)), 'mask': one(torch.cat([sc['masks'], sc['masks'][:1]], 0)),
            'calib': one(torch.cat([sc['calibs'], sc['q_calib'][None]], 0)), 'persps': one(torch.cat([sc['persps'], sc['q_persps'][None]], 0)),
            'bbox': torch.tensor([[16, 48, 16, 48]]), 'center': one(sc['mesh_param']['center']), 'spatial_freq': torch.tensor([sc['mesh_param']['spatial_freq']]),
            'smpl_rot': smpl['rot'], 'smpl_verts': one(smpl['verts']), 'smpl_faces': one(smpl['faces']), 'smpl_t_verts': one(smpl['t_verts']),
            'smpl_t_faces': one(smpl['faces'])}
    if with_depth is not None:
        data['smpl_depth'] = one(with_depth)
    return data


def check_prepare_data(dev):
    """a batch without smpl_depth (or with an empty one) gets the body's own maps, a batch that brings its maps keeps them; the
    configuration's build_network is used unchanged"""
    import test_gpu_gnr_encoder as TE
    from xrnerf_amd import builder, gnr_raster as R
    torch.manual_seed(1)
    net = builder.build_network(TE.network_cfg())
    assert net.cfg.use_smpl_depth
    sc = scene()
    rank = 0 if dev.type == 'cuda' else 'cpu'                   # prepare_data's device: the GPU under test, else the host
    want = None
    for data in (loader_batch(), dict(loader_batch(), smpl_depth=torch.zeros((1, 0)))):
        out = net.prepare_data(net.cfg, data, rank)
        depth = out['smpl']['depth']
        tdev = depth.device
        if want is None:
            want = R.depth_maps(sc['smpl']['verts'].to(tdev), sc['smpl']['faces'].to(tdev), sc['calibs'].to(tdev), sc['persps'].to(tdev), 64, 64)
        sync()
        assert tuple(depth.shape) == (4, 1, 64, 64) and int((depth > 0).sum()) > 1000
        same(depth, want, 'prepare_data depth')
    own = torch.from_numpy(np.random.default_rng(2).uniform(0, 4, (4, 64, 64)).astype(np.float32))
    out = net.prepare_data(net.cfg, loader_batch(own), rank)
    same(out['smpl']['depth'], own[:, None], 'a batch\'s own smpl_depth')


def check_render_rays_on_raster_depth(dev):
    """render_rays on synthetic_scene(depth='raster'): finite, repeats its bits, the maps are depth_maps'; scan_depth_maps gives the
    layout inside_pts_vh samples; the default scene is unchanged"""
    import test_gpu_gnr_render as TR
    from xrnerf_amd import gnr_raster as R
    from xrnerf_amd.gnr_render import synthetic_scene
    sc = synthetic_scene(depth='raster')
    base = scene()
    assert torch.equal(sc['rays'], base['rays']) and torch.equal(sc['masks'], base['masks']) and not torch.equal(sc['smpl']['depth'], base['smpl']['depth'])
    same(sc['smpl']['depth'], R.depth_maps(base['smpl']['verts'], base['smpl']['faces'], base['calibs'], base['persps'], 64, 64), 'the scene\'s maps')
    with pytest.raises(ValueError):
        synthetic_scene(depth='other')
    mlp, ren = TR.built(dev, TR.load_params())
    d = lambda t: t.to(dev)
    smpl = {k: d(v) for k, v in sc['smpl'].items()}
    param = {'center': d(sc['mesh_param']['center']), 'spatial_freq': sc['mesh_param']['spatial_freq']}
    runs = []
    for _ in range(2):
        with torch.no_grad():
            rgb, depth = ren.render_rays(d(sc['rays']), d(sc['feats']), d(sc['images']), d(sc['masks']), d(sc['calibs']), smpl, param,
                                         persps=d(sc['persps']), q_persps=sc['q_persps'], is_train=True, t_rand=d(sc['t_rand']), noise=d(sc['noise']))
        sync()
        runs.append((rgb, depth))
    assert tuple(runs[0][0].shape) == (48, 6) and bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][1]).all())
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    scan = ren.scan_depth_maps([d(sc['smpl']['verts']), d(sc['smpl']['faces'])], d(sc['calibs']), d(sc['persps']))
    sync()
    same(scan, R.depth_maps(d(sc['smpl']['verts']), d(sc['smpl']['faces']), d(sc['calibs']), d(sc['persps']), 64, 64), 'scan_depth_maps')
    assert tuple(scan.shape) == (4, 1, 64, 64)
    inside, smpl_vis, scan_vis = ren.inside_pts_vh(d(sc['smpl']['verts']), d(sc['masks']), dict(smpl, scan_depth=scan), d(sc['calibs']), d(sc['persps']))
    assert smpl_vis is not None and smpl_vis.shape[1] == 4 and 0 < int(smpl_vis.sum()) < smpl_vis.numel()


def check_symbols():
    """the header, the ctypes table and the library name the same xr_gnr_raster_* entry points; the other GNR tables are as they were"""
    import re
    from xrnerf_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_gnr_raster.h')).read()
    declared = set(re.findall(r'^(?:int|size_t) (xr_gnr_raster_\w+)\(', header, re.M))
    assert declared == set(_lib.GNR_RASTER_SIGNATURES) and len(declared) == 2
    for name, (res, args) in _lib.GNR_RASTER_SIGNATURES.items():
        text = header[header.index(' %s(' % name):]
        text = text[:text.index(');')]
        assert text.count(',') + 1 == len(args), name
        assert hasattr(_lib.load(), name), name
    assert not any(k.startswith('xr_gnr_raster') for t in (_lib.GNR_SIGNATURES, _lib.GNR_RENDER_SIGNATURES, _lib.GNR_RECON_SIGNATURES) for k in t)


def check_refusals(dev):
    """eps < 0, the size limits and wrong dtypes are XrError; outputs of a refused C call stay untouched"""
    import ctypes as C
    from xrnerf_amd import _lib, gnr_raster as R, ops
    v, tri = random_mesh(7, 8, 4, 6, 6, True)
    tv, tt = torch.from_numpy(v).to(dev), torch.from_numpy(tri).to(dev)
    for bad in (dict(eps=-1e-6), dict(eps=float('nan')), dict(h=0), dict(w=0), dict(h=ops.GNR_RASTER_MAX_SIDE + 1), dict(h=32768, w=32768, views=2)):
        args = dict(h=6, w=6, eps=K.EPS, views=1)
        args.update(bad)
        with pytest.raises(_lib.XrError):
            R.rasterize(tv.expand(args['views'], -1, -1), tt, args['h'], args['w'], True, args['eps'])
    with pytest.raises(_lib.XrError):
        R.rasterize(tv.double(), tt, 6, 6, True)
    with pytest.raises(_lib.XrError):
        R.rasterize(tv, tt.float(), 6, 6, True)
    with pytest.raises(_lib.XrError):
        R.rasterize(tv[0, :, :2], tt, 6, 6, True)
    with pytest.raises(_lib.XrError):
        R.render_forward(tv, tt, 6, 6, True)
    if not ops._on_device(tv):
        return
    with pytest.raises(_lib.XrError):
        ops.gnr_raster_forward(tv, tt, 6, 6, True)                  # int64 faces
    with pytest.raises(_lib.XrError):
        ops.gnr_raster_forward(tv, tt.to(torch.int32), 6, 6, True, eps=-1.0)
    lib = _lib.load()
    assert ops.gnr_raster_workspace_bytes(1, 8, 6, 6) > 0 and ops.gnr_raster_workspace_bytes(4, 8, 32768, 32768) == 0
    assert ops.gnr_raster_workspace_bytes(1, 2 ** 31, 6, 6) == 0 and ops.gnr_raster_workspace_bytes(3, 2 ** 30, 6, 6) == 0
    p = lambda t: C.c_void_p(t.data_ptr())
    t32 = tt.to(torch.int32)
    index, coeff = torch.full((1, 6, 6), 7, dtype=torch.int64, device=dev), torch.full((1, 6, 6, 3), 7.0, device=dev)
    vis, depth = torch.ones((1, 8), dtype=torch.bool, device=dev), torch.full((1, 6, 6), 7.0, device=dev)
    ws = torch.zeros(ops.gnr_raster_workspace_bytes(1, 8, 6, 6) + 8, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 8
    call = lambda V=1, N=8, F=4, H=6, W=6, eps=1e-6, nbytes=ws.numel() - off, shift=0: lib.xr_gnr_raster_forward(
        p(tv), V, N, p(t32), F, H, W, 1, 0, eps, p(index), p(coeff), p(vis), p(depth), C.c_void_p(ws.data_ptr() + off + shift), nbytes, None)
    assert call(eps=-1e-6) < 0 and call(H=0) < 0 and call(W=40000) < 0 and call(V=4, H=32768, W=32768) < 0 and call(N=2 ** 31) < 0
    assert call(F=2 ** 32 - 1) < 0 and call(nbytes=64) < 0 and call(shift=4) < 0 and call(V=0) < 0
    sync()
    assert bool((index == 7).all()) and bool((coeff == 7).all()) and bool(vis.all()) and bool((depth == 7).all())
    assert call() == 0
    sync()
    assert not bool((index == 7).any())


# ------------------------------------------------------------------------------------------ the MI355X
@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from xrnerf_amd import ops
    assert ops.gnr_raster_kernels_available(), 'the library has no xr_gnr_raster entry points'
    yield torch.device('cuda')


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_fixture_cases_bit_for_bit(dev, name):
    check_fixture(dev, name)


@pytest.mark.gpu
def test_one_pixel_no_face_one_vertex_one_face(dev):
    check_small_shapes(dev)


@pytest.mark.gpu
@pytest.mark.parametrize('persp', (True, False))
def test_random_meshes_equal_the_restatement(dev, persp):
    check_random_meshes(dev, persp)


@pytest.mark.gpu
def test_more_than_a_wave_of_vertices_in_one_pixel(dev):
    check_crowded_pixel(dev)


@pytest.mark.gpu
def test_views_in_one_call_output_slices_and_repeatability(dev):
    check_views_slices_and_repeat(dev)


@pytest.mark.gpu
def test_depth_maps_of_the_generated_scene(dev):
    check_depth_maps(dev)


@pytest.mark.gpu
def test_prepare_data_builds_or_keeps_the_depth_maps(dev):
    check_prepare_data(dev)


@pytest.mark.gpu
def test_render_rays_on_rasterised_depth_and_scan_depth_maps(dev):
    check_render_rays_on_raster_depth(dev)


@pytest.mark.gpu
def test_header_table_and_library_agree(dev):
    check_symbols()


@pytest.mark.gpu
def test_refusals(dev):
    check_refusals(dev)
    from xrnerf_amd import _lib, ops
    v, tri = random_mesh(7, 8, 4, 6, 6, True)
    with pytest.raises(_lib.XrError):                               # host tensors handed to ops.*: there is no quiet CPU run
        ops.gnr_raster_forward(torch.from_numpy(v), torch.from_numpy(tri).to(torch.int32), 6, 6, True)
