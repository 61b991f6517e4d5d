"""The shared bodies of the scene-pipeline tests (xrnerf_amd/pipelines.py, xrnerf_amd/csrc/xr_pipeline.hip).  Every check_* takes the
device, so tests/test_gpu_pipeline.py runs it on the MI355X and tests/test_emu_pipeline.py on the kernel's host build;
tests/test_pipeline_host.py runs the tensor-op path on host tensors.

Reference (tests/golden/ref_pipeline.npz, made by tests/golden/make_golden_pipeline.py): the reference's own create.py / augment.py /
transforms.py / compose.py run on the host in float32, with the draws (select_inds, t_rand) stored beside the outputs, and per output
`dev` = max|reference32 - restatement64| against tests/pipeline_restatement.py.
Bars: every output of the kernel and of the fused Compose is bit for bit the fixture, on the MI355X and on the host build alike: the
3-term torch.sum adds in index order and torch.norm accumulates acc = fma(x, x, acc), which reproduces the reference's bits, so BAR4 (the
outputs the issue would allow at 4 x the stored `dev`) is empty.
The tensor-op path is torch's own arithmetic on the device it runs on.  On host tensors it is the reference's, bit for bit.  On the GPU
torch.sum and torch.norm associate differently from the host's (the association the code does not state), so rays_d, viewdirs, radii
and what follows from them (pts; rays_o under ToNDC) of the DEVICE tensor-op path are compared at the issue's exception bar, 4 x the
stored `dev`, against the fixture and against the fused run; every other output (target_s, near, far, z_vals, src_shape) stays bit for bit
(DESIGN.md section 20)."""
import ctypes as C
import os
import re
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')

FX, FY, CX, CY = 7.3, 6.9, 2.2, 3.1          # fx != fy, an off-centre principal point
BAR4 = ()                                     # outputs compared at 4 x dev instead of bit for bit

_BASE = dict(H=6, W=5, chain='select', sel_n=7, iter_n=1000, precrop_iters=500, viewdirs=True, ndc=False, radius=False, near=2., far=6.,
             near_new=None, far_new=None, S=5, lindisp=False, perturb=True, randomized=False, pts=True, pose='orbit')
CASES = {
    'blender_train': {},
    'blender_precrop': dict(sel_n=3, iter_n=0),                                        # the 2 x 2 centre window
    'blender_test_S1': dict(chain='flatten', perturb=False, S=1),
    'blender_test_S2': dict(chain='flatten', perturb=False, S=2),
    'blender_test_S5': dict(chain='flatten', perturb=False, S=5),
    'blender_test_S64': dict(chain='flatten', perturb=False, S=64),
    'llff_ndc': dict(ndc=True, near=0., far=1., precrop_iters=0, pose='forward'),
    'llff_ndc_test': dict(chain='flatten', ndc=True, near=0., far=1., perturb=False, pose='forward'),
    'llff_lindisp': dict(lindisp=True, near=1.2, far=9.7, S=6, precrop_iters=0, pose='forward'),
    'mip_H3': dict(chain='flatten', H=3, radius=True, near=0., far=1., near_new=2., far_new=6., perturb=False, pts=False),
    'mip_H6': dict(radius=True, near=0., far=1., near_new=2., far_new=6., perturb=False, randomized=True, pts=False, precrop_iters=0),
    'mip_H6_test': dict(chain='flatten', radius=True, near=0., far=1., near_new=2., far_new=6., perturb=False, pts=False),
    'batch_sample': dict(chain='batch', N_rand=7, idx=1, lindisp=False, near=1.2, far=9.7),
}
CASES = {k: dict(_BASE, **v) for k, v in CASES.items()}
CASE_NAMES = tuple(CASES)


def intrinsics(c):
    return np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]])


def datainfo(c):
    """what SceneBaseDataset.get_info hands to every step"""
    return {'H': c['H'], 'W': c['W'], 'focal': FX, 'K': intrinsics(c), 'hwf': [c['H'], c['W'], FX], 'near': c['near'], 'far': c['far']}


def pipeline_list(c):
    """the config-shaped list of the case: the train_pipeline / test_pipeline of the three baseline configs"""
    bounds = dict(type='GetBounds', enable=True)
    if c['near_new'] is not None:
        bounds.update(near_new=c['near_new'], far_new=c['far_new'])
    tail = [dict(type='GetViewdirs', enable=c['viewdirs']), dict(type='ToNDC', enable=c['ndc']), bounds,
            dict(type='GetZvals', enable=True, lindisp=c['lindisp'], N_samples=c['S'], randomized=c['randomized'])]
    if not c['radius']:                                         # the mip configs end at GetZvals
        tail += [dict(type='PerturbZvals', enable=c['perturb']), dict(type='GetPts', enable=c['pts'])]
    if c['chain'] == 'select':
        head = [dict(type='Sample'), dict(type='DeleteUseless', keys=['images', 'poses', 'i_data', 'idx']),
                dict(type='ToTensor', enable=True, keys=['pose', 'target_s']), dict(type='GetRays', enable=True, include_radius=c['radius']),
                dict(type='SelectRays', enable=True, sel_n=c['sel_n'], precrop_iters=c['precrop_iters'], precrop_frac=0.5, include_radius=c['radius'])]
        return head + tail + [dict(type='DeleteUseless', enable=True, keys=['pose', 'iter_n'])]
    if c['chain'] == 'flatten':
        head = [dict(type='ToTensor', enable=True, keys=['pose']), dict(type='GetRays', enable=True, include_radius=c['radius']),
                dict(type='FlattenRays', enable=True, include_radius=c['radius'])]
        return head + tail + [dict(type='DeleteUseless', enable=True, keys=['pose'])]
    head = [dict(type='BatchSample', enable=True, N_rand=c['N_rand']), dict(type='DeleteUseless', keys=['rays_rgb', 'idx']),
            dict(type='ToTensor', enable=True, keys=['rays_o', 'rays_d', 'target_s'])]
    return head + tail + [dict(type='DeleteUseless', enable=True, keys=['iter_n'])]


def inputs(name):
    """the generated inputs of a case: pose [4,4], image [H,W,3], table [30,3,3] (fp32)"""
    c = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if c['pose'] == 'orbit':                                    # a camera on a sphere of radius 4 looking anywhere
        q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
        t = 4.0 * q[:, 2] + rng.normal(0, 0.1, 3)
    else:                                                       # forward-facing: small rotations about -z, no rays_d[2] near zero
        a = rng.normal(0, 0.08, 3)
        rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        q, t = rx @ ry, rng.normal(0, 0.3, 3)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3], pose[:3, 3] = q, t
    image = rng.uniform(0, 1, (c['H'], c['W'], 3)).astype(np.float32)
    table = np.stack([rng.normal(0, 1, (30, 3)), rng.normal(0, 1, (30, 3)) - [0, 0, 3.0], rng.uniform(0, 1, (30, 3))], 1).astype(np.float32)
    return pose, image, table


def first_dict(name, conv=lambda a: a):
    """the dict the chain starts from; conv places the arrays (numpy for the reference, device tensors here)"""
    c = CASES[name]
    pose, image, table = inputs(name)
    if c['chain'] == 'select':
        return {'poses': conv(pose[None]), 'images': conv(image[None]), 'i_data': np.array([0]), 'idx': 0, 'iter_n': c['iter_n']}
    if c['chain'] == 'flatten':
        return {'pose': conv(pose[:3, :4].copy())}
    return {'rays_rgb': conv(table), 'idx': c['idx'], 'iter_n': 0}


_cache = {}


def gold():
    if 'gold' not in _cache:
        _cache['gold'] = np.load(os.path.join(G, 'ref_pipeline.npz'))
    return _cache['gold']


def expected(name):
    """{key: (array, dev)} of the case's outputs, and its stored draws"""
    g = gold()
    pre = name + '.out.'
    outs = {k[len(pre):]: (g[k], float(g['%s.dev.%s' % (name, k[len(pre):])])) for k in g.files if k.startswith(pre)}
    draws = {k: g['%s.%s' % (name, k)] for k in ('select_inds', 't_rand') if '%s.%s' % (name, k) in g.files}
    return outs, draws


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    assert a.shape == b.shape and a.dtype == b.dtype, '%s: %r %s against %r %s' % (what, a.shape, a.dtype, b.shape, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), '%s: the bits differ (max |a - b| %.3e)' % (what, np.abs(a.astype(np.float64) - b).max())


def device_sum_outputs(dev, name):
    """the outputs of the DEVICE tensor-op path that depend on the GPU's torch.sum / torch.norm association (none on the host)"""
    if dev.type == 'cpu':
        return ()
    return ('rays_d', 'viewdirs', 'radii', 'pts') + (('rays_o',) if CASES[name]['ndc'] else ())


def against_fixture(dev, name, got, what, bar4=BAR4):
    """every stored output of the case: the same keys, shapes and dtypes, and the same bits (bar4 outputs: within 4 x dev); the distance
    of every output is printed before anything is asserted"""
    outs, _ = expected(name)
    lines = []
    for k, (ref, d) in outs.items():
        if k in got:
            err = float(np.abs(host(got[k]).astype(np.float64) - ref).max()) if ref.size else 0.0
            lines.append('%s %.3e (dev %.3e)' % (k, err, d))
    print('PIPE %s %s %s: %s' % (dev.type, what, name, '  '.join(lines)))
    assert sorted(got) == sorted(outs), (sorted(got), sorted(outs))
    for k, (ref, d) in outs.items():
        v = got[k]
        assert isinstance(v, torch.Tensor) and tuple(v.shape) == ref.shape and host(v).dtype == ref.dtype, (name, k, tuple(v.shape), v.dtype, ref.shape, ref.dtype)
        if k in bar4:
            assert float(np.abs(host(v).astype(np.float64) - ref).max()) <= 4 * d, (name, k, 4 * d)
        else:
            same_bits(v, ref, '%s %s %s' % (what, name, k))


def P():
    from xrnerf_amd import pipelines
    return pipelines


def to_dev(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Calls:
    """counts ops.pipe_ray_front calls"""

    def __enter__(self):
        from xrnerf_amd import ops
        self.ops, self.saved, self.n = ops, ops.pipe_ray_front, 0

        def counted(*a, **k):
            self.n += 1
            return self.saved(*a, **k)
        ops.pipe_ray_front = counted
        return self

    def __exit__(self, *exc):
        self.ops.pipe_ray_front = self.saved
        return False


def run_compose(dev, name, fuse=True, draws=True):
    """the case's config-shaped list through Compose on `dev` -> (result dict, kernel calls, the Compose)"""
    c = CASES[name]
    comp = P().Compose([dict(step, **datainfo(c)) for step in pipeline_list(c)])
    comp.fuse = fuse
    data = first_dict(name, to_dev(dev))
    if draws:
        for k, v in expected(name)[1].items():
            data[k] = to_dev(dev)(v)
    with Calls() as calls:
        out = comp(data)
    sync()
    return out, calls.n, comp


# ------------------------------------------------------------------------------------------ the fixture
def kernel_args(dev, name):
    """the arguments of ops.pipe_ray_front for a case, from its inputs and stored draws"""
    c = CASES[name]
    pose, image, table = inputs(name)
    _, draws = expected(name)
    up = to_dev(dev)
    near, far = (c['near'], c['far']) if c['near_new'] is None else (c['near_new'], c['far_new'])
    kw = dict(with_viewdirs=c['viewdirs'], ndc=c['ndc'], near=near, far=far, S=c['S'], lindisp=c['lindisp'])
    if 't_rand' in draws:
        kw['t_rand'] = up(draws['t_rand'])
    if c['chain'] == 'batch':
        kw['table'] = up(table[c['N_rand'] * c['idx']:c['N_rand'] * (c['idx'] + 1)])
    else:
        kw.update(c2w=up(pose[:3, :4].copy()), with_radii=c['radius'])
        if c['chain'] == 'select':
            h0, w0, nh, nw = P().SelectRays(sel_n=c['sel_n'], precrop_iters=c['precrop_iters'], H=c['H'], W=c['W'], K=None).window({'iter_n': c['iter_n']})
            ind = draws['select_inds'].astype(np.int64)
            kw.update(sel=up(((h0 + ind // nw) * c['W'] + w0 + ind % nw).astype(np.int32)), image=up(image))
    return (c['H'], c['W'], FX, FY, CX, CY), kw


def check_fixture_kernel(dev, name):
    """one ops.pipe_ray_front call reproduces the case; a second call gives the same bits"""
    from xrnerf_amd import ops
    c = CASES[name]
    args, kw = kernel_args(dev, name)
    got, again = ops.pipe_ray_front(*args, **kw), ops.pipe_ray_front(*args, **kw)
    sync()
    if not c['pts']:
        got.pop('pts'), again.pop('pts')
    if c['chain'] == 'flatten':
        got['src_shape'] = again['src_shape'] = torch.tensor((c['H'], c['W'], 3))
    against_fixture(dev, name, got, 'kernel')
    for k in got:
        same_bits(got[k], again[k], '%s second run %s' % (name, k))


def check_fixture_compose(dev, name, fused=True):
    """the config-shaped list through Compose: one launch when fused, none on the tensor-op path; the fixture's keys, shapes, dtypes, bits"""
    got, calls, comp = run_compose(dev, name, fuse=fused)
    assert comp.fused is not None and calls == (1 if fused else 0), (name, calls)
    assert 'select_inds' not in got and 't_rand' not in got
    against_fixture(dev, name, got, 'compose' if fused else 'tensor ops')


def check_fused_against_stepwise(dev, name):
    """the fused Compose against the same transforms called one by one on the device with the same draws"""
    fused, calls, comp = run_compose(dev, name)
    assert calls == 1
    c = CASES[name]
    data = first_dict(name, to_dev(dev))
    for k, v in expected(name)[1].items():
        data[k] = to_dev(dev)(v)
    with Calls() as counted:
        for t in comp.transforms:
            data = t(data)
    sync()
    assert counted.n == 0 and sorted(fused) == sorted(data), (sorted(fused), sorted(data))
    bar4, outs = device_sum_outputs(dev, name), expected(name)[0]
    print('PIPE %s fused - stepwise %s: %s' % (dev.type, name, '  '.join('%s %.3e (4 dev %.3e)' % (k, float((data[k].double() - fused[k].double()).abs().max()), 4 * outs[k][1])
                                                                    for k in data if k != 'src_shape')))
    for k, v in data.items():
        assert tuple(v.shape) == tuple(fused[k].shape) and v.dtype == fused[k].dtype and v.device.type == fused[k].device.type, (name, k)
        if k in bar4:
            assert float((v.double() - fused[k].double()).abs().max()) <= 4 * outs[k][1], (name, k)
        else:
            same_bits(fused[k], v, '%s fused against stepwise %s' % (name, k))


# ------------------------------------------------------------------------------------------ pieces, nullable outputs, R = 0
def check_pieces(dev):
    """sel = NULL: pieces of R = 1, 7 and 22 pixels concatenate to the whole frame (R = 30), which is the fixture's"""
    from xrnerf_amd import ops
    for name in ('blender_test_S5', 'mip_H6_test', 'llff_ndc_test'):
        args, kw = kernel_args(dev, name)
        whole = ops.pipe_ray_front(*args, **kw)
        parts = [ops.pipe_ray_front(*args, pix0=p0, R=n, **kw) for p0, n in ((0, 1), (1, 7), (8, 22))]
        sync()
        outs, _ = expected(name)
        for k, v in whole.items():
            same_bits(torch.cat([p[k] for p in parts], 0), v, '%s pieces %s' % (name, k))
            if k in outs:
                same_bits(v, outs[k][0], '%s whole frame %s' % (name, k))
        assert tuple(whole['rays_o'].shape) == (30, 3)
        with pytest.raises(Exception):
            ops.pipe_ray_front(*args, pix0=8, R=23, **kw)


def check_nullable_outputs(dev):
    """any subset of the outputs gives the bits of the full call"""
    from xrnerf_amd import ops
    args, kw = kernel_args(dev, 'blender_train')
    full = ops.pipe_ray_front(*args, **kw)
    for want in (('pts',), ('z_vals',), ('target_s',), ('rays_d', 'far'), ('rays_o', 'near', 'pts')):
        part = ops.pipe_ray_front(*args, want=want, **kw)
        sync()
        assert sorted(part) == sorted(set(want) | {'viewdirs'}), (want, sorted(part))
        for k in part:
            same_bits(part[k], full[k], 'want=%r %s' % (want, k))
    args, kw = kernel_args(dev, 'blender_test_S5')
    kw.update(S=0, with_viewdirs=False)
    assert sorted(ops.pipe_ray_front(*args, **kw)) == ['far', 'near', 'rays_d', 'rays_o']


def _raw(dev):
    """a raw xr_pipe_ray_front call on the blender_train case with sentinel-filled outputs: call(**overrides) -> rc"""
    from xrnerf_amd import _lib
    lib = _lib.load()
    (H, W, fx, fy, cx, cy), kw = kernel_args(dev, 'blender_train')
    R, S = 7, 5
    shapes = dict(rays_o=(R, 3), rays_d=(R, 3), viewdirs=(R, 3), radii=(R, 1), near=(R, 1), far=(R, 1), z_vals=(R, S), pts=(R, S, 3), target_s=(R, 3))
    out = {k: torch.full(s, 7.0, device=dev) for k, s in shapes.items()}
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    base = dict(c2w=p(kw['c2w']), fx=fx, fy=fy, H=H, W=W, sel=p(kw['sel']), pix0=0, R=R, image=p(kw['image']), Cn=3, table=None, vd=1, ndc=0, rad=0, S=S,
                t_rand=p(kw['t_rand']), **{k: p(v) for k, v in out.items()})
    base['radii'] = None
    keep = (kw, out)

    def call(**over):
        a = dict(base, **over)
        return lib.xr_pipe_ray_front(a['c2w'], a['fx'], a['fy'], cx, cy, a['H'], a['W'], a['sel'], a['pix0'], a['R'], a['image'], a['Cn'], a['table'], a['vd'],
                                     a['ndc'], a['rad'], -1.0, -1.0, 1.0, 2.0, 6.0, a['S'], 0, a['t_rand'], a['rays_o'], a['rays_d'], a['viewdirs'], a['radii'],
                                     a['near'], a['far'], a['z_vals'], a['pts'], a['target_s'], None)
    return call, out, keep, lib


def check_refusals_and_empty(dev):
    """-22 with a message on a null or out-of-range argument, nothing launched, every output untouched; R = 0 returns 0 and launches
    nothing; then the same buffers are written by a valid call"""
    from xrnerf_amd import _lib, ops
    call, out, keep, lib = _raw(dev)
    table = torch.zeros((7, 3, 3), device=dev)
    pt = C.c_void_p(table.data_ptr())
    assert call(c2w=None) == -22 and call(table=pt) == -22                                  # neither / both
    msg = lib.last_errors() if hasattr(lib, 'last_errors') else lib.xr_last_error().decode()
    assert 'exactly one of c2w / table' in msg, msg
    assert call(H=0) == -22 and call(W=0) == -22 and call(fx=0.0) == -22 and call(fy=float('nan')) == -22 and call(fx=float('inf')) == -22
    assert call(sel=None, pix0=24, R=7) == -22 and call(sel=None, pix0=31, R=0) == -22       # past the frame
    assert call(Cn=0) == -22 and call(Cn=5) == -22
    assert call(vd=0) == -22 and call(viewdirs=None) == -22                                  # switch and output go together
    assert call(rad=1) == -22 and call(rad=1, radii=out['radii'].data_ptr(), H=2, W=15) == -22
    assert call(S=0) == -22 and call(S=0, z_vals=None, pts=None) == -22                      # t_rand still asks for S
    assert call(c2w=None, table=pt) == -22 and call(c2w=None, table=pt, sel=None, image=None, rad=1, radii=out['radii'].data_ptr()) == -22
    assert call(R=0) == 0
    sync()
    assert all(bool((v == 7).all()) for v in out.values()), 'a refused call wrote an output'
    assert call(S=0, z_vals=None, pts=None, t_rand=None) == 0 and call(c2w=None, table=pt, sel=None, image=None) == 0 and call() == 0
    sync()
    assert all(not bool((v == 7).any()) for k, v in out.items() if k != 'radii') and bool((out['radii'] == 7).all())
    # the wrapper: empty selections return empty tensors; host tensors, wrong dtypes and shapes are refused in Python
    args, kw = kernel_args(dev, 'blender_train')
    empty = ops.pipe_ray_front(*args, **dict(kw, sel=kw['sel'][:0], t_rand=kw['t_rand'][:0]))
    assert tuple(empty['pts'].shape) == (0, 5, 3) and tuple(empty['target_s'].shape) == (0, 3)
    for bad in (dict(sel=kw['sel'].long()), dict(t_rand=kw['t_rand'][:, :4]), dict(image=kw['image'][:, :4]), dict(c2w=kw['c2w'].double()),
                dict(table=table), dict(c2w=None), dict(want=('radii',))):
        with pytest.raises(_lib.XrError):
            ops.pipe_ray_front(*args, **dict(kw, **bad))
    with pytest.raises(ValueError):
        ops.pipe_ray_front(2, 15, FX, FY, CX, CY, c2w=kw['c2w'], with_radii=True)
    # an index outside the frame: that ray is NaN, nothing is read, the others are the full call's
    sel = kw['sel'].clone()
    sel[2], sel[5] = 30, -1
    got, full = ops.pipe_ray_front(*args, **dict(kw, sel=sel)), ops.pipe_ray_front(*args, **kw)
    sync()
    ok = [0, 1, 3, 4, 6]
    for k in got:
        assert bool(torch.isnan(got[k][[2, 5]]).all()) or k in ('near', 'far', 'z_vals'), k
        same_bits(got[k][ok], full[k][ok], 'rays beside an out-of-frame index: %s' % k)


def check_default_draws(dev):
    """without stored draws: the selected pixels are distinct and, under precrop, inside the window; z stays inside its bin; the item
    differs from call to call"""
    pl = P()
    H, W, S = 6, 5, 5
    c = dict(CASES['blender_train'], sel_n=4)
    code = (torch.arange(H * W, dtype=torch.float32).reshape(H, W, 1) * torch.ones(3)).to(dev)          # pixel value = flat index
    pose = to_dev(dev)(inputs('blender_train')[0][:3, :4].copy())
    steps = [dict(s, **datainfo(c)) for s in pipeline_list(c)[3:]]
    for fuse in (True, False):
        comp = pl.Compose(steps)
        comp.fuse = fuse
        seen = []
        for iter_n, window in ((0, {11, 12, 16, 17}), (1000, set(range(H * W)))):
            out = comp({'pose': pose, 'target_s': code, 'iter_n': iter_n})
            sync()
            px = [int(v) for v in host(out['target_s'])[:, 0]]
            assert len(set(px)) == 4 and set(px) <= window, (fuse, iter_n, px)
            z = host(out['z_vals']).astype(np.float64)
            base = 2.0 + 4.0 * np.arange(S) / (S - 1)
            mids = .5 * (base[1:] + base[:-1])
            lo, hi = np.concatenate([base[:1], mids]), np.concatenate([mids, base[-1:]])
            assert ((z >= lo - 1e-6) & (z <= hi + 1e-6)).all() and tuple(z.shape) == (4, S)
            seen.append(host(out['z_vals']).copy())
        assert not np.array_equal(seen[0], seen[1])
    with pytest.raises(ValueError):                                          # 5 of the window's 4 pixels
        pl.Compose([dict(s, **datainfo(dict(c, sel_n=5))) for s in pipeline_list(dict(c, sel_n=5))[3:]])({'pose': pose, 'target_s': code, 'iter_n': 0})


def check_foreign_callable_is_not_fused(dev):
    """a callable that is not one of the transforms inside the run: no fusion, the tensor-op result"""
    pl = P()
    c = CASES['blender_test_S5']
    steps = [pl.PIPELINES.build(dict(s, **datainfo(c))) for s in pipeline_list(c)]
    seen = []
    steps.insert(4, lambda r: (seen.append(sorted(r)), r)[1])
    comp = pl.Compose(steps)
    assert comp.fused is None
    with Calls() as calls:
        got = comp(first_dict('blender_test_S5', to_dev(dev)))
    assert calls.n == 0 and seen
    assert pl.Compose([lambda r: None, steps[0]])({'pose': 1}) is None
    against_fixture(dev, 'blender_test_S5', got, 'unfused', bar4=device_sum_outputs(dev, 'blender_test_S5'))


def check_symbols():
    """the header, the ctypes table and the library name the same xr_pipe_* entry points; the table is disjoint from every other"""
    from xrnerf_amd import _lib, build, ops
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_pipeline.h')).read()
    declared = set(re.findall(r'^(?:int|size_t) (xr_pipe_\w+)\(', header, re.M))
    assert declared == set(_lib.PIPELINE_SIGNATURES) == {'xr_pipe_ray_front'}
    lib = _lib.load()
    for name, (res, args) in _lib.PIPELINE_SIGNATURES.items():
        text = header[header.index(' %s(' % name):]
        text = text[:text.index(');')]
        assert text.count(',') + 1 == len(args), name
        assert hasattr(lib, name), name
    others = [v for k, v in vars(_lib).items() if k.endswith('SIGNATURES') and k != 'PIPELINE_SIGNATURES']
    assert len(others) >= 11 and not any(set(t) & set(_lib.PIPELINE_SIGNATURES) for t in others)
    assert not any(k.startswith('xr_pipe_') for t in others for k in t)
    assert 'xr_pipe_' not in open(os.path.join(ROOT, 'include', 'xrnerf_mi355.h')).read()
    assert ops.pipeline_kernels_available()
    assert build.SOURCES['xr_pipeline.hip'] == ['-ffp-contract=off']
