"""GNR body-shape queries on the MI355X (xrnerf_amd/csrc/xr_gnr.hip behind xrnerf_amd/gnr.py).  The check_* bodies take the device, so
tests/test_emu_gnr.py runs the same bodies on the kernels' host build.

Reference: tests/golden/ref_gnr.npz -- the reference's own mesh_grid kernels compiled for the host and run serially through its own
MeshGridSearcher, and its own GnrRenderer.make_nerf_input (tests/golden/make_golden_gnr.py).  The reference's kernels are the
specification, quirks included; brute force is not the oracle.

Bars.  Structure (tri_num, tri_idx): exact, and a second build repeats the bits.  Nearest faces and signs: exact.  near_pts and coeff:
bitwise -- every operation is a correctly rounded float32 + - x /, a compare or a floor, with contraction off.  Embedding: per output
column 4 x the deviation of the reference's float32 run from its float64 run (floor 2^-22 of the column's maximum), the rule of
test_gpu_neuralbody.held(); alpha_smpl exact.  Every check prints its worst figure next to the bar."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')

STRUCT_CASES = ('one_face', 'spanning', 'm0', 'm3')       # F = 1, a triangle across the whole grid, F = 20, F = 1280
QUERY_N = (1, 63, 65, 1000)
FLOOR = 2.0 ** -22


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_gnr.npz'))


_cache = {}


def case(gold, key):
    """the stored case `key` ('m3' / 'm0'): (mesh dict, queries [nq,3]) on the host, generated once"""
    if key not in _cache:
        from xrnerf_amd.gnr import synthetic_mesh, synthetic_queries
        mesh = synthetic_mesh(int(gold[key + '.subdivisions']), int(gold[key + '.seed']))
        _cache[key] = (mesh, synthetic_queries(mesh, int(gold[key + '.queries']), int(gold[key + '.seed'])))
    return _cache[key]


def other_mesh(name):
    """meshes the fixture does not store -> (verts [V,3] float32, faces [F,3] int32)"""
    from xrnerf_amd.gnr import synthetic_mesh
    if name == 'one_face':
        return torch.tensor([[0.1, 0.2, 0.3], [1.3, 0.4, 0.9], [0.5, 1.7, 1.1]]), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    m = synthetic_mesh(1, 3)                              # 42 vertices: a grid of a few cells per axis
    v = m['verts']
    lo, hi = v.min(0)[0], v.max(0)[0]
    extra = torch.stack([lo, torch.stack([hi[0], hi[1], lo[2]]), hi])          # a triangle from corner to corner of the box
    verts = torch.cat([v, extra])
    faces = torch.cat([torch.tensor([[42, 43, 44]], dtype=torch.int32), m['faces'][:7]])
    return verts, faces


def searcher_for(dev, verts, faces):
    from xrnerf_amd.gnr import MeshGridSearcher
    return MeshGridSearcher(verts.to(dev), faces.to(dev))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


# ------------------------------------------------------------------------------------------ structure
def check_structure(dev, gold, name):
    import gnr_restatement as RS
    from xrnerf_amd import gnr, ops
    assert ops.gnr_kernels_available()
    if name in ('m0', 'm3'):
        mesh, _ = case(gold, name)
        verts, faces = mesh['verts'], mesh['faces']
    else:
        verts, faces = other_mesh(name)
    s = searcher_for(dev, verts, faces)
    tn, ti = s.tri_num.cpu().numpy(), s.tri_idx.cpu().numpy()
    assert tn.dtype == np.int32 and ti.dtype == np.int32
    if name in ('m0', 'm3'):
        assert np.array_equal(bits(s.step.cpu().numpy()), bits(gold[name + '.step'])) and np.array_equal(s.num.cpu().numpy(), gold[name + '.num'])
        assert np.array_equal(bits(s.minmax.cpu().numpy()), bits(gold[name + '.minmax']))
        want_tn, want_ti = gold[name + '.tri_num'], gold[name + '.tri_idx']
    else:
        want_tn, want_ti = RS.grid_tables(verts.numpy(), faces.numpy(), float(s.step), s.minmax[:3].tolist(), s.num.tolist())
        if name == 'spanning':
            cells = s.num[:3].tolist()
            assert min(cells) >= 2 and int((want_ti == 1).sum()) >= cells[0] * cells[1] * cells[2] // 2, 'the big triangle must span the grid'
    seg0 = np.concatenate([[0], want_tn[:-1]])
    repeats = int(sum((b - a) - len(np.unique(want_ti[a:b])) for a, b in zip(seg0, want_tn)))
    print('%s: %d cells, %d slots (%d repeated), %d differing counts, %d differing slots (bar 0)' % (
        name, tn.size, ti.size, repeats, int((tn != want_tn).sum()) if tn.shape == want_tn.shape else -1,
        int((ti != want_ti).sum()) if ti.shape == want_ti.shape else -1))
    assert np.array_equal(tn, want_tn) and np.array_equal(ti, want_ti)
    again = searcher_for(dev, verts, faces)
    assert torch.equal(again.tri_num, s.tri_num) and torch.equal(again.tri_idx, s.tri_idx), 'a second build must repeat the bits'


# ------------------------------------------------------------------------------------------ nearest and inside
def check_queries(dev, gold, key, N, device_allowance=False):
    """faces and signs exact, near_pts and coeff bitwise against the reference's serial run.  device_allowance (the MI355X only, and only
    once a differing operation is found and written down in DESIGN.md section 14): at most 0.1 % of the points may name another face,
    and only where the two returned points' float64 distances to the query agree within 2^-20 relative."""
    mesh, pts = case(gold, key)
    N = min(N, pts.shape[0])
    s = searcher_for(dev, mesh['verts'], mesh['faces'])
    q = pts[:N].to(dev)
    near_pts, near_faces, coeff = s.nearest(q)
    signs = s.inside_mesh(q)
    torch.cuda.synchronize()
    assert near_faces.dtype == torch.int32 and near_pts.shape == (N, 3) and coeff.shape == (N, 3) and signs.shape == (N,)
    f, p, c, sg = near_faces.cpu().numpy(), near_pts.cpu().numpy(), coeff.cpu().numpy(), signs.cpu().numpy()
    wf, wp, wc, ws = gold[key + '.near_faces'][:N], gold[key + '.near_pts'][:N], gold[key + '.coeff'][:N], gold[key + '.signs'][:N]
    step, mm, num = float(gold[key + '.step']), gold[key + '.minmax'], gold[key + '.num']
    if N >= 8:
        rel = (pts[:N].numpy() - mm[:3]) / step
        out = ((rel < 0) | (rel >= num[:3])).any(1)
        assert all(((rel[:, d] < 0).any() and (rel[:, d] >= num[d]).any()) for d in range(3)), 'queries beyond every side of the grid'
        assert (pts[:N].numpy() == mm[:3]).all(1).any(), "a query on minmax's lower corner"
        assert (ws[out] == -1).all()
    bad_f = f != wf
    bad_p = (bits(p) != bits(wp)).any(1)
    bad_c = (bits(c) != bits(wc)).any(1)
    bad_s = sg != ws
    print('%s N=%d: %d faces, %d points, %d coefficient rows, %d signs differ (bar 0 each; %d inside)' % (
        key, N, int(bad_f.sum()), int(bad_p.sum()), int(bad_c.sum()), int(bad_s.sum()), int((ws > 0).sum())))
    assert not bad_s.any()
    if device_allowance and (bad_f.any() or bad_p.any() or bad_c.any()):
        x = pts[:N].numpy().astype(np.float64)
        dg, dw = np.linalg.norm(p.astype(np.float64) - x, axis=1), np.linalg.norm(wp.astype(np.float64) - x, axis=1)
        any_bad = bad_f | bad_p | bad_c
        relgap = np.abs(dg - dw)[any_bad] / np.maximum(dw[any_bad], 1e-300)
        print('  %d of %d points differ (bar %.1f), worst distance gap %.3e relative (bar %.3e)' % (int(any_bad.sum()), N, 1e-3 * N, float(relgap.max()), 2.0 ** -20))
        assert any_bad.sum() <= 1e-3 * N and (relgap <= 2.0 ** -20).all()
        return
    assert not bad_f.any() and not bad_p.any() and not bad_c.any()


# ------------------------------------------------------------------------------------------ embedding
def held_columns(got, e32, e64, what):
    """per column: max |got - float64| within 4 x the reference's own float32 deviation, floor 2^-22 of the column's maximum"""
    got, e32, e64 = np.asarray(got, np.float64), np.asarray(e32, np.float64), np.asarray(e64, np.float64)
    assert got.shape == e64.shape and np.isfinite(got).all(), what
    scale = np.abs(e64).max(0)
    bar = np.maximum(4.0 * np.abs(e32 - e64).max(0), FLOOR * scale)
    worst = np.abs(got - e64).max(0)
    for j in range(got.shape[1]):
        print('%s column %d: worst %.3e, bar %.3e (max|ref| %.3e)' % (what, j, worst[j], bar[j], scale[j]))
    assert (worst <= bar).all(), (what, worst.tolist(), bar.tolist())


def check_embedding(dev, gold, key, N=None):
    from xrnerf_amd import gnr
    mesh, pts = case(gold, key)
    N = pts.shape[0] if N is None else min(N, pts.shape[0])
    smpl = {k: v.to(dev) for k, v in mesh.items()}
    param = {'center': torch.from_numpy(gold[key + '.center']).to(dev), 'spatial_freq': float(gold['spatial_freq'])}
    out, alpha = gnr.body_shape_embedding(pts[:N].to(dev), smpl, param, int(gold['width']), True, True, True)
    torch.cuda.synchronize()
    assert out.shape == (N, 10) and alpha.shape == (N,)
    held_columns(out.cpu().numpy(), gold[key + '.embed32'][:N], gold[key + '.embed64'][:N], '%s embedding N=%d' % (key, N))
    n_alpha = int((alpha.cpu().numpy() != gold[key + '.alpha_smpl'][:N]).sum())
    print('%s alpha_smpl: %d differ (bar 0)' % (key, n_alpha))
    assert n_alpha == 0
    # the other layouts: columns are the same quantities
    o2, a2 = gnr.body_shape_embedding(pts[:N].to(dev), smpl, param, int(gold['width']), True, False, True)
    assert a2 is not None and torch.equal(o2, torch.cat([out[:, :3], out[:, 6:]], 1))
    o3, a3 = gnr.body_shape_embedding(pts[:N].to(dev), smpl, param, int(gold['width']), False, True, False)
    assert a3 is None and torch.equal(o3, torch.cat([pts[:N].to(dev), out[:, 3:6]], 1))


# ------------------------------------------------------------------------------------------ guards
def check_launch_nothing(dev, gold):
    """a flat mesh (no cell edge), N = 0 and F = 0: XR_EINVAL or a no-op, and nothing is written (the sentinels stay)"""
    import ctypes as C
    from xrnerf_amd import _lib, gnr, ops
    lib = _lib.load()
    mesh, pts = case(gold, 'm0')
    flat = mesh['verts'].clone()
    flat[:, 2] = 0.25
    with pytest.raises(ValueError):
        searcher_for(dev, flat, mesh['faces'])
    with pytest.raises(ValueError):
        searcher_for(dev, mesh['verts'], mesh['faces'][:0])
    bad = mesh['faces'].clone()
    bad[3, 1] = mesh['verts'].shape[0]
    with pytest.raises(ValueError):
        searcher_for(dev, mesh['verts'], bad)
    bad[3, 1] = -1
    with pytest.raises(ValueError):
        searcher_for(dev, mesh['verts'], bad)
    s = searcher_for(dev, mesh['verts'], mesh['faces'])
    p = lambda t: C.c_void_p(t.data_ptr())
    q = pts[:4].to(dev).contiguous()
    nf = torch.full((4,), 7, dtype=torch.int32, device=dev)
    np_, co, sg = torch.full((4, 3), 7.0, device=dev), torch.full((4, 3), 7.0, device=dev), torch.full((4,), 7.0, device=dev)
    tn = torch.full((27,), 7, dtype=torch.int32, device=dev)
    st = torch.full((2,), 7, dtype=torch.int32, device=dev)
    mn = (C.c_float * 3)(*s._min3)
    for step, num in ((0.0, s._num3), (-1.0, s._num3), (float('nan'), s._num3), (float('inf'), s._num3), (s._step, [3, 0, 3]),
                      (s._step, [1 << 12, 1 << 12, 1 << 12])):
        nm = (C.c_int32 * 3)(*num)
        head = (p(s.verts), p(s.faces), s.verts.shape[0], s.faces.shape[0], step, C.cast(mn, C.c_void_p), C.cast(nm, C.c_void_p))
        assert lib.xr_gnr_grid_count(*head, p(tn), p(st), ops._stream()) < 0
        assert lib.xr_gnr_nearest(*head, p(s.tri_num), p(s.tri_idx), s.tri_idx.numel(), p(q), 4, p(nf), p(np_), p(co), ops._stream()) < 0
        assert lib.xr_gnr_inside(*head, p(s.tri_num), p(s.tri_idx), s.tri_idx.numel(), p(q), 4, p(sg), ops._stream()) < 0
    nm = (C.c_int32 * 3)(*s._num3)
    head = (p(s.verts), p(s.faces), s.verts.shape[0], s.faces.shape[0], s._step, C.cast(mn, C.c_void_p), C.cast(nm, C.c_void_p))
    assert lib.xr_gnr_nearest(*head, p(s.tri_num), p(s.tri_idx), s.tri_idx.numel(), p(q), 0, p(nf), p(np_), p(co), ops._stream()) == 0
    assert lib.xr_gnr_inside(*head, p(s.tri_num), p(s.tri_idx), s.tri_idx.numel(), p(q), 0, p(sg), ops._stream()) == 0
    head0 = head[:3] + (0,) + head[4:]
    assert lib.xr_gnr_grid_count(*head0, p(tn), p(st), ops._stream()) == 0
    torch.cuda.synchronize()
    for t in (nf, np_, co, sg, tn, st):
        assert bool((t == 7).all())
    e = torch.zeros((0, 3), device=dev)
    pe, fe = s.nearest_points(e)
    assert pe.shape == (0, 3) and fe.shape == (0,) and s.inside_mesh(e).shape == (0,)
    with pytest.raises(NotImplementedError):
        s.intersects_any(q, q)


def check_non_finite_queries(dev, gold):
    """(emulated and host tiers only) a non-finite coordinate touches no table: face -1, NaN point and coefficients, sign -1"""
    mesh, pts = case(gold, 'm0')
    s = searcher_for(dev, mesh['verts'], mesh['faces'])
    q = pts[:6].clone()
    q[0, 0], q[2, 1], q[4, 2] = float('nan'), float('inf'), float('-inf')
    p, f, c = s.nearest(q.to(dev))
    sg = s.inside_mesh(q.to(dev))
    for i in (0, 2, 4):
        assert int(f[i]) == -1 and bool(torch.isnan(p[i]).all()) and bool(torch.isnan(c[i]).all()) and float(sg[i]) == -1.0
    for i in (1, 3, 5):
        assert int(f[i]) == int(gold['m0.near_faces'][i]) and np.array_equal(bits(p[i].cpu().numpy()), bits(gold['m0.near_pts'][i]))
        assert float(sg[i]) == float(gold['m0.signs'][i])


# ------------------------------------------------------------------------------------------ the MI355X


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    return torch.device('cuda')


@pytest.mark.gpu
@pytest.mark.parametrize('name', STRUCT_CASES)
def test_structure_is_exact_and_repeats(dev, gold, name):
    check_structure(dev, gold, name)


@pytest.mark.gpu
@pytest.mark.parametrize('N', QUERY_N)
def test_nearest_and_inside_against_the_reference_kernels(dev, gold, N):
    check_queries(dev, gold, 'm3', N)


@pytest.mark.gpu
def test_nearest_and_inside_on_the_icosahedron(dev, gold):
    check_queries(dev, gold, 'm0', 64)


@pytest.mark.gpu
def test_all_fixture_queries_vertices_and_centroids_included(dev, gold):
    check_queries(dev, gold, 'm3', 4000)


@pytest.mark.gpu
@pytest.mark.parametrize('key', ('m0', 'm3'))
def test_embedding_against_the_reference_lines(dev, gold, key):
    check_embedding(dev, gold, key)


@pytest.mark.gpu
def test_flat_mesh_no_points_and_bad_grids_launch_nothing(dev, gold):
    check_launch_nothing(dev, gold)
