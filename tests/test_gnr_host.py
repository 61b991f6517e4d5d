"""The host path of xrnerf_amd/gnr.py (no GPU, no emulated kernels): the numpy grid build, the numpy searches (xrnerf_amd/gnr_host.py)
and the tensor-op embedding against the reference's own kernels and lines (tests/golden/ref_gnr.npz) -- on this tier the bitwise bars
are absolute -- the restatement tests/gnr_restatement.py pinned to the same fixture, the synthetic body, and the pieces that must
refuse (intersects_any)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')

import test_gpu_gnr as T  # noqa: E402


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_gnr.npz'))


@pytest.mark.parametrize('sub,V,F', ((0, 12, 20), (1, 42, 80), (3, 642, 1280)))
def test_synthetic_mesh_is_closed_and_posed(sub, V, F):
    from xrnerf_amd.gnr import synthetic_mesh
    m = synthetic_mesh(sub, 0)
    assert m['verts'].shape == (V, 3) and m['t_verts'].shape == (V, 3) and m['faces'].shape == (F, 3) and m['rot'].shape == (1, 3, 3)
    assert m['verts'].dtype == torch.float32 and m['faces'].dtype == torch.int32
    f = m['faces'].numpy()
    edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und, counts = np.unique(np.sort(edges, 1), axis=0, return_counts=True)
    assert (counts == 2).all() and len(np.unique(edges, axis=0)) == edges.shape[0], 'every edge once in each direction: closed and oriented'
    R = m['rot'][0].double()
    assert torch.allclose(R @ R.t(), torch.eye(3, dtype=torch.float64), atol=1e-6)
    off = m['verts'].double() - m['t_verts'].double() @ R.t()
    assert float((off - off.mean(0)).abs().max()) < 1e-6
    again = synthetic_mesh(sub, 0)
    assert all(torch.equal(m[k], again[k]) for k in m)


@pytest.mark.parametrize('key', ('m0', 'm3'))
def test_host_grid_build_and_geometry_equal_the_reference(gold, key):
    from xrnerf_amd.gnr import MeshGridSearcher
    mesh, _ = T.case(gold, key)
    s = MeshGridSearcher(mesh['verts'], mesh['faces'])
    assert np.array_equal(T.bits(s.step.numpy()), T.bits(gold[key + '.step'])) and np.array_equal(s.num.numpy(), gold[key + '.num'])
    assert np.array_equal(T.bits(s.minmax.numpy()), T.bits(gold[key + '.minmax']))
    assert s.tri_num.dtype == torch.int32 and np.array_equal(s.tri_num.numpy(), gold[key + '.tri_num'])
    assert np.array_equal(s.tri_idx.numpy(), gold[key + '.tri_idx'])
    assert s.verts is not None and s.faces is not None


@pytest.mark.parametrize('key', ('m0', 'm3'))
def test_restatement_is_pinned_to_the_reference(gold, key):
    import gnr_restatement as RS
    mesh, _ = T.case(gold, key)
    tn, ti = RS.grid_tables(mesh['verts'].numpy(), mesh['faces'].numpy(), float(gold[key + '.step']), gold[key + '.minmax'][:3], gold[key + '.num'])
    assert np.array_equal(tn, gold[key + '.tri_num']) and np.array_equal(ti, gold[key + '.tri_idx'])
    # the quirk is there: some slots repeat a face inside a cell
    assert int(gold[key + '.info.repeated_slots']) > 0


@pytest.mark.parametrize('name', ('one_face', 'spanning'))
def test_host_grid_build_agrees_with_the_restatement(name):
    import gnr_restatement as RS
    from xrnerf_amd.gnr import MeshGridSearcher
    verts, faces = T.other_mesh(name)
    s = MeshGridSearcher(verts, faces)
    tn, ti = RS.grid_tables(verts.numpy(), faces.numpy(), float(s.step), s.minmax[:3].tolist(), s.num.tolist())
    assert np.array_equal(s.tri_num.numpy(), tn) and np.array_equal(s.tri_idx.numpy(), ti)


@pytest.mark.parametrize('key', ('m0', 'm3'))
def test_host_embedding_against_the_reference_lines(gold, key):
    """the tensor-op path, fed the reference's search results: column bars of test_gpu_gnr.held_columns, alpha_smpl exact"""
    from xrnerf_amd import gnr
    mesh, pts = T.case(gold, key)
    param = {'center': torch.from_numpy(gold[key + '.center']), 'spatial_freq': float(gold['spatial_freq'])}
    out, alpha = gnr.embed(pts, torch.from_numpy(gold[key + '.near_pts']), torch.from_numpy(gold[key + '.near_faces']),
                           torch.from_numpy(gold[key + '.signs']), mesh, param, int(gold['width']))
    T.held_columns(out.numpy(), gold[key + '.embed32'], gold[key + '.embed64'], key + ' host embedding')
    assert np.array_equal(alpha.numpy(), gold[key + '.alpha_smpl'])


def test_guards_and_refusals_on_the_host(gold):
    from xrnerf_amd import gnr, mesh_grid
    mesh, pts = T.case(gold, 'm0')
    flat = mesh['verts'].clone()
    flat[:, 0] = 1.0
    with pytest.raises(ValueError):
        gnr.MeshGridSearcher(flat, mesh['faces'])
    bad = mesh['faces'].clone()
    bad[0, 0] = 12
    with pytest.raises(ValueError):
        gnr.MeshGridSearcher(mesh['verts'], bad)
    with pytest.raises(ValueError):
        gnr.MeshGridSearcher(mesh['verts'].double(), mesh['faces'])
    s = gnr.MeshGridSearcher(mesh['verts'], mesh['faces'])
    with pytest.raises(NotImplementedError):
        s.intersects_any(pts, pts)
    e = torch.zeros((0, 3))
    assert s.nearest_points(e)[0].shape == (0, 3) and s.inside_mesh(e).shape == (0,)
    with pytest.raises(NotImplementedError):
        mesh_grid.search_intersect(*([None] * 10))
    t = torch.tensor([1, 2, 3], dtype=torch.int32)
    r = mesh_grid.cumsum(t)
    assert t.tolist() == [1, 3, 6] and r.shape == (1, 1, 3)


@pytest.fixture
def host(monkeypatch):
    """the bodies of test_gpu_gnr.py synchronise the device; there is none here"""
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    return torch.device('cpu')


@pytest.mark.parametrize('N', T.QUERY_N)
def test_host_nearest_and_inside_against_the_reference_kernels(host, gold, N):
    T.check_queries(host, gold, 'm3', N)


def test_host_nearest_and_inside_on_the_icosahedron(host, gold):
    T.check_queries(host, gold, 'm0', 64)


def test_host_searches_on_every_fixture_query(host, gold):
    """vertices and face centroids included: the degenerate branches of the solve"""
    T.check_queries(host, gold, 'm3', 4000)


def test_host_non_finite_queries_touch_no_table(host, gold):
    T.check_non_finite_queries(host, gold)


def test_host_body_shape_embedding_end_to_end(host, gold):
    from xrnerf_amd import gnr
    mesh, pts = T.case(gold, 'm0')
    param = {'center': torch.from_numpy(gold['m0.center']), 'spatial_freq': float(gold['spatial_freq'])}
    out, alpha = gnr.body_shape_embedding(pts, mesh, param, int(gold['width']))
    T.held_columns(out.numpy(), gold['m0.embed32'], gold['m0.embed64'], 'm0 host embedding end to end')
    assert np.array_equal(alpha.numpy(), gold['m0.alpha_smpl'])


def test_the_library_table_and_the_package_know_gnr():
    import xrnerf_amd
    from xrnerf_amd import _lib
    assert hasattr(xrnerf_amd, 'gnr')
    assert set(_lib.GNR_SIGNATURES) == {'xr_gnr_grid_count', 'xr_gnr_grid_fill', 'xr_gnr_nearest', 'xr_gnr_inside', 'xr_gnr_shape_embed'}
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_gnr.h')).read()
    for name in _lib.GNR_SIGNATURES:
        assert 'int %s(' % name in header
