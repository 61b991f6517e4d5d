"""The REFERENCE's own MeshGridSearcher (extensions/mesh_grid/mesh_grid_searcher.py), imported unmodified from where it lies with
    sys.modules['mesh_grid'] = xrnerf_amd.mesh_grid      (and `trimesh` an empty stub: the file imports it and never uses it)
must reproduce the fixture of the reference's own kernels (tests/golden/ref_gnr.npz): set_mesh, nearest_points, inside_mesh -- first
on the drop-in's host path, then on the kernels, the real source (xrnerf_amd/csrc/xr_gnr.hip) executed on the host by tests/hip_emu.
Needs the reference tree."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ref_import  # noqa: E402

pytestmark = pytest.mark.skipif(not ref_import.available(), reason='needs the reference tree')
G = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_gnr.npz'))


@pytest.fixture(scope='module')
def edev():
    import test_emu_gnr as E
    with E.emulated_gnr() as dev:
        yield dev


@pytest.fixture(scope='module')
def ref_searcher():
    import xrnerf_amd.mesh_grid as drop_in
    saved = {k: sys.modules.get(k) for k in ('mesh_grid', 'trimesh')}
    sys.modules['mesh_grid'] = drop_in
    sys.modules['trimesh'] = types.ModuleType('trimesh')
    try:
        path = os.path.join(ref_import.REF, 'extensions', 'mesh_grid', 'mesh_grid_searcher.py')
        spec = importlib.util.spec_from_file_location('ref_mesh_grid_searcher_on_shims', path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod.MeshGridSearcher


def reproduces(ref_searcher, gold, key, N, dev):
    import test_gpu_gnr as T
    mesh, pts = T.case(gold, key)
    s = ref_searcher(mesh['verts'].to(dev), mesh['faces'].to(dev))
    assert np.array_equal(s.tri_num.numpy(), gold[key + '.tri_num']) and np.array_equal(s.tri_idx.numpy(), gold[key + '.tri_idx'])
    assert np.array_equal(s.num.numpy(), gold[key + '.num'])
    p, f = s.nearest_points(pts[:N])
    sg = s.inside_mesh(pts[:N])
    assert np.array_equal(f.numpy(), gold[key + '.near_faces'][:N])
    assert np.array_equal(T.bits(p.numpy()), T.bits(gold[key + '.near_pts'][:N]))
    assert np.array_equal(sg.numpy(), gold[key + '.signs'][:N])
    with pytest.raises(NotImplementedError):
        s.intersects_any(pts[:2], pts[:2])


@pytest.mark.parametrize('key,N', (('m0', 64), ('m3', 500)))
def test_reference_searcher_on_the_drop_in_host_path(ref_searcher, gold, key, N):
    from xrnerf_amd import gnr
    assert not gnr._use_kernels(torch.zeros(1)), 'this test runs before the emulated kernels are switched on'
    reproduces(ref_searcher, gold, key, N, torch.device('cpu'))


@pytest.mark.parametrize('key,N', (('m0', 64), ('m3', 500)))
def test_reference_searcher_on_the_drop_in_kernels(edev, ref_searcher, gold, key, N):
    from xrnerf_amd import gnr
    assert gnr._use_kernels(torch.zeros(1))
    reproduces(ref_searcher, gold, key, N, edev)
