"""GNR's mesh reconstruction without a GPU: the restatement (tests/gnr_recon_restatement.py) held to the reference's serial form and to
the kernel source's triangle table, and the tensor-op path of xrnerf_amd/gnr_recon.py -- what host tensors take -- through the bodies
of tests/test_gpu_gnr_recon.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import gnr_recon_restatement as RS  # noqa: E402
import test_gpu_gnr_recon as T  # noqa: E402

CPU = torch.device('cpu')


# ------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize('N,reso0', ((33, 4), (17, 2), (21, 4)))
def test_parallel_fill_rule_equals_the_serial_loop(N, reso0):
    """last skipped cell in C order wins == the reference's loop that applies the cells one after the other (float64 volumes)"""
    open_ = np.zeros((N, N, N), bool)
    open_[:-1, :-1, :-1] = True
    for kind in ('blob', 'ramp', 'constant', 'checker'):
        table = T.field(N, reso0, kind)
        fn = lambda flat: table[flat]
        vol, todo, levels = RS.octree(N, reso0, open_, fn, store=np.float64)
        svol, stodo = RS.octree_serial(N, reso0, open_, fn)
        assert np.array_equal(vol, svol) and np.array_equal(todo, stodo), kind
        if kind == 'ramp':
            assert levels[0][1] > 8 and len(np.unique(vol[:reso0 * 2 + 1])) > 2        # neighbouring skipped cells with different fills


@pytest.mark.parametrize('tag', ('32', '64'))
def test_restatement_octree_reproduces_the_reference_volume(tag):
    """the restatement's octree on the fixture's hull with the reference's recorded occupancies: the reference's level counts, and its
    volume's sum and non-zero count exactly (the maker asserted the whole volume equal); with a float32 store the same decisions and the
    same values up to that store.  No cell is excluded: the same doubles give the same decisions."""
    gold = T.load_gold()
    vol, levels, flats, occ = T.replay_reference(gold, tag)
    if tag == '32':
        assert [m for m, _ in levels] == gold['level_M'].tolist() and [s for _, s in levels] == gold['level_skipped'].tolist()
    assert levels[0][1] >= 100 and len(levels) == 2
    assert float(vol.sum()) == float(gold['vol_sum' + tag]) and int(np.count_nonzero(vol)) == int(gold['vol_nonzero' + tag])
    if tag == '32':
        vol32, levels32, _, _ = T.replay_reference(gold, tag, store=np.float32)
        assert levels32 == levels and np.array_equal(vol32, vol.astype(np.float32))
        assert (gold['margins_small'] < 1e-4).sum() <= 0.01 * 64 ** 3


def test_table_in_the_kernel_source_equals_the_derived_one():
    from xrnerf_amd import gnr_recon as R
    typed = R.cube_table().numpy()
    derived = RS.table()
    assert typed.shape == (256, 16)
    for case in range(256):
        flat = [e for tri in derived[case] for e in tri]
        assert typed[case].tolist() == flat + [-1] * (16 - len(flat)), case
    assert sum(len(r) for r in derived) == 820 and max(len(r) for r in derived) == 5
    # no complement symmetry: two inside corners on a face diagonal are cut apart, two outside ones are not
    assert len(derived[0b00001001]) == 2 and len(derived[0b11110110]) == 4


def test_restatement_surfaces_are_closed_and_outward():
    for case in range(1, 256):
        vol = np.zeros((4, 4, 4))
        for c in range(8):
            if (case >> c) & 1:
                o = RS.corner_offset(c)
                vol[1 + o[0], 1 + o[1], 1 + o[2]] = 1.0
        v, f, n = RS.marching_cubes(vol, 0.5)
        assert RS.is_closed(f) and RS.signed_volume(v, f) > 0, case
    v, f, n = RS.marching_cubes(T.solid('sphere'), 0.5)
    assert RS.euler(len(v), f) == 2


def test_world_transform_keeps_the_reference_off_by_one():
    v = np.array([[0.0, 0.0, 0.0], [128.0, 64.0, 32.0]])
    w = RS.to_world(v, 129, (10, 500), 90.0, np.array([0.1, 0.2, 0.3], np.float32))
    assert np.allclose(w[1], (np.array([128.0, 64.0, 32.0]) - 64.5) / 129 * np.array([512.0, 490.0, 512.0]) / 90.0 + np.array([0.1, 0.2, 0.3], np.float32).astype(np.float64), rtol=0, atol=1e-15)
    from xrnerf_amd import gnr_recon as R
    got, pts = R.to_world(torch.from_numpy(v).float(), 129, (10, 500), 90.0, torch.tensor([0.1, 0.2, 0.3]))
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), w) and np.array_equal(pts.numpy(), w.astype(np.float32))


# ------------------------------------------------------------------------------------------ the tensor-op path
@pytest.mark.parametrize('N', T.HULL_SIZES)
def test_grid_points_bit_for_bit_and_hull_flags(N):
    T.check_grid_hull(CPU, N)


@pytest.mark.parametrize('N,reso0,kind', T.OCTREE_CASES)
def test_octree_bookkeeping_equals_the_restatement(N, reso0, kind):
    T.check_octree(CPU, N, reso0, kind)


def test_surface_of_all_256_corner_patterns_is_closed():
    T.check_surface_patterns(CPU)


def test_surface_of_random_volumes_is_closed():
    T.check_surface_random(CPU)


def test_surface_sphere_and_torus():
    T.check_surface_solids(CPU)


def test_surface_degenerate_volumes():
    T.check_surface_degenerate(CPU)


def test_world_transform_point_rows_and_sigmoid_scatter():
    T.check_small_stages(CPU)


def test_laplacian_smoothing():
    T.check_smooth(CPU)


def test_reconstruct_on_the_generated_scene():
    """N_grid = 64: the reference's N // 64 leaves one level there, which a CPU affords"""
    T.check_reconstruct(CPU, N_grid=64, laplacian=2)


def test_refusals_come_before_anything_is_touched():
    ren = T.renderer(CPU, 64, 0)
    with pytest.raises(NotImplementedError, match='projection'):
        ren.reconstruct(None, None, None, None, None, None)
    with pytest.raises(NotImplementedError, match='projection'):
        ren.octree_reconstruct(None, None)


def test_header_table_and_library_name_the_same_entry_points():
    import re
    from xrnerf_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_gnr_recon.h')).read()
    assert set(re.findall(r'^(?:int|size_t) (xr_gnr_recon_\w+)\(', header, re.M)) == set(_lib.GNR_RECON_SIGNATURES)
    for name, (res, args) in _lib.GNR_RECON_SIGNATURES.items():
        text = header[header.index(' %s(' % name):]
        assert text[:text.index(');')].count(',') + 1 == len(args), name
