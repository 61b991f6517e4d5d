"""The tensor-op path of xrnerf_amd/gnr_raster.py (host tensors: per face, vectorised over its box, the same fp32 operations in the same
order) through the bodies of tests/test_gpu_gnr_raster.py, and the restatement against the fixture -- no GPU and no compiler needed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import test_gpu_gnr_raster as T  # noqa: E402

CPU = torch.device('cpu')


@pytest.mark.parametrize('name', T.CASE_NAMES)
def test_restatement_equals_the_fixture_bit_for_bit(name):
    g = T.gold()
    _, v, tri, h, w, persp = T.cases()[name]
    for view in range(v.shape[0]):
        index, coeff, vis, zbuf = T.RS.zbuffer_forward(v[view], tri, h, w, persp, T.K.EPS)
        for got, what in zip((index, coeff, vis, zbuf), ('index', 'coeff', 'visual', 'zbuf')):
            T.same(got, g['%s.%d.%s' % (name, view, what)], '%s view %d %s' % (name, view, what))


def test_fixture_is_not_vacuous():
    """every triangle type wins a pixel, a vertex is hidden, a face is culled, a pixel holds an exact-z tie won by the lower face; the
    orthographic quirk (c[2] twice) shows in the stored z of the line"""
    total = dict(full=0, line=0, point=0, culled=0, ties=0, hidden=0)
    for name in ('quads', 'degenerate_persp', 'degenerate_ortho'):
        _, v, tri, h, w, persp = T.cases()[name]
        info = {}
        T.RS.zbuffer_forward(v[0], tri, h, w, persp, T.K.EPS, info=info)
        for k in total:
            total[k] += info[k]
    assert all(n > 0 for n in total.values()), total
    g = T.gold()
    assert (g['quads.0.index'] == 4).sum() == 0 and (g['quads.0.index'] == 0).sum() > 0 and (g['quads.0.index'] == 5).sum() == 0
    row = g['degenerate_ortho.0.index'][5]
    assert row.tolist() == [-1, -1] + [0] * 8 + [-1, -1] and int(g['degenerate_ortho.0.index'][9, 4]) == 1
    z, c = g['degenerate_ortho.0.zbuf'][5, 2:10], g['degenerate_ortho.0.coeff'][5, 2:10]
    assert np.array_equal(z, c[:, 0] * np.float32(2.0) + c[:, 2] * np.float32(2.5) + c[:, 2] * np.float32(3.0))
    assert not np.array_equal(z, c[:, 0] * np.float32(2.0) + c[:, 1] * np.float32(2.5) + c[:, 2] * np.float32(3.0))
    assert g['degenerate_ortho.0.visual'].tolist() == [True, True, True, True, False, False, True]


@pytest.mark.parametrize('name', T.CASE_NAMES)
def test_tensor_ops_fixture_cases_bit_for_bit(name):
    T.check_fixture(CPU, name)


def test_tensor_ops_one_pixel_no_face_one_vertex_one_face():
    T.check_small_shapes(CPU)


@pytest.mark.parametrize('persp', (True, False))
def test_tensor_ops_random_meshes_equal_the_restatement(persp):
    T.check_random_meshes(CPU, persp)


def test_tensor_ops_more_than_a_wave_of_vertices_in_one_pixel():
    T.check_crowded_pixel(CPU)


def test_tensor_ops_views_and_repeatability():
    T.check_views_slices_and_repeat(CPU)


def test_tensor_ops_depth_maps_of_the_generated_scene():
    T.check_depth_maps(CPU)


def test_prepare_data_builds_or_keeps_the_depth_maps_on_the_host():
    T.check_prepare_data(CPU)


def test_refusals_on_host_tensors():
    T.check_refusals(CPU)
    from xrnerf_amd import _lib, ops
    v, tri = T.random_mesh(7, 8, 4, 6, 6, True)
    with pytest.raises(_lib.XrError):                               # host tensors handed to ops.*: there is no quiet CPU run
        ops.gnr_raster_forward(torch.from_numpy(v), torch.from_numpy(tri).to(torch.int32), 6, 6, True)


def test_table_and_header_name_the_same_entry_points():
    import re
    from xrnerf_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_gnr_raster.h')).read()
    assert set(re.findall(r'^(?:int|size_t) (xr_gnr_raster_\w+)\(', header, re.M)) == set(_lib.GNR_RASTER_SIGNATURES)
