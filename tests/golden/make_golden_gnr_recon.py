"""Generates tests/golden/ref_gnr_recon.npz from the REFERENCE'S OWN GnrRenderer.octree_reconstruct and reconstruct, in the build
container only:
    python tests/golden/make_golden_gnr_recon.py

The machinery is make_golden_gnr_render.py's (imported unchanged): the reference's mesh_grid kernels compiled for the host behind its
own MeshGridSearcher, gnr_render.py and gnr_mlp.py imported unmodified, the render fixture's weight recipe.  On top of it:
  * `np.bool`, which the reference's lines spell and numpy has dropped, is set to `bool`;
  * `measure.marching_cubes_lewiner` -- removed from scikit-image, and scikit-image is not on this machine -- is set on the loaded
    module's `measure` stub to the float64 restatement's extractor (tests/gnr_recon_restatement.marching_cubes), so the reference's vertex
    transform and colouring lines run unmodified on this project's surface;
  * the float64 run is handed the float32 run's hull flags and mesh-query results (CastingSearcher), and its hard-coded
    `dtype=torch.float32` points are cast back to float64 where they enter make_nerf_input / make_att_input, so the two runs differ by
    rounding only.

Scene: xrnerf_amd.gnr_render.synthetic_scene(size=512) (the hard-coded 0 .. 512 range frames the body), GNRMLP(W=64, input_ch_feat=16),
N_grid = 128 (129 points per axis: the reference's own two levels, reso 2 then 1), laplacian = 0, bbox = (0, 512, 0, 512), and
gamma = 20 (the reference's attribute; with 1 the occupancy of this network nowhere flattens and no cell is skipped).

Stored (each file under 1 MiB, so not the volume):
    hull_bits        the post-hull `notprocessed` [129^3], packed bits
    near_bits        packed bits: the points whose float64 distance from a rounding boundary of the nearest-mask decision is <= 1e-3 pixel
    level_M, level_skipped   per level: evaluated points, skipped cells (the restatement's replay of the recorded occupancies, which
                     reproduces the reference's volume exactly -- asserted here)
    margins_small    float64 |max - min - 0.01| of the coarse cells below 1e-3, with their cell ids
    occ32, occ64d    the occupancies of every evaluated point in evaluation order: float32 run, and float64 run minus float32 run
    vol_sum, vol_nonzero (both runs)
    Nv, T; vert_ids (2000 seeded vertices); verts_idx, normals (the surface handed to the reference, at those vertices);
    verts32 / verts64, rgbs32 / rgbs64 at those vertices
The maker asserts, for the reference alone: both levels evaluate points; at least 100 cells skipped and 100 refined at the coarse level;
at most 1 % of the coarse cells within 1e-4 of the skip threshold; at least 500 triangles; occupancies on both sides of 0.5."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_gnr as MG  # noqa: E402
import make_golden_gnr_render as MR  # noqa: E402
import ref_import  # noqa: E402
import gnr_recon_restatement as RS  # noqa: E402

N_GRID, SIZE, GAMMA, BBOX, N_SAMPLES = 128, 512, 20, (0, 512, 0, 512), 2000
RENDER_OPT = dict(MR.RENDER_OPT, N_grid=N_GRID, loadSize=SIZE, laplacian=0)


def run(mod, renderer_cls, mlp, searcher, scene, dtype, handed=None):
    """one reconstruct call of the reference -> dict of what it made"""
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t
    opt = ref_import.Cfg(RENDER_OPT)
    opt['model'] = mlp
    ren = renderer_cls(opt)
    ren.gamma = GAMMA
    ren.mesh_searcher = MG.CastingSearcher(searcher)
    rec = {'flags': [], 'occ': [], 'surface': None}
    vh = ren.inside_pts_vh

    def inside_pts_vh(pts, masks, smpl_, calibs, persps=None):
        if handed is not None:
            inside = handed[len(rec['flags'])]
            rec['flags'].append(inside)
            return inside, None, None
        inside, vis, scan_vis = vh(pts, masks, smpl_, calibs, persps)
        rec['flags'].append(inside)
        return inside, vis, scan_vis
    mni, mai, oct_ = ren.make_nerf_input, ren.make_att_input, ren.octree_reconstruct

    def nerf(x, attdirs=None, alpha_only=False, smpl_vis=None):
        out = mlp(x, attdirs, alpha_only=alpha_only, smpl_vis=smpl_vis)
        if alpha_only:
            rec['occ'].append(torch.sigmoid(out * ren.gamma).detach().reshape(-1))
        return out

    def octree_reconstruct(coords, masks, **kw):
        rec['sdf'] = oct_(coords, masks.float(), **kw)               # (the reference's dilation kernel is float32 in either run)
        return rec['sdf']

    def extractor(sdf, level):
        v, f, n = RS.marching_cubes(sdf, level)
        rec['surface'] = (v, f, n)
        return v, f, n, None
    ren.inside_pts_vh, ren.nerf, ren.octree_reconstruct = inside_pts_vh, nerf, octree_reconstruct
    ren.make_nerf_input = lambda pts, **k: mni(pts.to(dtype), **k)
    ren.make_att_input = lambda pts, viewdirs, calibs, smpl_: mai(pts.to(dtype), viewdirs.to(dtype), calibs, smpl_)
    mod.measure = types.SimpleNamespace(marching_cubes_lewiner=extractor)
    smpl = {k: cast(v) for k, v in scene['smpl'].items()}
    with torch.no_grad():
        verts, faces, rgbs = ren.reconstruct(cast(scene['feats']), cast(scene['images']), cast(scene['masks']), cast(scene['calibs']), BBOX,
                                             {'center': cast(scene['mesh_param']['center']), 'spatial_freq': scene['mesh_param']['spatial_freq']},
                                             smpl=smpl, persps=cast(scene['persps']))
    rec.update(verts=np.asarray(verts), faces=np.asarray(faces), rgbs=np.asarray(rgbs))
    return rec


def main():
    assert ref_import.available(), 'needs the reference checkout (run in the build container)'
    from xrnerf_amd.gnr_render import synthetic_scene
    from xrnerf_amd import gnr_recon as R
    if not hasattr(np, 'bool'):
        np.bool = bool
    scene = synthetic_scene(size=SIZE)
    N = N_GRID + 1
    with tempfile.TemporaryDirectory() as tmp:
        lib = MG.build_reference_kernels(tmp)
        searcher_cls = MG.load_reference_searcher(MG.mesh_grid_module(lib))
        mod, renderer_cls, mlp_cls = MR.load_reference(searcher_cls)
        mlp32 = mlp_cls(ref_import.Cfg(MR.MLP_OPT), W=64)
        MR.gnr_weights(mlp32)
        torch.set_default_dtype(torch.float64)
        try:
            mlp64 = mlp_cls(ref_import.Cfg(MR.MLP_OPT), W=64)
        finally:
            torch.set_default_dtype(torch.float32)
        mlp64.load_state_dict({k: v.double() for k, v in mlp32.state_dict().items()}, strict=True)
        r32 = run(mod, renderer_cls, mlp32, searcher_cls(), scene, torch.float32)
        torch.set_default_dtype(torch.float64)
        try:
            r64 = run(mod, renderer_cls, mlp64, searcher_cls(), scene, torch.float64, handed=r32['flags'])
        finally:
            torch.set_default_dtype(torch.float32)
    open_ = np.zeros((N, N, N), bool)
    open_[:-1, :-1, :-1] = True
    hull = open_ & torch.cat(r32['flags']).numpy().astype(bool).reshape(N, N, N)
    out = {'hull_bits': np.packbits(hull.reshape(-1)), 'gamma': np.float64(GAMMA)}
    # the restatement's replay of the recorded occupancies is the reference's volume: the level and skip counts are then the reference's
    for tag, r in (('32', r32), ('64', r64)):
        occ = torch.cat(r['occ']).numpy()
        cursor = [0]

        def recorded(flat):
            v = occ[cursor[0]:cursor[0] + len(flat)]
            cursor[0] += len(flat)
            return v
        vol, _, levels = RS.octree(N, N // 64, hull, recorded, store=np.float64)
        assert cursor[0] == len(occ) and [m for m, _ in levels] == [len(o) for o in r['occ']], (levels, [len(o) for o in r['occ']])
        assert np.array_equal(vol, r['sdf']), 'the replay is not the reference\'s volume (%s)' % tag
        out['vol_sum' + tag], out['vol_nonzero' + tag] = np.float64(r['sdf'].sum()), np.int64(np.count_nonzero(r['sdf']))
        if tag == '32':
            out['level_M'], out['level_skipped'] = np.array([m for m, _ in levels], np.int64), np.array([s for _, s in levels], np.int64)
            levels32, occ32 = levels, occ
    occ64 = torch.cat(r64['occ']).numpy()
    assert occ32.dtype == np.float32 and occ64.dtype == np.float64 and occ32.shape == occ64.shape
    out['occ32'], out['occ64d'] = occ32, (occ64 - occ32.astype(np.float64)).astype(np.float32)
    # margins of the coarse level's cells (float32 run's values, float64 arithmetic as in the reference)
    reso = N // 64
    first = np.zeros((N, N, N))
    lattice = np.zeros((N, N, N), bool)
    lattice[::reso, ::reso, ::reso] = True
    first.reshape(-1)[np.flatnonzero(lattice & hull)] = occ32[:levels32[0][0]]
    g = np.arange(0, N, reso)
    n = len(g) - 1
    v = first[np.ix_(g, g, g)]
    corners = np.stack([v[a:a + n, b:b + n, c:c + n] for a in (0, 1) for b in (0, 1) for c in (0, 1)], 0)
    margin = np.abs(corners.max(0) - corners.min(0) - 0.01).reshape(-1)
    small = np.flatnonzero(margin < 1e-3)
    out['margin_cells'], out['margins_small'] = small.astype(np.int32), margin[small]
    # decision distance of the hull, float64 on the float32 points
    pts = torch.from_numpy(RS.grid_points(N, *RS.bounding_box(BBOX, SIZE, SIZE), scene['mesh_param']['spatial_freq'], scene['mesh_param']['center'].numpy()).reshape(-1, 3))
    masks = R.dilate_masks(scene['masks'])
    near = np.zeros(N ** 3, bool)
    for i in range(0, N ** 3, 1 << 19):
        xy = R._project(pts[i:i + (1 << 19)].double(), scene['calibs'].double(), scene['persps'].double(), SIZE, SIZE)
        near[i:i + (1 << 19)] = (RS_decision(torch.nan_to_num(xy), masks[:, 0].double()) <= 1e-3).numpy()
    out['near_bits'] = np.packbits(near)
    sv, sf, sn = r32['surface']
    assert np.array_equal(sf, r32['faces']) and np.array_equal(r64['faces'], sf), 'the two runs must extract the same triangles'
    ids = np.sort(np.random.default_rng([7, 17]).choice(len(sv), N_SAMPLES, replace=False))
    out.update(Nv=np.int64(len(sv)), T=np.int64(len(sf)), vert_ids=ids.astype(np.int32), verts_idx=sv[ids], normals=sn[ids],
               verts32=r32['verts'][ids], verts64=r64['verts'][ids], rgbs32=r32['rgbs'][ids], rgbs64=r64['rgbs'][ids])
    cells_hull = int((corners.max(0) > 0).sum())
    print('levels (M, skipped):', levels32, ' cells touching the hull:', cells_hull, ' Nv, T:', len(sv), len(sf))
    print('cells within 1e-4 of the threshold: %.5f; hull points near a rounding boundary: %.5f; occupancy %.4f .. %.4f' % (
        float((margin < 1e-4).mean()), float(near.mean()), float(occ32.min()), float(occ32.max())))
    assert len(levels32) == 2 and all(m > 0 for m, _ in levels32)
    assert levels32[0][1] >= 100 and cells_hull - levels32[0][1] >= 100
    assert (margin < 1e-4).mean() <= 0.01 and near.mean() <= 0.01
    assert len(sf) >= 500 and occ32.min() < 0.5 < occ32.max()
    assert r32['rgbs'].dtype == np.float32 and r64['rgbs'].dtype == np.float64 and r64['verts'].dtype == np.float64
    path = os.path.join(HERE, 'ref_gnr_recon.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


def RS_decision(xy, maps):
    from gnr_render_restatement import decision_distance
    return decision_distance(xy, maps, True).amin(0)


if __name__ == '__main__':
    main()
