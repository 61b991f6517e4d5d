"""Generates tests/golden/ref_scenedata.npz, the fixture of the BungeeNeRF / KiloNeRF data tests:
    python tests/golden/make_golden_scenedata.py

Needs the reference tree (tests/golden/ref_import.py); runs on the CPU.  Run unmodified, in this process: the reference's
load_google_data, load_nsvf_dataset, load_data (datasets/load_data/), load_rays_bungee (get_rays.py), BungeeBatchSample, GetViewdirs,
GetRays, ToTensor (datasets/pipelines/), get_global_domain_min_and_max (utils/data_helper.py) and
KiloNerfNodeDataset.get_nodes_fixed_resolution (datasets/kilonerf_node_dataset.py, called unbound).  cv2 and imageio are not installed:
PIL-backed stand-ins for imread / cvtColor / resize are placed on the stub modules, at factor 1 only, where the resize is the identity.
The permutation is pinned by reseeding torch before load_rays_bungee draws it; it is stored beside the outputs.

Stored, per stage 0 / 1 / 2 of the generated google-format directory (tests/scenedata_cases.py): every item of the shuffled table
(N_rand 16, the short last slice included) concatenated and cast to fp32 -- rays_o, rays_d, target_s, radii, viewdirs -- with scale_code,
the permutation and the splits; per NSVF variant: what load_nsvf_dataset and load_data return; the scene box, the [2, 1, 2] node boxes
and GetRays of one pose.
Asserted here, element by element: the float64 restatement tests/scenedata_restatement.py rounds to the reference's float64 values
cast to fp32 (the count is printed)."""
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402


def stand_ins():
    """imread / cvtColor / resize over PIL on the stub cv2 and imageio modules"""
    from PIL import Image
    cv2, imageio = sys.modules['cv2'], sys.modules['imageio']

    def cv_imread(path, flag=None):
        a = np.array(Image.open(path))
        return a[..., ::-1].copy() if a.shape[-1] == 3 else a[..., [2, 1, 0, 3]].copy()          # BGR(A), as OpenCV hands it over

    def cvt(im, code):
        assert code in ('bgr2rgb', 'bgra2rgba')
        return im[..., ::-1].copy() if code == 'bgr2rgb' else im[..., [2, 1, 0, 3]].copy()

    def resize(im, size, interpolation=None):
        assert tuple(size) == (im.shape[1], im.shape[0]), 'the stand-in resize is the identity: factor 1 only'
        return im
    cv2.imread, cv2.cvtColor, cv2.resize = cv_imread, cvt, resize
    cv2.IMREAD_UNCHANGED, cv2.COLOR_BGR2RGB, cv2.COLOR_BGRA2RGBA, cv2.INTER_AREA = -1, 'bgr2rgb', 'bgra2rgba', 3
    imageio.imread = lambda path: np.array(Image.open(path))


def reference_modules():
    """every reference module this generator executes, imported unmodified, under one namespace.  Stubs, all stated here: ref_import's mmcv /
    cv2 / imageio shells (the latter two filled by stand_ins), and two names that kilonerf_node_dataset.py imports at module level but
    get_nodes_fixed_resolution never touches -- its base class (xrnerf.datasets.scene_dataset.SceneBaseDataset -> object) and
    xrnerf.datasets.pipelines.Compose (the reference's own compose.Compose, placed on the package shell)."""
    import types
    ref_import.load_mip()
    stand_ins()
    ns = types.SimpleNamespace()
    ns.load = importlib.import_module('xrnerf.datasets.load_data.load')
    ns.get_rays = importlib.import_module('xrnerf.datasets.load_data.get_rays')
    ns.nsvf = importlib.import_module('xrnerf.datasets.load_data.load_nsvf_dataset')
    ns.create = importlib.import_module('xrnerf.datasets.pipelines.create')
    ns.compose = importlib.import_module('xrnerf.datasets.pipelines.compose')
    utils = types.ModuleType('xrnerf.utils')
    utils.__path__ = [os.path.join(ref_import.REF, 'xrnerf', 'utils')]
    sys.modules['xrnerf.utils'] = utils
    ns.helper = importlib.import_module('xrnerf.utils.data_helper')
    sys.modules['xrnerf.datasets.pipelines'].Compose = ns.compose.Compose
    base = types.ModuleType('xrnerf.datasets.scene_dataset')
    base.SceneBaseDataset = object
    sys.modules['xrnerf.datasets.scene_dataset'] = base
    ns.node_dataset = importlib.import_module('xrnerf.datasets.kilonerf_node_dataset').KiloNerfNodeDataset
    return ns


def main():
    import scenedata_cases as K
    import scenedata_restatement as RS
    from xrnerf_amd import bungeedata
    ref = reference_modules()
    load, get_rays, create, compose, nsvf, helper = ref.load, ref.get_rays, ref.create, ref.compose, ref.nsvf, ref.helper
    out, compared = {}, 0
    with tempfile.TemporaryDirectory() as tmp:
        # ---- BungeeNeRF: the google-format directory at stages 0, 1, 2
        root = K.write_google(os.path.join(tmp, 'google'))
        for stage in K.STAGES:
            args = ref_import.Cfg(K.google_cfg(root, stage))
            images, poses, render_poses, hwf, Kmat, scale, origin, split, i_train, i_val, i_test, n_images = load.load_data(args)
            assert type(hwf[2]) is np.float64 and images.dtype == np.float32 and poses.dtype == np.float64 and n_images == 6
            torch.manual_seed(K.PERM_SEED)
            rays_rgb, radii, codes = get_rays.load_rays_bungee(hwf[0], hwf[1], hwf[2], poses, images, i_train, n_images, split, stage)
            torch.manual_seed(K.PERM_SEED)
            perm = torch.randperm(rays_rgb.shape[0]).numpy()
            assert rays_rgb.dtype == np.float64 and radii.dtype == np.float64 and codes.dtype == np.int64
            assert torch.equal(torch.from_numpy(perm), torch.randperm(len(perm), generator=torch.Generator().manual_seed(K.PERM_SEED)))
            items = []
            for idx in range(-(-len(perm) // K.N_RAND)):
                r = {'rays_rgb': rays_rgb, 'radii': radii, 'scale_code': codes, 'idx': idx}
                r = create.BungeeBatchSample(enable=True, N_rand=K.N_RAND)(r)
                r = compose.ToTensor(keys=['rays_o', 'rays_d', 'target_s', 'scale_code'])(r)
                items.append(create.GetViewdirs(enable=True)(r))
            cat = lambda k: np.concatenate([np.asarray(it[k]) for it in items], 0)
            ref64 = {k: cat(k) for k in K.RAY_KEYS}
            assert ref64['rays_d'].dtype == np.float64 and ref64['viewdirs'].dtype == np.float32 and ref64['scale_code'].dtype == np.int64
            codes_img = np.asarray(bungeedata.scale_codes(len(poses), n_images, split, stage))
            spec = RS.table(hwf[0], hwf[1], hwf[2], poses, images, codes_img, i_train, perm)
            for k in K.RAY_KEYS:
                want = ref64[k] if k == 'scale_code' else ref64[k].astype(np.float32)
                have = spec[k] if k == 'scale_code' else spec[k].astype(np.float32)
                assert want.shape == have.shape, (k, want.shape, have.shape)
                bad = np.flatnonzero(want.reshape(-1).view(np.uint32 if want.dtype == np.float32 else np.uint64)
                                     != have.reshape(-1).view(np.uint32 if want.dtype == np.float32 else np.uint64))
                assert bad.size == 0, 'stage %d %s: %d of %d values round elsewhere (first at %d): pick another scene seed' % (stage, k, bad.size, want.size, bad[0])
                compared += want.size
                out['bungee.s%d.%s' % (stage, k)] = want
            out['bungee.s%d.perm' % stage] = perm.astype(np.int64)
            out['bungee.s%d.i_train' % stage], out['bungee.s%d.i_test' % stage] = np.asarray(i_train), np.asarray(i_test)
            assert np.array_equal(render_poses, poses[i_test]) and np.array_equal(i_val, i_test)
        out['bungee.K'], out['bungee.scale_split'] = np.asarray(Kmat, np.float64), np.asarray(split)
        # ---- KiloNeRF: the NSVF directory in four variants
        for name, v in K.NSVF_VARIANTS.items():
            root = K.write_nsvf(os.path.join(tmp, 'nsvf_' + name), name)
            rgbs, poses, intr, near, far, bg, traj, i_split = nsvf.load_nsvf_dataset(root, v['testskip'])
            pre = 'nsvf.%s.' % name
            assert rgbs.dtype == np.float32 and rgbs.shape[1:] == (K.NSVF_H, K.NSVF_W, 4) and poses.dtype == np.float32 and bg is None
            out[pre + 'rgbs'], out[pre + 'poses'], out[pre + 'traj'] = rgbs, poses, np.asarray(traj)
            out[pre + 'intrinsics'] = np.array([intr.fx, intr.fy, intr.cx, intr.cy], np.float64)
            out[pre + 'near_far'] = np.array([near, far], np.float64)
            for a, k in zip(i_split, ('i_train', 'i_val', 'i_test')):
                out[pre + 'split.' + k] = a
            images, poses2, render_poses, hwf, Kmat, near2, far2, i_train, i_val, i_test = load.load_data(ref_import.Cfg(K.nsvf_cfg(root, name)))
            assert np.array_equal(poses2, poses) and float(near2) == float(near) and float(far2) == float(far) and images.shape[-1] == 3
            out[pre + 'images'], out[pre + 'render_poses'], out[pre + 'K'] = images, np.asarray(render_poses), np.asarray(Kmat, np.float64)
            out[pre + 'i_train'], out[pre + 'i_val'], out[pre + 'i_test'] = i_train, i_val, i_test
            if name == 'A':
                pose = torch.from_numpy(poses[int(i_test[0])])
                r = create.GetRays(enable=True, H=hwf[0], W=hwf[1], K=Kmat)({'pose': pose})
                out['nsvf.getrays.rays_o'], out['nsvf.getrays.rays_d'] = r['rays_o'].contiguous().numpy(), r['rays_d'].numpy()
                assert r['rays_d'].dtype == torch.float32
        gmin, gmax = helper.get_global_domain_min_and_max(ref_import.Cfg(K.nsvf_cfg(root, 'D')))
        out['nsvf.gmin'], out['nsvf.gmax'] = np.asarray(gmin), np.asarray(gmax)
        nodes = ref.node_dataset.get_nodes_fixed_resolution(None, [2, 1, 2], gmin, gmax)
        out['nodes.mins'], out['nodes.maxs'] = np.array([n.domain_min for n in nodes], np.float64), np.array([n.domain_max for n in nodes], np.float64)
        out['nodes.total_volume'] = np.asarray(helper.calculate_volume(gmin, gmax))
    path = os.path.join(HERE, 'ref_scenedata.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes; the restatement rounds to the reference in all %d compared values' % (path, len(out), os.path.getsize(path), compared))


if __name__ == '__main__':
    main()
