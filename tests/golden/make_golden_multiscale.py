"""Generates tests/golden/ref_multiscale.npz, the fixture of the Mip-NeRF multiscale data tests:
    python tests/golden/make_golden_multiscale.py

Needs the reference tree (tests/golden/ref_import.py).  Run unmodified, in this process: the reference's load_rays_multiscale
(datasets/load_data/get_rays.py), flatten (datasets/utils/flatten.py), load_multiscale_data (datasets/load_data/load_multiscale.py),
MipMultiScaleSample and GetZvals (datasets/pipelines/create.py); and load_renderings / down2 / convert_to_nerfdata of
tools/convert_blender_data.py, whose function definitions are compiled from the file's syntax tree into a namespace that holds numpy, json,
os and PIL (the script's module level imports absl, which is not installed, and defines flags).  The draws are pinned in this process,
not by editing the reference: `time.time` is held constant in create.py's namespace (MipMultiScaleSample seeds numpy with it), numpy's
randint is wrapped for the one call so that the draw also holds the pixels the tests need, and torch is re-seeded before GetZvals; the
draw and t_rand are stored beside the outputs.

Stored: the converter's metadata.json text and PNG bytes of the generated Blender scene (tests/multiscale_cases.py), the loader's packed
pixels with and without the white background; over the rays scene (fixture_meta: distinct scalars per level, one 5 x 7 entry) the
flattened fp32 tables of every key, GetZvals of them, and the sampled training item.  Asserted here, element by element: the float64
restatement tests/multiscale_restatement.py rounds to the reference's fp32 tables, and its pyramid gives the converter's bytes and the
loader's pixels."""
import ast
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402

T0, SEED = 1234567.0, 21


def converter():
    """the function definitions of tools/convert_blender_data.py, compiled without its module level"""
    from PIL import Image
    path = os.path.join(ref_import.REF, 'tools', 'convert_blender_data.py')
    tree = ast.parse(open(path).read(), path)
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ('load_renderings', 'down2', 'convert_to_nerfdata')]
    ns = {'np': np, 'json': json, 'os': os, 'path': os.path, 'Image': Image, 'print': lambda *a, **k: None}
    exec(compile(tree, path, 'exec'), ns)
    return ns


def leaf(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_import.REF, *rel.split('/')))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import multiscale_cases as K
    import multiscale_restatement as RS
    from PIL import Image
    ns = ref_import.load_mip()
    create = importlib.import_module('xrnerf.datasets.pipelines.create')
    load_multiscale_data = importlib.import_module('xrnerf.datasets.load_data.load_multiscale').load_multiscale_data
    flatten = leaf('xrnerf/datasets/utils/flatten.py', 'ref_flatten').flatten
    conv = converter()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        # ---- the converter on the generated Blender scene
        src, dst = K.write_blender(os.path.join(tmp, 'blender')), os.path.join(tmp, 'multiscale')
        conv['convert_to_nerfdata'](src, dst, K.N_DOWN)
        text = open(os.path.join(dst, 'metadata.json')).read()
        out['metadata_json'] = np.array(text)
        meta = json.loads(text)['train']
        saved = [np.array(Image.open(os.path.join(dst, f))) for f in meta['file_path']]
        assert all(s.dtype == np.uint8 and s.shape == (h, w, 4) for s, h, w in zip(saved, meta['height'], meta['width']))
        out['pyramid.bytes'] = np.concatenate([s.reshape(-1, 4) for s in saved], 0)
        for white, key in ((True, 'pyramid.pixels'), (False, 'pyramid.pixels_plain')):
            _, images, n = load_multiscale_data(dst, 'train', white)
            assert n == K.N_VIEWS * K.N_DOWN and all(im.dtype == np.float32 for im in images)
            out[key] = np.concatenate([im.reshape(-1, 3) for im in images], 0)
            rs = [RS.pyramid(v, K.N_DOWN, white) for v in K.base_views()]
            assert np.array_equal(np.concatenate([b.reshape(-1, 4) for s, _ in rs for b in s], 0), out['pyramid.bytes']), 'restated pyramid bytes'
            assert np.array_equal(np.concatenate([p.reshape(-1, 3) for _, l in rs for p in l], 0).view(np.uint32), out[key].view(np.uint32)), 'restated pixels'
        for i, j in enumerate(meta['label']):                   # the script's pix2cam, restated
            assert np.array_equal(RS.pix2cam(meta['focal'][i], meta['width'][i], meta['height'][i]), np.array(meta['pix2cam'][i]))
        alpha = out['pyramid.bytes'][:, 3]
        assert ((alpha > 0) & (alpha < 255)).any() and (alpha == 0).any() and (alpha == 255).any()
        # ---- the rays scene: the reference's loader, rays and tables
        K._cache['gold'] = out                                  # write_fixture_scene reads the converter's results from the fixture
        root = os.path.join(tmp, 'rays')
        K.write_fixture_scene(root)
        meta, images, n = load_multiscale_data(root, 'train', True)
        assert n == 10 and meta['height'].tolist() == [12, 6, 3] * 3 + [5] and meta['width'].tolist() == [16, 8, 4] * 3 + [7]
        rays = ns.load_rays_multiscale(meta, n)
        assert all(r.dtype == np.float64 for k in ('rays_d', 'viewdirs', 'radii') for r in rays[k])
        table = {k: flatten(v) for k, v in rays.items()}
        table['target_s'] = flatten(images)
        spec = RS.tables(meta)
        for k in K.RAY_KEYS:
            got = table[k].numpy()
            assert got.dtype == np.float32 and got.shape == spec[k].shape, (k, got.shape, spec[k].shape)
            bad = int((got.view(np.uint32) != spec[k].view(np.uint32)).sum())
            assert bad == 0, 'the restatement rounds to another fp32 in %d of %d values of %s: pick another seed' % (bad, got.size, k)
        total = table['rays_o'].shape[0]
        assert total == 791
        for k, v in table.items():
            out['table.' + k] = v.numpy()
        # ---- GetZvals of the fp32 tables (what a test frame's GetZvals computes per ray once the frame is fp32)
        S = K.S_DRAW
        det = create.GetZvals(enable=True, lindisp=False, N_samples=S, randomized=False)({k: v for k, v in table.items()})
        out['table.z_vals'] = np.ascontiguousarray(det['z_vals'].numpy())
        assert out['table.z_vals'].shape == (total, S) and out['table.z_vals'].dtype == np.float32
        # ---- the training item: MipMultiScaleSample's own draw with the pixels the tests need written over its first entries
        offs = np.concatenate([[0], np.cumsum(meta['height'] * meta['width'])])
        forced = [int(offs[i]) for i in range(10)] + [int(offs[i + 1]) - 1 for i in range(10)]
        forced += [int(offs[0]) + 10 * 16 + 5, int(offs[0]) + 11 * 16 + 5, int(offs[2]) + 1 * 4 + 2, int(offs[2]) + 2 * 4 + 1, int(offs[9]) + 3 * 7 + 2, int(offs[9]) + 4 * 7 + 1]
        create.time = types.SimpleNamespace(time=lambda: T0)
        real = np.random.randint
        drawn = {}

        def randint(low, high, size):
            d = real(low, high, size)                            # numpy's generator, seeded by the reference's own reseed just before
            d[:len(forced)] = forced
            d[41] = d[40]                                        # a duplicated index
            drawn['draw'] = d.copy()
            return d
        np.random.randint = randint
        try:
            sample = create.MipMultiScaleSample(keys=['target_s'] + K.RAY_KEYS, N_rand=K.N_DRAW)
            item = sample({k: v for k, v in table.items()})
        finally:
            np.random.randint = real
        np.random.seed(int(T0) + 0)
        assert np.array_equal(real(0, total, (K.N_DRAW,))[len(forced):40], drawn['draw'][len(forced):40]), 'the wrapped draw is not the seeded one'
        out['draw'] = drawn['draw'].astype(np.int64)
        torch.manual_seed(SEED)
        item = create.GetZvals(enable=True, lindisp=False, N_samples=S, randomized=True)(item)
        torch.manual_seed(SEED)
        out['t_rand'] = torch.rand(K.N_DRAW, S).numpy()
        for k in ['target_s', 'z_vals'] + K.RAY_KEYS:
            v = item[k].numpy()
            assert v.dtype == np.float32 and v.shape[0] == K.N_DRAW
            out['train.' + k] = np.ascontiguousarray(v)
            if k != 'z_vals':
                assert np.array_equal(v.view(np.uint32), out['table.' + k][out['draw']].view(np.uint32))
        assert np.array_equal(RS.z_vals(out['train.near'], out['train.far'], S, False, out['t_rand']).view(np.uint32), out['train.z_vals'].view(np.uint32))
        assert np.array_equal(RS.z_vals(out['table.near'], out['table.far'], S).view(np.uint32), out['table.z_vals'].view(np.uint32))
    path = os.path.join(HERE, 'ref_multiscale.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes, %d rays, %d values compared with the restatement' % (path, os.path.getsize(path), total, sum(out['table.' + k].size for k in K.RAY_KEYS)))


if __name__ == '__main__':
    main()
