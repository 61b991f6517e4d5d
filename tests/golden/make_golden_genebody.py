"""Generates tests/golden/ref_genebody.npz, the fixture of the GeneBody data tests:
    python tests/golden/make_golden_genebody.py

Needs the reference tree (tests/golden/ref_import.py).  Run unmodified, in this process: the reference's GeneBodyDataset
(datasets/genebody_dataset.py) with its load_obj_mesh / load_ply (datasets/utils/genebody.py), on a generated GeneBody tree written to a
temporary directory by tests/genebody_cases.write_tree.  Stand-ins live in this process only, because cv2, imageio and torchvision are
absent here: `cv2.resize` (INTER_NEAREST, INTER_CUBIC) is tests/genebody_restatement.py's, `cv2.Rodrigues` is xrnerf_amd.bodydata.rodrigues,
`imageio.imread` is PIL, `torchvision.transforms` has Compose, Resize (the identity at equal size, anything else raises), ToTensor and
Normalize as torch ops.  So the fixture pins everything the reference does AROUND those calls -- index arithmetic, crop rule, roles,
masks, K, near / far, spatial_freq, bbox, the loaders -- and the resizes only as far as the restatement goes: equality with OpenCV itself
is unverified.

Stored: the tree's arrays (`tree.*`), and per recorded item of genebody_cases.ITEMS every key the reference returns (`item.<name>.*`)
plus its subject, frame and view ids.  Asserted here: the coverage genebody_cases.coverage lists."""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import genebody_cases as K  # noqa: E402
import genebody_restatement as RS  # noqa: E402
import ref_import  # noqa: E402

# (r0, r1, c0, c1) of each view's mask rectangle, inclusive; None: an all-zero mask.  Chosen for genebody_cases.coverage
RECTS = {('dannier', '0001'): [(33, 39, 37, 39), (34, 47, 20, 32), (7, 11, 0, 34), None, (15, 47, 1, 7), (29, 36, 8, 22)],
         ('dannier', '0002'): [(43, 47, 7, 13), (29, 35, 1, 2), (3, 34, 17, 26), (37, 42, 2, 35), (28, 41, 32, 37), (5, 6, 3, 17)],
         ('amanda', '0005'): [(10, 31, 0, 34), (12, 29, 9, 22), (0, 34, 43, 44), (2, 3, 31, 37), (37, 39, 10, 28), (3, 16, 0, 1)]}
SHAPE = {'dannier': (48, 40), 'amanda': (40, 48)}


def stand_ins():
    from PIL import Image
    from xrnerf_amd.bodydata import rodrigues
    cv2 = types.ModuleType('cv2')
    cv2.INTER_NEAREST, cv2.INTER_CUBIC = 0, 2

    def resize(src, dsize, interpolation=None):
        assert dsize[0] == dsize[1] and src.shape[0] > 0 and src.shape[1] > 0
        if interpolation == cv2.INTER_NEAREST:
            return RS.resize_nearest(src, dsize[0])
        assert interpolation == cv2.INTER_CUBIC and src.dtype == np.uint8
        return RS.resize_cubic_u8(src, dsize[0])
    cv2.resize = resize
    cv2.Rodrigues = lambda r: (rodrigues(np.asarray(r, np.float64).reshape(3)), None)
    imageio = types.ModuleType('imageio')
    imageio.imread = lambda path: np.asarray(Image.open(path))
    tv, tr = types.ModuleType('torchvision'), types.ModuleType('torchvision.transforms')

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    class Resize:
        def __init__(self, size):
            self.size = size

        def __call__(self, img):
            if img.size != (self.size, self.size):
                raise AssertionError('the stand-in Resize is the identity only')
            return img

    class ToTensor:
        def __call__(self, img):
            return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)

        def __call__(self, t):
            return t.clone().sub_(self.mean[:, None, None]).div_(self.std[:, None, None])
    tr.Compose, tr.Resize, tr.ToTensor, tr.Normalize = Compose, Resize, ToTensor, Normalize
    tv.transforms = tr
    sys.modules.update({'cv2': cv2, 'imageio': imageio, 'torchvision': tv, 'torchvision.transforms': tr})


def reference():
    stand_ins()
    ref_import.load_mip()
    pipes = sys.modules['xrnerf.datasets.pipelines']
    pipes.Compose = importlib.import_module('xrnerf.datasets.pipelines.compose').Compose
    utils = types.ModuleType('xrnerf.datasets.utils')
    utils.__path__ = [os.path.join(ref_import.REF, 'xrnerf', 'datasets', 'utils')]
    sys.modules['xrnerf.datasets.utils'] = utils
    return importlib.import_module('xrnerf.datasets.genebody_dataset').GeneBodyDataset


def body(rng, n=60, offset=(0., 0., 0.)):
    verts = (rng.uniform([-0.4, -0.9, -0.3], [0.4, 0.9, 0.3], (n, 3)) + np.array(offset)).astype(np.float32)
    tris = np.stack([rng.permutation(n)[:3] for _ in range(40)]).astype(np.int32)
    return verts, tris


def cameras(rng, h, w):
    Ks, Ds, c2ws = [], [], []
    for v in range(K.N_CAM):
        ang = 2 * np.pi * v / K.N_CAM + 0.2
        pos = np.array([3.0 * np.cos(ang), 0.3 * np.sin(3 * ang), 3.0 * np.sin(ang)])
        z = -pos / np.linalg.norm(pos)
        x = np.cross(np.array([0., 1., 0.]), z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = np.stack([x, y, z], axis=1), pos
        Ks.append(np.array([[52. + v, 0, w / 2 + 0.3 * v], [0, 51.5 - v, h / 2 - 0.7], [0, 0, 1]]))
        Ds.append(rng.normal(0, 0.01, 5))
        c2ws.append(c2w)
    return np.stack(Ks), np.stack(Ds), np.stack(c2ws)


def make_tree():
    rng = np.random.default_rng(2026)
    g = {}
    g['tree.t_pose.verts'], g['tree.t_pose.faces'] = body(rng, 50)
    for s, frames in K.SUBJECTS.items():
        h, w = SHAPE[s]
        g['tree.%s.K' % s], g['tree.%s.D' % s], g['tree.%s.c2w' % s] = cameras(rng, h, w)
        for f in frames:
            p = 'tree.%s.%s.' % (s, f)
            verts, tris = body(rng, 60 + len(f) + int(f), offset=(0.03, 0.05, -0.02))
            quad = np.array([0, 1, 2, 3], np.int32)
            if s == 'dannier':
                tris = np.concatenate([np.array([[0, 1, 2], [2, 3, 0]], np.int32), tris])
                g[p + 'quad'] = quad
            g[p + 'verts'], g[p + 'faces'] = verts, tris
            g[p + 'scale'] = np.float64(rng.uniform(0.9, 1.1))
            g[p + 'orient'] = rng.normal(0, 0.6, (1, 3)).astype(np.float32)
            g[p + 'betas'] = rng.normal(0, 1, (1, 10)).astype(np.float32)
            for v, rect in enumerate(RECTS[(s, f)]):
                g[K.vkey(s, f, v, 'image')] = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
                m = np.zeros((h, w), np.uint8)
                if rect is not None:
                    r0, r1, c0, c1 = rect
                    m[r0:r1 + 1, c0:c1 + 1] = rng.choice(np.array([128, 129, 255, 255], np.uint8), (r1 - r0 + 1, c1 - c0 + 1))
                    m[[r0, r0, r1, r1], [c0, c1, c0, c1]] = 255
                g[K.vkey(s, f, v, 'mask')] = m
                if v in K.INPUT_VIEWS:
                    d = np.zeros((h, w), np.uint16)
                    r0, r1, c0, c1 = rect
                    rr0, cc0 = max(r0 - 3, 0), max(c0 - 2, 0)
                    d[rr0:max(r1 - 2, rr0 + 1), cc0:max(c1 - 1, cc0 + 1)] = rng.integers(500, 4000, (max(r1 - 2, rr0 + 1) - rr0, max(c1 - 1, cc0 + 1) - cc0))
                    d[r1, c1] = 0                                         # zero inside the mask; the block above reaches outside it
                    g[K.vkey(s, f, v, 'smpl_depth')] = d
    return g


def to_np(v):
    if isinstance(v, torch.Tensor):
        return v.numpy()
    return np.asarray(v)


def main():
    g = make_tree()
    K.coverage(g)
    Ref = reference()
    with tempfile.TemporaryDirectory() as root:
        for name, (phase, S, white, skip, index, rnd) in K.ITEMS.items():
            opt = dict(K.write_tree(root, g), loadSize=S, use_white_bkgd=white, random_multiview=rnd)
            opt['train_skip' if phase == 'train' else 'eval_skip'] = skip
            ds = Ref(ref_import.Cfg(opt), [], phase=phase)
            ds.input_views, ds.test_views = list(K.INPUT_VIEWS), list(range(K.N_CAM))
            seen = []
            real = ds.get_image

            def spy(sid, num_views, view_id=None, random_sample=False, smpl_verts=None, real=real, seen=seen, ds=ds):
                out = real(sid, num_views, view_id=view_id, random_sample=random_sample, smpl_verts=smpl_verts)
                seen.append(sid)
                return out
            ds.get_image = spy
            if rnd:
                np.random.seed(K.RANDOM_SEED)
            item = ds[index]
            assert tuple(item.keys()) == K.ITEM_KEYS, item.keys()
            sid = seen[0]
            s, f = ds.subjects[sid], ds.frames[sid]
            # the view ids the item used, recovered from its extrinsics
            w2cs = [np.linalg.inv(np.array(c, dtype=np.float32)) for c in g['tree.%s.c2w' % s]]
            vids = [int(np.argmin([np.abs(w - c.numpy()).max() for w in w2cs])) for c in item['calib']]
            assert vids[:K.NUM_VIEWS] == K.INPUT_VIEWS
            for k, v in item.items():
                g['item.%s.%s' % (name, k)] = to_np(v)
            g['item.%s.subject' % name], g['item.%s.frame' % name], g['item.%s.view_ids' % name] = np.array(s), np.array(f), np.array(vids)
            g['item.%s.len' % name] = np.array(len(ds))
            print('%-14s %s %s views %r  bbox %r  spatial_freq %.6f' % (name, s, f, vids, item['bbox'].tolist(), item['spatial_freq']))
    # the restatement equals what the reference computed, before anything is stored
    for name in K.ITEMS:
        K._gold = g
        spec = K.spec_item(name)
        K.same_bits(np.stack(spec['img']), np.concatenate([g['item.%s.img' % name], g['item.%s.render_gt' % name].reshape((-1,) + g['item.%s.img' % name].shape[1:])]), 'img ' + name)
    np.savez_compressed(K.GOLD, **g)
    print('wrote %s: %d arrays, %d bytes' % (K.GOLD, len(g), os.path.getsize(K.GOLD)))


if __name__ == '__main__':
    main()
