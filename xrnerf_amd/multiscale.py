"""Mip-NeRF multiscale data on the device: MipMultiScaleDataset, MipMultiScaleSample, the Compose planner that runs a training item as one
xr_ms_rays launch, and the Blender -> multiscale converter -- the data side of configs/mipnerf/mipnerf_multiscale.py.

Mirrors, relative to the reference's tree:
  xrnerf/datasets/mip_multiscale_dataset.py            MipMultiScaleDataset
  xrnerf/datasets/load_data/load_multiscale.py         load_multiscale_data
  xrnerf/datasets/load_data/get_rays.py:101-153        load_rays_multiscale (host path: _frame_rays; device path: the kernel)
  xrnerf/datasets/utils/flatten.py                     flatten
  xrnerf/datasets/pipelines/create.py:48-79            MipMultiScaleSample
  tools/convert_blender_data.py                        convert_blender_scene

The reference materialises seven float64 arrays per pixel of every image at every scale and flattens them into fp32 tables of 16 floats
per ray.  Here the packed images [total, 3] and a CameraTable of 24 doubles per image are resident on the device, and an item makes the
rays of the pixels it drew (xrnerf_amd/csrc/xr_multiscale.hip).  Without the library, or with device='cpu', the reference's tables are
materialised on the host from _frame_rays (float64 in the kernel's operation order, rounded to fp32 once) and indexed.

Deviations from the reference:
  * the draw is torch.randint from a generator on the data's device seeded `seed + rank` once, not numpy reseeded from time() + rank at
    every item (the same documented deviation as SelectRays); results['ray_indices'], when present, replaces the draw and is popped
  * test and val frames are fp32 (the reference hands float64 numpy views to GetZvals, which current numpy / torch refuse to multiply)
"""
import json
import os

import numpy as np
import torch

from . import builder, ops, pipelines
from .networks import get_dist_info
from .pipelines import DATASETS, PIPELINES, Compose, GetZvals, ToTensor

RAY_KEYS = ('rays_o', 'rays_d', 'viewdirs', 'radii', 'lossmult', 'near', 'far')
META_KEYS = ('file_path', 'cam2world', 'width', 'height', 'focal', 'label', 'near', 'far', 'lossmult', 'pix2cam')
TABLE_KEY = 'camera_table'          # the results key a CameraTable travels under


# ------------------------------------------------------------------------------------------ the host restatement
def _frame_rays(pix2cam, cam2world, H, W, lossmult, near, far):
    """load_rays_multiscale for one image: the seven [H, W, .] float64 arrays, every product and sum in the kernel's order"""
    H, W = int(H), int(W)
    if H < 3:                    # dx[-2:-1] is empty below 3 rows: the reference returns fewer radii than rays
        raise ValueError('multiscale rays need H >= 3 (got %d)' % H)
    P, C = np.asarray(pix2cam, np.float64), np.asarray(cam2world, np.float64)
    x = (np.arange(W, dtype=np.float64) + 0.5)[None, :] * np.ones((H, 1))
    y = (np.arange(H, dtype=np.float64) + 0.5)[:, None] * np.ones((1, W))
    cam = [(x * P[r, 0] + y * P[r, 1]) + P[r, 2] for r in range(3)]
    d = np.stack([(cam[0] * C[r, 0] + cam[1] * C[r, 1]) + cam[2] * C[r, 2] for r in range(3)], -1)
    n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    e = d[:-1] - d[1:]
    dx = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
    dx = np.concatenate([dx, dx[-2:-1]], 0)
    ones = np.ones((H, W, 1))
    return dict(rays_o=np.broadcast_to(C[:3, 3], (H, W, 3)), rays_d=d, viewdirs=d / n[..., None], radii=(dx[..., None] * 2) / np.sqrt(12.0),
                lossmult=float(lossmult) * ones, near=float(near) * ones, far=float(far) * ones)


def _down2(img):
    """convert_blender_data.py:43-45 in the association numpy's mean takes: (((a + b) + c) + d) / 4, float32"""
    return (((img[0::2, 0::2] + img[0::2, 1::2]) + img[1::2, 0::2]) + img[1::2, 1::2]) / np.float32(4)


def _host_pyramid(base, n_down, white_bkgd):
    """[N,H,W,C] uint8 -> (bytes [N per_view, C], pixels [N per_view, 3]) packed like ops.ms_pyramid, in numpy"""
    saved, loaded = [], []
    for view in base:
        img = view.astype(np.float32) / np.float32(255)
        for j in range(n_down):
            b = (img * np.float32(255)).astype(np.uint8)
            saved.append(b.reshape(-1, b.shape[-1]))
            loaded.append(_composite(b, white_bkgd).reshape(-1, 3))
            if j + 1 < n_down:
                img = _down2(img)
    return np.concatenate(saved, 0), np.concatenate(loaded, 0)


def _composite(image8, white_bkgd):
    """load_multiscale.py:18-22 on one uint8 image"""
    image = np.asarray(image8, dtype=np.float32) / 255.
    if white_bkgd:
        image = image[..., :3] * image[..., -1:] + (1. - image[..., -1:])
    return image[..., :3]


# ------------------------------------------------------------------------------------------ loading
def load_multiscale_data(datadir, mode, white_bkgd):
    """metadata.json[mode] as arrays, the images [h, w, 3] float32 and their number (load_multiscale.py)"""
    from PIL import Image
    with open(os.path.join(datadir, 'metadata.json'), 'r') as fp:
        meta = json.load(fp)[mode]
    meta = {k: np.array(meta[k]) for k in meta}
    images = []
    for fbase in meta['file_path']:
        with open(os.path.join(datadir, fbase), 'rb') as imgin:
            images.append(_composite(np.array(Image.open(imgin)), white_bkgd))
    return meta, images, len(images)


class CameraTable:
    """the device-resident form of a split: 24 doubles per image (pix2cam, cam2world rows 0..2, lossmult, near, far), the sizes, the int64
    prefix of H W, and the packed images [total, 3]"""

    def __init__(self, meta, images, device):
        self.sizes = [(int(h), int(w)) for h, w in zip(meta['height'], meta['width'])]
        if not self.sizes or min(h for h, _ in self.sizes) < 3:
            raise ValueError('multiscale rays need at least one image and H >= 3 everywhere (got %r)' % (self.sizes[:4],))
        n = len(self.sizes)
        self.offsets = np.concatenate([[0], np.cumsum([h * w for h, w in self.sizes])]).astype(np.int64)
        self.total = int(self.offsets[-1])
        cams = np.concatenate([np.asarray(meta['pix2cam'], np.float64).reshape(n, 9), np.asarray(meta['cam2world'], np.float64)[:, :3, :4].reshape(n, 12),
                               np.stack([np.asarray(meta[k], np.float64) for k in ('lossmult', 'near', 'far')], 1)], 1)
        self.device = torch.device(device)
        self.cams = torch.from_numpy(np.ascontiguousarray(cams)).to(self.device)
        self.hw = torch.tensor(self.sizes, dtype=torch.int32).to(self.device)
        self.prefix = torch.from_numpy(self.offsets).to(self.device)
        if isinstance(images, torch.Tensor):
            self.images = images.to(self.device)
        else:
            self.images = torch.from_numpy(np.concatenate([np.ascontiguousarray(im, dtype=np.float32).reshape(-1, 3) for im in images], 0)).to(self.device)
        if tuple(self.images.shape) != (self.total, 3) or self.images.dtype != torch.float32:
            raise ValueError('the images hold %r %s, the metadata asks for [%d, 3] float32' % (tuple(self.images.shape), self.images.dtype, self.total))

    def __len__(self):
        return len(self.sizes)

    def image(self, i):
        h, w = self.sizes[i]
        return self.images[int(self.offsets[i]):int(self.offsets[i + 1])].view(h, w, 3)

    def rays(self, idx, **kw):
        """the rays of flat indices idx (int64, on the device): one launch"""
        return ops.ms_rays(self.cams, self.hw, self.prefix, self.sizes, images=self.images, idx=idx, **kw)

    def frame(self, i, want=RAY_KEYS, **kw):
        """the rays of every pixel of image i as [H, W, .]: one launch"""
        h, w = self.sizes[i]
        out = ops.ms_rays(self.cams, self.hw, self.prefix, self.sizes, images=self.images, image=i, want=want, **kw)
        return {k: v.view(h, w, v.shape[-1]) for k, v in out.items()}

    def z_row(self, i, S, lindisp):
        """the un-randomised z_vals of image i, [1, S]: they depend on the image's near / far only"""
        return ops.ms_rays(self.cams, self.hw, self.prefix, self.sizes, image=i, R=1, S=S, lindisp=lindisp, want=('z_vals',))['z_vals']


# ------------------------------------------------------------------------------------------ the transform and its fused run
@PIPELINES.register_module()
class MipMultiScaleSample:
    """N_rand rays of the whole set, drawn with replacement (create.py:48-79).  Handed plain tensors it indexes every key with one draw;
    handed the dataset's CameraTable (results['camera_table']) it makes the drawn rays in one launch."""

    def __init__(self, enable=True, N_rand=1024, keys=[], seed=0, **kwargs):
        self.enable, self.keys, self.N_rand, self.seed = enable, keys, N_rand, seed
        self._generators = {}

    def draw(self, results, n, device):
        """int64 [N_rand] on `device`; pops results['ray_indices']"""
        inds = results.pop('ray_indices', None)
        if inds is None:
            device = torch.device(device)
            if device not in self._generators:
                self._generators[device] = torch.Generator(device=device).manual_seed(self.seed + get_dist_info()[0])
            return torch.randint(0, n, (self.N_rand,), device=device, generator=self._generators[device])
        return torch.as_tensor(inds).to(device=device, dtype=torch.int64)

    def __call__(self, results):
        if self.enable:
            table = results.pop(TABLE_KEY, None)
            if table is not None:
                got = table.rays(self.draw(results, table.total, table.device), want=list(self.keys))
                results.update({k: got[k] for k in self.keys})
            else:
                first = results[self.keys[0]]
                inds = self.draw(results, first.shape[0], first.device if isinstance(first, torch.Tensor) else 'cpu')
                for k in self.keys:
                    results[k] = results[k][inds if isinstance(results[k], torch.Tensor) else inds.cpu().numpy()]
        return results

    def __repr__(self):
        return '{}:slice a batch of rays from all rays'.format(self.__class__.__name__)


class MultiscaleRun:
    """Compose's second planner: transforms[start .. end] over a CameraTable as xr_ms_rays calls.
    Train: [MipMultiScaleSample, GetZvals, ToTensor ...] is ONE launch (the draw, the rays, the targets and z_vals).
    Test / val: [GetZvals(randomized=False), ToTensor ...] over a frame that carries its table: z_vals is one [1, S] row expanded."""

    def __init__(self, start, end, sample, zvals, side):
        self.start, self.end, self.sample, self.zvals, self.side = start, end, sample, zvals, side

    @staticmethod
    def plan(transforms):
        enabled = lambda t: getattr(t, 'enable', True)
        live = [(i, t) for i, t in enumerate(transforms) if enabled(t)]
        if not live or type(live[0][1]) not in (MipMultiScaleSample, GetZvals) or any(type(t) is MipMultiScaleSample for _, t in live[1:]):
            return None
        (start, first), sample = live[0], None
        rest = live[1:]
        if type(first) is MipMultiScaleSample:
            if not rest or type(rest[0][1]) is not GetZvals:
                return None
            sample, (zi, zvals), rest = first, rest[0], rest[1:]
            if any(k not in RAY_KEYS + ('target_s',) for k in sample.keys) or not {'near', 'far', 'rays_o'} <= set(sample.keys):
                return None
        else:
            zi, zvals = start, first
            if zvals.randomized:
                return None
        side = []
        for i, t in rest:                                          # only ToTensor may follow inside the run
            if type(t) is not ToTensor or i != zi + len(side) + 1:
                break
            side.append(t)
        return MultiscaleRun(start, zi + len(side), sample, zvals, side)

    def ready(self, results):
        table = results.get(TABLE_KEY)
        if not isinstance(table, CameraTable) or not ops._on_device(table.cams) or not ops.multiscale_kernels_available():
            return False
        if self.sample is None:                                    # a frame made by CameraTable.frame, with its index
            return isinstance(results.get('idx'), int) and isinstance(results.get('near'), torch.Tensor) and results['near'].dim() == 3
        return True

    def __call__(self, results):
        table, z = results.pop(TABLE_KEY), self.zvals
        if self.sample is not None:
            s = self.sample
            idx = s.draw(results, table.total, table.device)
            kw = {}
            if z.randomized:
                t_rand = results.pop('t_rand', None)
                kw['t_rand'] = torch.rand((idx.shape[0], z.N_samples), device=table.device) if t_rand is None else t_rand.to(table.device)
            results.update(table.rays(idx, S=z.N_samples, lindisp=z.lindisp, want=list(s.keys) + ['z_vals'], **kw))
        else:
            h, w = results['near'].shape[:2]
            results['z_vals'] = table.z_row(results['idx'], z.N_samples, z.lindisp).expand(h, w, z.N_samples)
        for t in self.side:
            for k in t.keys:
                if k in results:
                    results[k] = pipelines.to_tensor(results[k])
        return results


# ------------------------------------------------------------------------------------------ the dataset
@DATASETS.register_module()
class MipMultiScaleDataset:
    """the reference's MipMultiScaleDataset (mip_multiscale_dataset.py).  On the device the split is a CameraTable and the packed images;
    on the host (device='cpu', or no library) it is the reference's flattened fp32 tables."""
    mode = 'train'

    def __init__(self, cfg, pipeline, device=None, seed=0, _loaded=None):
        self.iter_n = 0
        self.cfg = builder.ConfigDict.wrap(dict(cfg))
        if 'mode' in self.cfg: self.mode = self.cfg.mode
        self.device = torch.device(device) if device is not None else torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
        self.seed = seed
        self._init_load(_loaded)
        self._init_pipeline(pipeline)

    @classmethod
    def from_blender(cls, cfg, pipeline, blenderdir, n_down=4, device=None, seed=0):
        """the dataset of cfg.mode over a Blender scene converted in memory: nothing is written to disk"""
        cfg = builder.ConfigDict.wrap(dict(cfg))
        mode = cfg.mode if 'mode' in cfg else cls.mode
        device = torch.device(device) if device is not None else torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
        meta, packed = convert_blender_scene(blenderdir, None, n_down, device, white_bkgd=cfg.white_bkgd, splits=(mode,))[mode]
        return cls(cfg, pipeline, device=device, seed=seed, _loaded=({k: np.array(meta[k]) for k in meta}, packed))

    @property
    def native(self):
        """the kernels serve this dataset (otherwise: the reference's tables on the host)"""
        return ops._on_device(torch.empty(0, device=self.device)) and ops.multiscale_kernels_available()

    def _init_load(self, loaded=None):
        if loaded is None:
            if self.cfg.get('dataset_type', 'multiscale') != 'multiscale':
                raise NotImplementedError('MipMultiScaleDataset: dataset_type %r is not supported (multiscale is)' % (self.cfg.dataset_type,))
            self.meta, images, self.n_examples = load_multiscale_data(self.cfg.datadir, self.mode, self.cfg.white_bkgd)
        else:
            self.meta, images = loaded
            self.n_examples = len(self.meta['height'])
        self.table = self.images = self.rays = None
        if self.native:
            self.table = CameraTable(self.meta, images, self.device)
            return
        m = self.meta
        sizes = [(int(h), int(w)) for h, w in zip(m['height'], m['width'])]
        if isinstance(images, torch.Tensor):                      # packed [total, 3]: back to one array per image
            offs = np.concatenate([[0], np.cumsum([h * w for h, w in sizes])])
            images = [images[int(offs[i]):int(offs[i + 1])].cpu().numpy().reshape(h, w, 3) for i, (h, w) in enumerate(sizes)]
        frames = [_frame_rays(m['pix2cam'][i], m['cam2world'][i], h, w, m['lossmult'][i], m['near'][i], m['far'][i]) for i, (h, w) in enumerate(sizes)]
        if self.mode == 'train':                                  # flatten(): one fp32 table per key
            flat = lambda xs: torch.tensor(np.concatenate([x.reshape(-1, x.shape[-1]) for x in xs], 0), dtype=torch.float32).to(self.device)
            self.images = flat(images)
            self.rays = {k: flat([f[k] for f in frames]) for k in RAY_KEYS}
        else:
            up = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float32).to(self.device)
            self.images = [up(im) for im in images]
            self.rays = {k: [up(f[k]) for f in frames] for k in RAY_KEYS}

    def _init_pipeline(self, pipeline):
        self.pipeline = Compose(pipeline)
        for t in self.pipeline.transforms:
            if isinstance(t, MipMultiScaleSample):
                t.seed = self.seed

    def _fetch_train_data(self, idx):
        if self.table is not None:
            return {TABLE_KEY: self.table}
        data = {'target_s': self.images}
        data.update(self.rays)
        return data

    def _fetch_test_data(self, idx):
        """one test example: the frame, its index and its seven ray arrays [H, W, .]"""
        idx = int(idx)
        if self.table is not None:
            datas = {'image': self.table.image(idx), 'idx': idx, TABLE_KEY: self.table}
            datas.update(self.table.frame(idx))
            return datas
        datas = {'image': self.images[idx], 'idx': idx}
        for key in RAY_KEYS:
            datas[key] = self.rays[key][idx]
        return datas

    def set_iter(self, iter_n):
        self.iter_n = iter_n

    def __getitem__(self, idx):
        data = self.pipeline(self._fetch_train_data(idx) if self.mode == 'train' else self._fetch_test_data(idx))
        if data is not None:
            data.pop(TABLE_KEY, None)
        return data

    def __len__(self):
        return self.n_examples


# ------------------------------------------------------------------------------------------ the converter
def _load_renderings(data_dir, split):
    """convert_blender_data.py:19-40, the images kept as the bytes they are"""
    from PIL import Image
    with open(os.path.join(data_dir, 'transforms_{}.json'.format(split)), 'r') as fp:
        meta = json.load(fp)
    images, cams = [], []
    for frame in meta['frames']:
        with open(os.path.join(data_dir, frame['file_path'] + '.png'), 'rb') as imgin:
            images.append(np.array(Image.open(imgin), dtype=np.uint8))
        cams.append(frame['transform_matrix'])
    images = np.stack(images, axis=0)
    if images.ndim != 4 or images.shape[3] not in (3, 4):
        raise ValueError('convert_blender_scene: RGB or RGBA images expected (got %r)' % (images.shape,))
    return images, np.stack(cams, axis=0), .5 * images.shape[2] / np.tan(.5 * float(meta['camera_angle_x']))


def convert_blender_scene(blenderdir, outdir=None, n_down=4, device=None, white_bkgd=True, splits=('train', 'val', 'test')):
    """tools/convert_blender_data.py for one scene -> {split: (meta, packed images [total, 3] fp32 on `device`)}: the 2x2 box pyramid with an
    8-bit requantisation per level (ops.ms_pyramid on the device, numpy on the host) and the reference's metadata.  With outdir it also
    writes images_{split}/{i:03d}_d{j}.png and metadata.json in the reference's layout."""
    device = torch.device(device) if device is not None else torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
    native = ops._on_device(torch.empty(0, device=device)) and ops.multiscale_kernels_available()
    out, bigmeta = {}, {}
    for split in splits:
        base, camtoworlds, f = _load_renderings(blenderdir, split)
        N, H, W, Cn = base.shape
        sizes = ops.ms_pyramid_sizes(H, W, n_down)
        if native:
            got = ops.ms_pyramid(torch.from_numpy(base).to(device), n_down, white_bkgd, want=('bytes', 'pixels') if outdir else ('pixels',))
            packed, saved = got['pixels'], got.get('bytes')
        else:
            saved, packed = _host_pyramid(base, n_down, white_bkgd)
            packed = torch.from_numpy(packed).to(device)
        meta = {k: [] for k in META_KEYS if k != 'pix2cam'}
        imgdir = 'images_{}'.format(split)
        for i in range(N):
            for j, (h, w) in enumerate(sizes):
                meta['file_path'].append('{}/{:03d}_d{}.png'.format(imgdir, i, j))
                meta['width'].append(w)
                meta['height'].append(h)
                meta['focal'].append(f / 2**j)
                meta['cam2world'].append(camtoworlds[i].tolist())
                meta['lossmult'].append(4.**j)
                meta['label'].append(j)
                meta['near'].append(2.)
                meta['far'].append(6.)
        fx = fy = np.array(meta['focal'])
        cx, cy = np.array(meta['width']) * .5, np.array(meta['height']) * .5
        arr0, arr1 = np.zeros_like(cx), np.ones_like(cx)
        k_inv = np.array([[arr1 / fx, arr0, -cx / fx], [arr0, -arr1 / fy, cy / fy], [arr0, arr0, -arr1]])
        meta['pix2cam'] = np.moveaxis(k_inv, -1, 0).tolist()
        if outdir:
            from PIL import Image
            os.makedirs(os.path.join(outdir, imgdir), exist_ok=True)
            saved = saved.cpu().numpy() if isinstance(saved, torch.Tensor) else saved
            at = 0
            for name, h, w in zip(meta['file_path'], meta['height'], meta['width']):
                with open(os.path.join(outdir, name), 'wb') as imgout:
                    Image.fromarray(saved[at:at + h * w].reshape(h, w, Cn)).save(imgout)
                at += h * w
        bigmeta[split] = meta
        out[split] = (meta, packed)
    if outdir:
        with open(os.path.join(outdir, 'metadata.json'), 'w') as fp:
            json.dump(bigmeta, fp, ensure_ascii=False, indent=4)
    return out
