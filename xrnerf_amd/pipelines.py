"""Scene data pipelines on the device: the DATASETS / PIPELINES registries, Compose, the per-item transforms that
configs/nerf/nerf_blender_base01.py, configs/nerf/nerf_llff_base01.py and configs/mipnerf/mipnerf_blender.py list as `train_pipeline` /
`test_pipeline`, and SceneBaseDataset.

Mirrors, relative to the reference's xrnerf/:
  datasets/builder.py:8-23                    DATASETS, PIPELINES, build_dataset
  datasets/pipelines/compose.py:13-100        Compose, to_tensor, ToTensor
  datasets/pipelines/create.py                Sample, BatchSample, GetRays, GetViewdirs, GetBounds, GetZvals, GetPts, DeleteUseless
  datasets/pipelines/augment.py:12-80,261-286 SelectRays, PerturbZvals
  datasets/pipelines/transforms.py:10-86      ToNDC, FlattenRays
  datasets/base.py, scene_dataset.py          BaseDataset._init_pipeline / set_iter, SceneBaseDataset
  datasets/load_data/load.py:18-68,177-189    load_data (llff and blender branches)
  core/hooks/validation_hooks.py:13-21, train_hooks.py:12-23   SetValPipelineHook, PassIterHook

Every transform, called on its own, runs the reference's tensor ops on whatever device its inputs live on.  Compose plans once, at
construction: a run that starts at GetRays (or BatchSample) and ends at the last of GetZvals / PerturbZvals / GetPts is executed as ONE
xr_pipe_ray_front launch (xrnerf_amd/csrc/xr_pipeline.hip) when its inputs are fp32 device tensors -- the SelectRays gather, the precrop
window and the target gather included; only the selected pixels are ever touched.

Deviations from the reference (documented in DESIGN.md section 20):
  * the draws come from torch's generator on the data's device, not from a host generator seeded with time(): another stream, the same
    distribution (SelectRays still draws without replacement).  SelectRays reads an optional results['select_inds'], PerturbZvals and
    GetZvals an optional results['t_rand']; both are popped after use
  * images and poses are uploaded once and stay on the device; with is_batching the [N H W, 3, 3] table is built and shuffled there
"""
from collections.abc import Sequence

import numpy as np
import torch

from . import builder, datasets as _datasets, ops

PIPELINES = builder.Registry('pipeline')
DATASETS = builder.Registry('dataset')


def build_dataset(cfg, default_args=None):
    return DATASETS.build(cfg, default_args)


# ------------------------------------------------------------------------------------------ formatting
def to_tensor(data):
    """compose.py:56-73"""
    if isinstance(data, torch.Tensor):
        return data
    if isinstance(data, np.ndarray):
        return torch.from_numpy(data)
    if isinstance(data, Sequence) and not isinstance(data, str):
        return torch.tensor(data)
    if isinstance(data, int):
        return torch.LongTensor([data])
    if isinstance(data, float):
        return torch.FloatTensor([data])
    raise TypeError('type %s cannot be converted to tensor.' % type(data))


@PIPELINES.register_module()
class ToTensor:
    def __init__(self, keys, **kwargs):
        self.keys, self.kwargs = keys, kwargs

    def __call__(self, results):
        for key in self.keys:
            results[key] = to_tensor(results[key])
        return results

    def __repr__(self):
        return '%s(keys=%s)' % (self.__class__.__name__, self.keys)


@PIPELINES.register_module()
class DeleteUseless:
    def __init__(self, enable=True, keys=[], **kwargs):
        self.enable, self.keys = enable, keys

    def __call__(self, results):
        if self.enable:
            for k in self.keys:
                results.pop(k, None)
        return results


# ------------------------------------------------------------------------------------------ sources of rays
@PIPELINES.register_module()
class Sample:
    """one image and its pose (create.py:29-41)"""

    def __init__(self, enable=True, N_rand=1024, **kwargs):
        self.enable, self.kwargs = enable, kwargs

    def __call__(self, results):
        if self.enable:
            img_i = results['i_data'][results['idx']]
            results['pose'] = results['poses'][img_i, :3, :4]
            results['target_s'] = results['images'][img_i]
        return results


@PIPELINES.register_module()
class BatchSample:
    """rows idx N_rand .. (idx + 1) N_rand of the shuffled ray table (create.py:93-108)"""

    def __init__(self, enable=True, N_rand=1024, **kwargs):
        self.enable, self.N_rand, self.kwargs = enable, N_rand, kwargs

    def rows(self, results):
        start = self.N_rand * int(results['idx'])
        return results['rays_rgb'][start:start + self.N_rand]

    def __call__(self, results):
        if self.enable:
            rows = self.rows(results)
            results['rays_o'], results['rays_d'], results['target_s'] = rows[:, 0, :], rows[:, 1, :], rows[:, 2, :]
        return results


@PIPELINES.register_module()
class GetRays:
    """rays of every pixel of the frame (create.py:211-245)"""

    def __init__(self, enable=True, include_radius=False, **kwargs):
        self.enable, self.kwargs, self.include_radius = enable, kwargs, include_radius

    def __call__(self, results):
        if self.enable:
            pose = results['pose']
            c2w = pose[:3, :4]
            H, W, K = self.kwargs['H'], self.kwargs['W'], self.kwargs['K']
            if self.include_radius and H < 3:              # dx[-2:-1] is empty below 3 rows: the reference returns fewer radii than rays
                raise ValueError('GetRays(include_radius=True) needs H >= 3 (got %d)' % H)
            dev = pose.device
            j, i = torch.meshgrid(torch.linspace(0, H - 1, H, device=dev), torch.linspace(0, W - 1, W, device=dev), indexing='ij')
            dirs = torch.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -torch.ones_like(i)], -1)
            rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)
            results['rays_d'] = rays_d
            results['rays_o'] = c2w[:3, -1].expand(rays_d.shape)
            if self.include_radius:
                dx = torch.sqrt(torch.sum((rays_d[:-1, :, :] - rays_d[1:, :, :]) ** 2, -1))
                dx = torch.cat([dx, dx[-2:-1, :]], 0)
                results['radii'] = dx[..., None] * 2 / torch.sqrt(torch.tensor(12)).to(dev)
        return results


@PIPELINES.register_module()
class KilonerfGetRays(GetRays):
    """GetRays under the name the KiloNeRF configs use (create.py:253-299).  The reference binds an external kilonerf_cuda.get_rays_d that
    is not in its tree; the commented block beside the call is GetRays' arithmetic, which is what runs here.  expand_origin=False leaves
    rays_o the [3] origin."""

    def __init__(self, enable=True, expand_origin=True, **kwargs):
        super().__init__(enable=enable, include_radius=False, **kwargs)
        self.expand_origin = expand_origin

    def __call__(self, results):
        results = super().__call__(results)
        if self.enable and not self.expand_origin:
            results['rays_o'] = results['pose'][:3, -1].contiguous()
        return results


@PIPELINES.register_module()
class SelectRays:
    """sel_n pixels of the frame (of its centre window during the first precrop_iters iterations), drawn without replacement
    (augment.py:37-76).  results['select_inds'] (indices into the window's row-major pixel list), when present, replaces the draw."""

    def __init__(self, enable=True, sel_n=1024, precrop_iters=0, precrop_frac=0.5, include_radius=False, **kwargs):
        self.enable, self.precrop_iters, self.precrop_frac = enable, precrop_iters, precrop_frac
        self.kwargs, self.sel_n, self.include_radius = kwargs, sel_n, include_radius

    def window(self, results):
        """(first row, first column, rows, columns) of the pixels the draw is made from"""
        H, W = self.kwargs['H'], self.kwargs['W']
        if self.precrop_iters != 0 and results['iter_n'] < self.precrop_iters:
            dH, dW = int(H // 2 * self.precrop_frac), int(W // 2 * self.precrop_frac)
            return H // 2 - dH, W // 2 - dW, 2 * dH, 2 * dW
        return 0, 0, H, W

    def pixels(self, results, device):
        """(h, w) int64 tensors on `device`: the selected pixels; pops results['select_inds']"""
        h0, w0, nh, nw = self.window(results)
        inds = results.pop('select_inds', None)
        if inds is None:
            if self.sel_n > nh * nw:
                raise ValueError('Cannot take a larger sample than population when replace is False')
            inds = torch.randperm(nh * nw, device=device)[:self.sel_n]
        inds = torch.as_tensor(inds).to(device=device, dtype=torch.int64)
        return h0 + torch.div(inds, nw, rounding_mode='floor'), w0 + inds % nw

    def __call__(self, results):
        if self.enable:
            h, w = self.pixels(results, results['rays_d'].device)
            for k in ('rays_o', 'rays_d', 'target_s') + (('radii',) if self.include_radius else ()):
                results[k] = results[k][h, w]
        return results


@PIPELINES.register_module()
class FlattenRays:
    """(H, W, ..) -> (H W, ..), the frame's shape kept in src_shape (transforms.py:70-82)"""

    def __init__(self, enable=True, include_radius=False, **kwargs):
        self.enable, self.include_radius = enable, include_radius

    def __call__(self, results):
        if self.enable:
            src_shape = results['rays_d'].shape
            results['rays_o'] = torch.reshape(results['rays_o'], [-1, 3]).float()
            results['rays_d'] = torch.reshape(results['rays_d'], [-1, 3]).float()
            if self.include_radius:
                results['radii'] = torch.reshape(results['radii'], [-1, 1]).float()
            results['src_shape'] = torch.tensor(src_shape)
        return results


# ------------------------------------------------------------------------------------------ per-ray steps
@PIPELINES.register_module()
class GetViewdirs:
    def __init__(self, enable=True, **kwargs):
        self.enable = enable

    def __call__(self, results):
        if self.enable:
            d = results['rays_d']
            results['viewdirs'] = torch.reshape(d / torch.norm(d, dim=-1, keepdim=True), [-1, 3]).float()
        return results


@PIPELINES.register_module()
class ToNDC:
    """normalized device coordinates of a forward-facing scene (transforms.py:27-47), near plane at 1"""

    def __init__(self, enable=True, **kwargs):
        self.enable, self.H, self.W, self.K = enable, kwargs['H'], kwargs['W'], kwargs['K']

    def __call__(self, results):
        if self.enable:
            results['rays_o'], results['rays_d'] = self.ndc_rays(self.H, self.W, self.K[0][0], 1., results['rays_o'], results['rays_d'])
        return results

    @staticmethod
    def ndc_rays(H, W, focal, near, rays_o, rays_d):
        fw, fh = ops.pipe_ndc_factors(H, W, focal)
        t = -(near + rays_o[..., 2]) / rays_d[..., 2]
        rays_o = rays_o + t[..., None] * rays_d
        ox, oy, oz = rays_o[..., 0] / rays_o[..., 2], rays_o[..., 1] / rays_o[..., 2], rays_o[..., 2]
        o = torch.stack([fw * rays_o[..., 0] / oz, fh * rays_o[..., 1] / oz, 1. + 2. * near / oz], -1)
        d = torch.stack([fw * (rays_d[..., 0] / rays_d[..., 2] - ox), fh * (rays_d[..., 1] / rays_d[..., 2] - oy), -2. * near / oz], -1)
        return o, d


@PIPELINES.register_module()
class GetBounds:
    def __init__(self, enable=True, near_new=None, far_new=None, **kwargs):
        self.enable = enable
        self.near = near_new if near_new is not None else kwargs['near']
        self.far = far_new if far_new is not None else kwargs['far']

    def __call__(self, results):
        if self.enable:
            ones = torch.ones_like(results['rays_d'][..., :1])
            results['near'], results['far'] = self.near * ones, self.far * ones
        return results


def _perturb(z_vals, t_rand):
    """one draw inside each sample's bin (augment.py:276-282, create.py:519-525)"""
    mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
    upper, lower = torch.cat([mids, z_vals[..., -1:]], -1), torch.cat([z_vals[..., :1], mids], -1)
    if t_rand is None:
        t_rand = torch.rand(z_vals.shape, device=z_vals.device)
    return lower + (upper - lower) * t_rand.to(z_vals.device)


@PIPELINES.register_module()
class GetZvals:
    def __init__(self, enable=True, lindisp=False, N_samples=64, randomized=False, **kwargs):
        self.enable, self.lindisp, self.N_samples, self.randomized = enable, lindisp, N_samples, randomized

    def __call__(self, results):
        if self.enable:
            t = torch.linspace(0., 1., steps=self.N_samples, device=results['rays_o'].device)
            near, far = results['near'], results['far']
            z = near * (1. - t) + far * t if not self.lindisp else 1. / (1. / near * (1. - t) + 1. / far * t)
            shape = list(results['rays_o'].shape[:-1]) + [self.N_samples]
            results['z_vals'] = _perturb(z, results.pop('t_rand', None)) if self.randomized else z.expand(shape)
        return results


@PIPELINES.register_module()
class PerturbZvals:
    def __init__(self, enable=True, **kwargs):
        self.enable = enable

    def __call__(self, results):
        if self.enable:
            results['z_vals'] = _perturb(results['z_vals'], results.pop('t_rand', None))
        return results


@PIPELINES.register_module()
class GetPts:
    def __init__(self, enable=True, **kwargs):
        self.enable = enable

    def __call__(self, results):
        if self.enable:
            results['pts'] = results['rays_o'][..., None, :] + results['rays_d'][..., None, :] * results['z_vals'][..., :, None]
        return results


# ------------------------------------------------------------------------------------------ the fused run
# the order the reference's configs list the steps in; a run is fused only when its enabled steps come in this order
_RANK = {GetRays: 0, KilonerfGetRays: 0, BatchSample: 0, SelectRays: 1, FlattenRays: 1, GetViewdirs: 2, ToNDC: 3, GetBounds: 4, GetZvals: 5, PerturbZvals: 6, GetPts: 7}
_PRODUCED = ('rays_o', 'rays_d', 'viewdirs', 'radii', 'near', 'far', 'z_vals', 'pts', 'target_s', 'src_shape')


class _FusedRun:
    """transforms[start .. end] of a Compose as one xr_pipe_ray_front call"""

    def __init__(self, start, end, steps, side):
        self.start, self.end, self.side = start, end, side
        by = {type(t): t for t in steps}
        self.rays, self.batch = by.get(GetRays) or by.get(KilonerfGetRays), by.get(BatchSample)
        self.select, self.flatten = by.get(SelectRays), by.get(FlattenRays)
        self.viewdirs, self.ndc, self.bounds = GetViewdirs in by, by.get(ToNDC), by.get(GetBounds)
        self.zvals, self.perturb, self.pts = by.get(GetZvals), PerturbZvals in by, GetPts in by

    @staticmethod
    def plan(transforms):
        """the run of `transforms` that can be fused, or None"""
        enabled = lambda t: getattr(t, 'enable', True)
        start = next((i for i, t in enumerate(transforms) if type(t) in (GetRays, KilonerfGetRays, BatchSample) and enabled(t)), None)
        ends = [i for i, t in enumerate(transforms) if type(t) in (GetZvals, PerturbZvals, GetPts) and enabled(t)]
        if start is None or not ends or ends[-1] < start:
            return None
        end, steps, side, rank = ends[-1], [], [], -1
        for t in transforms[start:end + 1]:
            if type(t) in (ToTensor, DeleteUseless):
                if enabled(t):
                    side.append(t)
            elif type(t) not in _RANK:
                return None                                        # a foreign callable inside the run: not fused
            elif enabled(t):
                if _RANK[type(t)] <= rank:
                    return None
                rank = _RANK[type(t)]
                steps.append(t)
        run = _FusedRun(start, end, steps, side)
        if not getattr(run.rays, 'expand_origin', True):           # the kernel writes one origin per ray
            return None
        radius = run.rays is not None and run.rays.include_radius
        picker = run.select or run.flatten
        if (run.rays is not None and (picker is None or picker.include_radius != radius)) or (run.batch is not None and picker is not None):
            return None
        if run.zvals is None or run.bounds is None or (run.zvals.randomized and run.perturb):
            return None
        if any(k in _PRODUCED for t in side if type(t) is DeleteUseless for k in t.keys):
            return None
        return run

    @staticmethod
    def _device_f32(t, shape_tail=None):
        return isinstance(t, torch.Tensor) and t.dtype == torch.float32 and ops._on_device(t) and (shape_tail is None or tuple(t.shape[-len(shape_tail):]) == shape_tail)

    def ready(self, results):
        """the inputs are fp32 device tensors of the expected shapes and the library has the entry point"""
        if self.batch is not None:
            ok = self._device_f32(results.get('rays_rgb'), (3, 3)) and results['rays_rgb'].dim() == 3
        else:
            pose = results.get('pose')
            ok = self._device_f32(pose) and pose.dim() == 2 and pose.shape[0] >= 3 and pose.shape[1] >= 4
            if ok and self.select is not None:
                img = results.get('target_s')
                H, W = self.rays.kwargs['H'], self.rays.kwargs['W']
                ok = self._device_f32(img) and img.dim() == 3 and tuple(img.shape[:2]) == (H, W) and img.shape[2] <= ops.PIPE_MAX_CHANNELS
        return bool(ok) and ops.pipeline_kernels_available()

    def __call__(self, results):
        z, radius = self.zvals, self.rays is not None and self.rays.include_radius
        kw = dict(with_viewdirs=self.viewdirs, ndc=self.ndc is not None, near=self.bounds.near, far=self.bounds.far, S=z.N_samples, lindisp=z.lindisp)
        want = ['rays_o', 'rays_d', 'near', 'far', 'z_vals', 'target_s'] + (['pts'] if self.pts else [])
        if self.batch is not None:
            table = self.batch.rows(results)
            H, W, K = (self.ndc.H, self.ndc.W, self.ndc.K) if self.ndc is not None else (1, 1, ((1., 0., 0.), (0., 1., 0.)))
            kw.update(table=table)
            n, dev = table.shape[0], table.device
        else:
            H, W, K = self.rays.kwargs['H'], self.rays.kwargs['W'], self.rays.kwargs['K']
            if radius and H < 3:
                raise ValueError('GetRays(include_radius=True) needs H >= 3 (got %d)' % H)
            pose = results['pose']
            dev = pose.device
            kw.update(c2w=pose[:3, :4], with_radii=radius)
            if self.select is not None:
                h, w = self.select.pixels(results, dev)
                kw.update(sel=(h * W + w).to(torch.int32), image=results['target_s'])
                n = h.shape[0]
            else:
                want.remove('target_s')
                n = H * W
                results['src_shape'] = torch.tensor((H, W, 3))
        if self.perturb or z.randomized:
            t_rand = results.pop('t_rand', None)
            kw.update(t_rand=torch.rand((n, z.N_samples), device=dev) if t_rand is None else t_rand.to(dev))
        results.update(ops.pipe_ray_front(H, W, K[0][0], K[1][1], K[0][2], K[1][2], want=want, **kw))
        for t in self.side:
            if type(t) is ToTensor:
                for k in t.keys:
                    if k in results:
                        results[k] = to_tensor(results[k])
            else:
                results = t(results)
        return results


@PIPELINES.register_module()
class Compose:
    """a sequence of transforms (config dicts or callables); returns None when a transform does (compose.py:20-45).  `fuse = False`
    forces the step-by-step tensor-op path (the timing baseline of tools/microbench_pipeline.py).  A list _FusedRun.plan leaves alone
    is offered to multiscale.MultiscaleRun.plan (the Mip-NeRF multiscale lists over a camera table), then to bodydata.BodyRun.plan (the
    NeuralBody / Animatable NeRF lists over a prepared picture), then to bungeedata.BungeeRun.plan (the BungeeNeRF lists)."""

    def __init__(self, transforms):
        assert isinstance(transforms, Sequence)
        self.transforms = []
        for transform in transforms:
            if isinstance(transform, dict):
                transform = PIPELINES.build(transform)
            elif not callable(transform):
                raise TypeError('transform must be callable or a dict, but got %s' % type(transform))
            self.transforms.append(transform)
        self.fused = _FusedRun.plan(self.transforms)
        if self.fused is None:              # the second planner: [MipMultiScaleSample, GetZvals, ToTensor ...] over a camera table
            from . import multiscale
            self.fused = multiscale.MultiscaleRun.plan(self.transforms)
        if self.fused is None:              # the third planner: [NBGetRays, NBSelectRays, ToTensor, GetZvals ...] over a prepared picture
            from . import bodydata
            self.fused = bodydata.BodyRun.plan(self.transforms)
        if self.fused is None:              # the fourth planner: [BungeeBatchSample ... BungeeGetZvals] over a BungeeState, or the frame list over a pose
            from . import bungeedata
            self.fused = bungeedata.BungeeRun.plan(self.transforms)
        self.fuse = True

    def __call__(self, data):
        i, run = 0, self.fused if self.fuse else None
        while i < len(self.transforms):
            if run is not None and i == run.start and run.ready(data):
                data, i = run(data), run.end + 1
            else:
                data, i = self.transforms[i](data), i + 1
            if data is None:
                return None
        return data

    def __repr__(self):
        return self.__class__.__name__ + '(' + ''.join('\n    %s' % t for t in self.transforms) + '\n)'


# ------------------------------------------------------------------------------------------ the dataset
def _frame_rays(H, W, K, pose, image):
    """[H W, 3, 3] rows (o, d, rgb) of one posed image, on its device: the kernel when it can, GetRays' tensor ops otherwise"""
    if ops._on_device(pose) and pose.dtype == torch.float32 and ops.pipeline_kernels_available():
        out = ops.pipe_ray_front(H, W, K[0][0], K[1][1], K[0][2], K[1][2], c2w=pose[:3, :4], image=image, want=('rays_o', 'rays_d', 'target_s'))
        return torch.stack([out['rays_o'], out['rays_d'], out['target_s']], 1)
    r = GetRays(H=H, W=W, K=K)({'pose': pose})
    return torch.stack([r['rays_o'], r['rays_d'], image], 2).reshape(-1, 3, 3)


@DATASETS.register_module()
class SceneBaseDataset:
    """the reference's SceneBaseDataset for dataset_type 'blender' and 'llff' (scene_dataset.py), device-resident: images, poses and
    (is_batching, train mode) the shuffled [N H W, 3, 3] ray table live on `device`; items are views of them"""
    is_batching = False
    mode = 'train'

    def __init__(self, cfg, pipeline, device=None, seed=0):
        self.iter_n = 0
        self.cfg = builder.ConfigDict.wrap(dict(cfg))
        if 'mode' in self.cfg: self.mode = self.cfg.mode
        if 'is_batching' in self.cfg: self.is_batching = self.cfg.is_batching
        self.device = torch.device(device) if device is not None else torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
        self.seed = seed
        self._init_load()
        self._init_pipeline(pipeline)

    def _load_data(self):
        """load.py:18-68,177-189"""
        cfg, K = self.cfg, None
        if cfg.dataset_type == 'llff':
            images, poses, bds, render_poses, i_test = _datasets.load_llff_data(cfg.datadir, cfg.factor, recenter=True, bd_factor=.75,
                                                                               spherify=cfg.get('spherify', False))
            hwf, poses = poses[0, :3, -1], poses[:, :3, :4]
            if not isinstance(i_test, list):
                i_test = [i_test]
            if cfg.llffhold > 0:
                i_test = np.arange(images.shape[0])[::cfg.llffhold]
            i_test = np.asarray(i_test)
            i_val = i_test
            i_train = np.array([i for i in np.arange(int(images.shape[0])) if i not in i_test])
            near, far = (float(np.ndarray.min(bds)) * .9, float(np.ndarray.max(bds)) * 1.) if cfg.no_ndc else (0., 1.)
        elif cfg.dataset_type == 'blender':
            images, poses, render_poses, hwf, (i_train, i_val, i_test) = _datasets.load_blender_data(cfg.datadir, cfg.half_res, cfg.testskip)
            near, far = 2., 6.
            if cfg.white_bkgd:
                images = images[..., :3] * images[..., -1:] + (1. - images[..., -1:])
            elif not ('load_alpha' in cfg and cfg.load_alpha):
                images = images[..., :3]
        elif cfg.dataset_type == 'nsvf':                           # load.py:108-143
            from . import kilodata
            images, poses, intrinsics, near, far, _, render_poses, (i_train, i_val, i_test) = kilodata.load_nsvf_dataset(
                cfg.datadir, cfg.testskip, cfg.test_traj_path if 'test_traj_path' in cfg else None)
            hwf, near, far = [intrinsics.H, intrinsics.W, intrinsics.fx], float(near), float(far)     # cx, cy, fy are not used: K is focal-centred below
            if i_test.size == 0:
                i_test = i_val
            if cfg.white_bkgd and images.shape[-1] == 4:
                images = images[..., :3] * images[..., -1:] + (1. - images[..., -1:])
            elif not ('load_alpha' in cfg and cfg.load_alpha):
                images = images[..., :3]
            render_subset = 'test' if cfg.get('render_test', False) else 'custom_path'
            if 'render_subset' in cfg:
                render_subset = cfg.render_subset
            if render_subset != 'custom_path':                     # the directory has no trajectory of its own: the poses of a split
                render_poses = np.array(poses[{'train': i_train, 'val': i_val, 'test': i_test}[render_subset]])
        else:
            raise NotImplementedError('SceneBaseDataset: dataset_type %r is not supported (blender, llff and nsvf are)' % (cfg.dataset_type,))
        H, W, focal = hwf
        H, W = int(H), int(W)
        if K is None:
            K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
        return images, poses, render_poses, [H, W, focal], K, near, far, i_train, i_val, i_test

    def _init_load(self):
        images, poses, render_poses, self.hwf, self.K, self.near, self.far, self.i_train, self.i_val, self.i_test = self._load_data()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        self.images, self.poses, self.render_poses = up(images), up(poses), up(render_poses)
        if self.is_batching and self.mode == 'train':
            self.N_rand = self.cfg.N_rand_per_sampler
            H, W = self.hwf[:2]
            rows = torch.cat([_frame_rays(H, W, self.K, self.poses[i], self.images[i]) for i in self.i_train], 0)
            g = torch.Generator(device=self.device).manual_seed(self.seed)
            self.rays_rgb = rows[torch.randperm(rows.shape[0], device=self.device, generator=g)].contiguous()

    def get_info(self):
        return {'H': self.hwf[0], 'W': self.hwf[1], 'focal': self.hwf[2], 'K': self.K, 'render_poses': self.render_poses, 'hwf': self.hwf,
                'near': self.near, 'far': self.far}

    def _init_pipeline(self, pipeline):
        datainfo = self.get_info()            # not known until the data are loaded: handed to every step
        self.pipeline = Compose([dict(step, **datainfo) if isinstance(step, dict) else step for step in pipeline])

    def _fetch_train_data(self, idx):
        if self.is_batching:
            data = {'rays_rgb': self.rays_rgb, 'idx': idx}
        else:
            data = {'poses': self.poses, 'images': self.images, 'i_data': self.i_train, 'idx': idx}
        data['iter_n'] = self.iter_n
        return data

    def _fetch_val_data(self, idx):
        return {'spiral_poses': self.render_poses, 'poses': self.poses[self.i_test], 'images': self.images[self.i_test]}

    def _fetch_test_data(self, idx):
        i = int(self.i_test[idx])
        return {'pose': self.poses[i], 'image': self.images[i], 'idx': idx}

    def set_iter(self, iter_n):
        self.iter_n = iter_n

    def __getitem__(self, idx):
        if self.mode == 'train':
            return self.pipeline(self._fetch_train_data(idx))
        if self.mode == 'val':                 # the pipeline runs inside network.val_step (SetValPipelineHook)
            return self._fetch_val_data(idx)
        return self._fetch_test_data(idx)

    def __len__(self):
        if self.mode == 'train':
            return self.rays_rgb.shape[0] // self.N_rand if self.is_batching else self.i_train.shape[0]
        return 1 if self.mode == 'val' else len(self.i_test)


def iterate(dataset):
    """the items of one pass over `dataset`, each with the leading batch axis of 1 that DataLoader(batch_size=1) collation gives and
    unfold_batching expects -- as views: no worker processes, no copy"""
    def batch(v):
        if isinstance(v, torch.Tensor):
            return v[None]
        if isinstance(v, np.ndarray):
            return torch.from_numpy(v)[None]
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            return v
        return torch.tensor([v], dtype=torch.int64 if isinstance(v, int) else torch.float64)
    for idx in range(len(dataset)):
        item = dataset[idx]
        if item is not None:
            yield {k: batch(v) for k, v in item.items()}


# ------------------------------------------------------------------------------------------ hooks
class SetValPipelineHook:
    """valset.pipeline -> model.set_val_pipeline, once (validation_hooks.py:13-21)"""

    def __init__(self, valset=None):
        self.val_pipeline = valset.pipeline

    def before_run(self, runner):
        model = getattr(runner.model, 'module', runner.model)
        model.set_val_pipeline(self.val_pipeline)
        del self.val_pipeline


class PassIterHook:
    """runner.iter -> dataset.set_iter after every training iteration (train_hooks.py:12-23)"""

    def __init__(self, dataset=None):
        self.dataset = dataset

    def after_train_iter(self, runner):
        dataset = self.dataset if self.dataset is not None else runner.data_loader.iter_loader._dataset
        dataset.set_iter(runner.iter)


from . import multiscale  # noqa: E402,F401  (registers MipMultiScaleSample and MipMultiScaleDataset: the data side of mipnerf_multiscale.py)
from . import bodydata  # noqa: E402,F401  (registers NeuralBodyDataset, AniNeRFDataset and their seven transforms: the data side of nb_zjumocap_*.py / an_*.py)
from . import genebody  # noqa: E402,F401  (registers GeneBodyDataset: the data side of gnr_genebody.py)
from . import bungeedata  # noqa: E402,F401  (registers BungeeDataset and its three transforms: the data side of bungeenerf_multiscale_google.py)
from . import kilodata  # noqa: E402,F401  (registers KiloNerfDataset, KiloNerfNodeDataset and ExampleSample: the data side of kilonerf_*.py)
from . import hashdata  # noqa: E402,F401  (registers HashNerfDataset and the four instant-ngp transforms: the data side of configs/instant_ngp/*.py)
