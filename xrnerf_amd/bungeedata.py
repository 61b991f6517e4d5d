"""BungeeNeRF data on the device: BungeeDataset, BungeeBatchSample, BungeeGetBounds, BungeeGetZvals and the Compose planner that runs a
training item as one xr_bgd_item launch and a validation frame as one xr_bgd_frame launch -- the data side of
configs/bungeenerf/bungeenerf_multiscale_google.py.

Mirrors, relative to the reference's tree:
  xrnerf/datasets/bungee_dataset.py                     BungeeDataset
  xrnerf/datasets/load_data/load.py:145-171             load_data, the 'mutiscale_google' branch
  xrnerf/datasets/load_data/get_rays.py:156-206         get_rays_np_bungee, load_rays_bungee (the kernel)
  xrnerf/datasets/pipelines/create.py:116-145           BungeeBatchSample      create.py:539-576   BungeeGetZvals      create.py:835-915   BungeeGetBounds

The reference materialises, for every pixel of every train image, nine doubles (o, d, rgb), a double radius and an int64 scale code -- 88
bytes per ray -- and shuffles them on the host.  Here a train split keeps the images (12 bytes per ray), twelve doubles and one code per
IMAGE, and the permutation of the flat ray indices (8 bytes per ray); an item makes the rays of its slice of the permutation
(xrnerf_amd/csrc/xr_bungeedata.hip).  BungeeState.materialise() gives the reference's three tables as plain tensors for callers who want them.

Deviations from the reference:
  * items are fp32, each value rounded from the reference's float64 once (the deviation of section 21)
  * the permutation is torch.randperm from a host generator seeded `seed`, drawn once per stage (the reference draws from the global
    generator at construction); `perm=` replaces the draw
  * PerturbZvals reads an optional results['t_rand'], popped after use (as in section 20)
There is no host path for the training rays: without the library, or with device='cpu', a train split raises (val / test splits need no
kernel until a frame is rendered).
"""
import numpy as np
import torch

from . import bungee, ops, pipelines
from .pipelines import DATASETS, PIPELINES, DeleteUseless, FlattenRays, GetRays, GetViewdirs, PerturbZvals, ToTensor

STATE_KEY = 'bungee_state'          # the results key a BungeeState travels under


def scale_codes(n, n_images, scale_split, cur_stage):
    """load_rays_bungee's codes for the n images of a stage: the first n_images - scale_split[0] get 0, the next scale_split[0] -
    scale_split[1] get 1, ...; ValueError when they do not number n"""
    codes, prev = [], int(n_images)
    for cur, spl in enumerate(list(scale_split)[:int(cur_stage) + 1]):
        codes += [cur] * (prev - int(spl))
        prev = int(spl)
    if len(codes) != n or not 0 <= int(cur_stage) < len(scale_split):
        raise ValueError('BungeeDataset: %d images at stage %d, but scale_split %s of %d images gives %d scale codes'
                         % (n, cur_stage, list(scale_split), n_images, len(codes)))
    return np.asarray(codes, np.int64)


class BungeeState:
    """the device-resident form of a train split: images [n,H,W,3] fp32, cams [n,12] double (cam2world rows 0..2), codes [n] int64,
    i_train [T] int32 and the permutation [T H W] int64 of the flat ray indices"""

    def __init__(self, H, W, focal, poses, images, codes, i_train, device, seed=0, perm=None):
        self.H, self.W, self.focal = int(H), int(W), float(focal)
        if self.H < 3:                    # dx[:, -2:-1] is empty below 3 rows: the reference returns fewer radii than rays
            raise ValueError('BungeeDataset: training rays need H >= 3 (got %d)' % self.H)
        self.device = torch.device(device)
        poses = np.ascontiguousarray(np.asarray(poses, np.float64)[:, :3, :4])
        n, i_train = poses.shape[0], np.asarray(i_train, np.int64).reshape(-1)
        if len(codes) != n or images.shape[0] != n or i_train.size < 1 or i_train.min() < 0 or i_train.max() >= n:
            raise ValueError('BungeeDataset: %d poses, %d images, %d codes, i_train %r' % (n, images.shape[0], len(codes), i_train.tolist()[:8]))
        self.cams = torch.from_numpy(poses.reshape(n, ops.BGD_CAM_DOUBLES)).to(self.device)
        self.codes = torch.from_numpy(np.asarray(codes, np.int64)).to(self.device)
        self.images = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images, dtype=np.float32))
        self.images = self.images.to(self.device)
        self.i_train = torch.from_numpy(i_train.astype(np.int32)).to(self.device)
        total = int(i_train.size) * self.H * self.W
        if perm is None:                  # load_rays_bungee's draw, from a generator of its own
            perm = torch.randperm(total, generator=torch.Generator().manual_seed(int(seed)))
        else:                             # a caller's: checked once, where it lives (one pass: every index met exactly once)
            perm = torch.as_tensor(perm).to(torch.int64).reshape(-1)
            inside = perm.numel() == total and bool(((perm >= 0) & (perm < total)).all())
            if not inside or not bool((torch.bincount(perm, minlength=total) == 1).all()):
                raise ValueError('BungeeDataset: perm must be a permutation of the %d rays' % total)
        self.perm = perm.to(self.device)

    def __len__(self):
        return int(self.perm.shape[0])

    def bytes_per_ray(self):
        """resident bytes per training ray (the reference's tables take 88)"""
        tables = sum(t.numel() * t.element_size() for t in (self.cams, self.codes, self.i_train, self.perm))
        return (len(self) * 3 * self.images.element_size() + tables) / float(len(self))      # the train images' pixels, from the shapes

    def item(self, idx, N_rand, **kw):
        """rows idx N_rand .. (idx + 1) N_rand of the shuffled rays: one launch"""
        return ops.bgd_item(self.cams, self.codes, self.images, self.i_train, self.H, self.W, self.focal, self.perm, int(N_rand) * int(idx), int(N_rand), **kw)

    def materialise(self):
        """the reference's shuffled tables as fp32 / int64 device tensors: rays_rgb [T H W,3,3], radii [.,1], scale_code [.,1]"""
        got = ops.bgd_item(self.cams, self.codes, self.images, self.i_train, self.H, self.W, self.focal, self.perm, 0, len(self),
                           want=('rays_o', 'rays_d', 'target_s', 'radii', 'scale_code'))
        return {'rays_rgb': torch.stack([got['rays_o'], got['rays_d'], got['target_s']], 1), 'radii': got['radii'], 'scale_code': got['scale_code']}


# ------------------------------------------------------------------------------------------ the transforms
@PIPELINES.register_module()
class BungeeBatchSample:
    """rows idx N_rand .. (idx + 1) N_rand of the shuffled rays (create.py:116-145).  Handed the materialised rays_rgb / radii / scale_code
    it slices them; handed the dataset's BungeeState (results['bungee_state']) it makes the rows in one launch."""

    def __init__(self, enable=True, N_rand=1024, **kwargs):
        self.enable, self.N_rand, self.kwargs = enable, N_rand, kwargs

    def __call__(self, results):
        if self.enable:
            state = results.pop(STATE_KEY, None)
            if state is not None:
                results.update(state.item(results['idx'], self.N_rand, want=('rays_o', 'rays_d', 'target_s', 'radii', 'scale_code')))
            else:
                start = self.N_rand * int(results['idx'])
                rows = results['rays_rgb'][start:start + self.N_rand]
                results['rays_o'], results['rays_d'], results['target_s'] = rows[:, 0, :], rows[:, 1, :], rows[:, 2, :]
                results['radii'] = results['radii'][start:start + self.N_rand]
                results['scale_code'] = results['scale_code'][start:start + self.N_rand]
        return results

    def __repr__(self):
        return '{}:sample a batch of rays from all rays'.format(self.__class__.__name__)


@PIPELINES.register_module()
class BungeeGetBounds:
    """near / far of every ray from the globe ('sphere') or the ground planes ('flat') (create.py:835-915): ops.bungee_zvals' bounds"""

    def __init__(self, enable=True, ray_nearfar='sphere', **kwargs):
        if ray_nearfar not in ('sphere', 'flat'):
            raise ValueError("BungeeGetBounds: ray_nearfar must be 'sphere' or 'flat' (got %r)" % (ray_nearfar,))
        self.enable, self.ray_nearfar, self.kwargs = enable, ray_nearfar, kwargs

    def scene(self):
        return dict(ray_nearfar=self.ray_nearfar, scene_origin=tuple(float(v) for v in np.asarray(self.kwargs['scene_origin']).reshape(-1)),
                    scaling=float(self.kwargs['scene_scaling_factor']))

    def __call__(self, results):
        if self.enable:
            o, v = results['rays_o'].contiguous(), results['viewdirs'].contiguous()      # a table's columns are strided views
            results['near'], results['far'], _ = ops.bungee_zvals(o, v, None, None, 2, **self.scene())
        return results

    def __repr__(self):
        return '{}:get bounds(near and far)'.format(self.__class__.__name__)


@PIPELINES.register_module()
class BungeeGetZvals:
    """N_samples edges per ray, the first two thirds linear in disparity, sorted (create.py:539-576): ops.bungee_zvals' z-values"""

    def __init__(self, enable=True, N_samples=64, **kwargs):
        self.enable, self.N_samples = enable, N_samples

    def __call__(self, results):
        if self.enable:
            _, _, results['z_vals'] = ops.bungee_zvals(None, None, results['near'], results['far'], int(self.N_samples), None)
        return results


# ------------------------------------------------------------------------------------------ the fused run
class BungeeRun:
    """Compose's fourth planner: transforms[start .. end] as one launch.
    Train: [BungeeBatchSample, GetViewdirs, BungeeGetBounds, BungeeGetZvals, PerturbZvals?] over a BungeeState is ONE xr_bgd_item launch.
    Test / val: [GetRays(include_radius=True), FlattenRays(include_radius=True), GetViewdirs, BungeeGetBounds, BungeeGetZvals] over a
    pose is ONE xr_bgd_frame launch.  ToTensor / DeleteUseless steps inside the run are applied after it."""
    _TRAIN = (BungeeBatchSample, GetViewdirs, BungeeGetBounds, BungeeGetZvals)
    _FRAME = (GetRays, FlattenRays, GetViewdirs, BungeeGetBounds, BungeeGetZvals)
    _PRODUCED = ('rays_o', 'rays_d', 'target_s', 'radii', 'scale_code', 'viewdirs', 'near', 'far', 'z_vals', 'src_shape')

    def __init__(self, start, end, steps, side):
        self.start, self.end, self.side = start, end, side
        by = {type(t): t for t in steps}
        self.sample, self.rays, self.bounds, self.zvals, self.perturb = by.get(BungeeBatchSample), by.get(GetRays), by[BungeeGetBounds], by[BungeeGetZvals], PerturbZvals in by

    @staticmethod
    def plan(transforms):
        enabled = lambda t: getattr(t, 'enable', True)
        start = next((i for i, t in enumerate(transforms) if type(t) in (BungeeBatchSample, GetRays) and enabled(t)), None)
        ends = [i for i, t in enumerate(transforms) if type(t) in (BungeeGetZvals, PerturbZvals) and enabled(t)]
        if start is None or not ends or ends[-1] < start:
            return None
        end, steps, side = ends[-1], [], []
        for t in transforms[start:end + 1]:
            if not enabled(t):
                continue
            (side if type(t) in (ToTensor, DeleteUseless) else steps).append(t)
        kinds = tuple(type(t) for t in steps)
        train = kinds in (BungeeRun._TRAIN, BungeeRun._TRAIN + (PerturbZvals,))
        if not train and (kinds != BungeeRun._FRAME or not steps[0].include_radius or not steps[1].include_radius):
            return None                                            # a perturbed frame, a foreign step or another order: step by step
        if any(k in BungeeRun._PRODUCED for t in side if type(t) is DeleteUseless for k in t.keys):
            return None
        return BungeeRun(start, end, steps, side)

    def ready(self, results):
        if not ops.bungeedata_kernels_available():
            return False
        if self.sample is not None:
            state = results.get(STATE_KEY)
            return isinstance(state, BungeeState) and ops._on_device(state.cams) and 'idx' in results
        pose = results.get('pose')
        return isinstance(pose, torch.Tensor) and pose.dtype == torch.float32 and ops._on_device(pose) and pose.dim() == 2 and pose.shape[0] >= 3 and pose.shape[1] >= 4

    def __call__(self, results):
        S, scene = int(self.zvals.N_samples), self.bounds.scene()
        if self.sample is not None:
            state, n_rand = results.pop(STATE_KEY), int(self.sample.N_rand)
            kw = {}
            if self.perturb:
                n = max(0, min(n_rand, len(state) - n_rand * int(results['idx'])))
                t_rand = results.pop('t_rand', None)
                kw['t_rand'] = torch.rand((n, S), device=state.device) if t_rand is None else t_rand.to(state.device)
            results.update(state.item(results['idx'], n_rand, S=S, **scene, **kw))
        else:
            H, W, K = self.rays.kwargs['H'], self.rays.kwargs['W'], self.rays.kwargs['K']
            results.update(ops.bgd_frame(results['pose'][:3, :4], H, W, K, S=S, **scene))
            results['src_shape'] = torch.tensor((H, W, 3))
        for t in self.side:
            if type(t) is ToTensor:
                for k in t.keys:
                    if k in results:
                        results[k] = pipelines.to_tensor(results[k])
            else:
                results = t(results)
        return results


# ------------------------------------------------------------------------------------------ the dataset
@DATASETS.register_module()
class BungeeDataset(pipelines.SceneBaseDataset):
    """the reference's BungeeDataset (bungee_dataset.py) for dataset_type 'mutiscale_google', device-resident.  set_stage(k) moves the
    dataset to another stage without reading the files again (the reference builds a new dataset per stage)."""

    def __init__(self, cfg, pipeline, device=None, seed=0, perm=None):
        self.cur_stage = int(dict(cfg)['cur_stage'])
        self._perm, self._pipeline_cfg = perm, pipeline
        super().__init__(cfg, pipeline, device=device, seed=seed)

    def _init_load(self):
        cfg = self.cfg
        if cfg.get('dataset_type', 'mutiscale_google') != 'mutiscale_google':
            raise NotImplementedError('BungeeDataset: dataset_type %r is not supported (mutiscale_google is)' % (cfg.dataset_type,))
        images, poses, self.scene_scaling_factor, self.scene_origin, self.scale_split = bungee.load_google_data(cfg.datadir, cfg.factor)
        self.n_images = len(images)                                # before the stage's slice
        if cfg.white_bkgd:
            images = images[..., :3] * images[..., -1:] + (1. - images[..., -1:])
        else:
            images = images[..., :3]
        self._all_images = torch.from_numpy(np.ascontiguousarray(images, dtype=np.float32)).to(self.device)
        self._all_poses = poses
        H, W, focal = poses[0, :3, -1]
        H, W = int(H), int(W)
        self.hwf = [H, W, focal]
        self.K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
        self._load_stage(self.cur_stage, self._perm)

    def _load_stage(self, stage, perm=None):
        """load.py:159-171 and load_rays_bungee's bookkeeping for one stage"""
        cfg, stage = self.cfg, int(stage)
        if not 0 <= stage < len(self.scale_split):
            raise ValueError('BungeeDataset: stage %d of %d' % (stage, len(self.scale_split)))
        first = int(self.scale_split[stage])
        images, poses = self._all_images[first:], self._all_poses[first:, :3, :4]
        n = int(images.shape[0])
        codes = scale_codes(n, self.n_images, self.scale_split, stage)
        if cfg.holdout > 0:
            self.i_test = np.arange(n)[::cfg.holdout]
        self.i_val = self.i_test
        self.i_train = np.array([i for i in np.arange(n) if i not in self.i_test])
        self.cur_stage, self.images = stage, images
        self.poses = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float32)).to(self.device)
        self.render_poses = self.poses[torch.as_tensor(self.i_test, dtype=torch.int64)]
        self.state = None
        if self.is_batching and self.mode == 'train':
            self.N_rand = cfg.N_rand_per_sampler
            self.state = BungeeState(self.hwf[0], self.hwf[1], self.hwf[2], poses, images, codes, self.i_train, self.device, seed=self.seed, perm=perm)

    def set_stage(self, stage, perm=None):
        """the dataset a fresh BungeeDataset(cfg with cur_stage=stage) would be: images, cameras, codes and the permutation re-sliced"""
        self._load_stage(stage, perm)
        self._init_pipeline(self._pipeline_cfg)

    def get_info(self):
        return {'H': self.hwf[0], 'W': self.hwf[1], 'focal': self.hwf[2], 'K': self.K, 'render_poses': self.render_poses, 'hwf': self.hwf,
                'cur_stage': self.cur_stage, 'scene_origin': self.scene_origin, 'scene_scaling_factor': self.scene_scaling_factor,
                'scale_split': self.scale_split}

    def _fetch_train_data(self, idx):
        if self.is_batching:
            data = {STATE_KEY: self.state, 'idx': idx}
        else:
            data = {'poses': self.poses, 'images': self.images, 'n_images': self.n_images, 'i_data': self.i_train, 'idx': idx}
        data['iter_n'] = self.iter_n
        return data

    def __getitem__(self, idx):
        data = super().__getitem__(idx)
        if data is not None:
            data.pop(STATE_KEY, None)
        return data

    def __len__(self):
        if self.mode == 'train':
            return len(self.state) // self.N_rand if self.is_batching else self.i_train.shape[0]
        return 1 if self.mode == 'val' else len(self.i_test)
