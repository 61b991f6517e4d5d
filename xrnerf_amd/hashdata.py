"""The data names of configs/instant_ngp/*.py in the registries: HashNerfDataset (xrnerf_amd/datasets.py) in DATASETS, and HashBatchSample,
RandomBGColor, HashGetRays and HashSetImgids in PIPELINES as plain tensor-op steps.  Training does not go through
them: the loop draws through DeviceRayTable.next_batch, which slices and composites in one launch; these make the configs' `data` dicts
resolve and serve callers who run the lists themselves.

Mirrors, relative to the reference's xrnerf/datasets/pipelines/: create.py:153-191 (HashBatchSample), create.py:356-425 (HashGetRays,
HashSetImgids), augment.py:290-317 (RandomBGColor, whose __repr__ text is the reference's own)."""
import numpy as np
import torch

from . import datasets, ops
from .pipelines import DATASETS, PIPELINES

DATASETS.register_module()(datasets.HashNerfDataset)       # the device ray table and its fused next_batch


@PIPELINES.register_module()
class HashBatchSample:
    """rows cur_i .. cur_i + N_rand of the [N, 11] table (o3, d3, rgb3, alpha, img_id), the cursor wrapping (create.py:153-191).  The
    training loop itself draws through DeviceRayTable.next_batch, which does this and RandomBGColor in one launch."""

    def __init__(self, enable=True, N_rand=1024, **kwargs):
        self.enable, self.N_rand, self.kwargs, self.cur_i = enable, N_rand, kwargs, 0

    def __call__(self, results):
        if self.enable:
            N_rand = results.pop('N_rand', self.N_rand)
            if self.cur_i + N_rand >= results['rays_rgb'].shape[0]:
                self.cur_i = 0
            rows = results['rays_rgb'][self.cur_i:self.cur_i + N_rand]
            results['rays_o'], results['rays_d'], results['target_s'] = rows[:, :3], rows[:, 3:6], rows[:, 6:9]
            results['alpha'], results['img_ids'] = rows[:, 9:10], rows[:, 10:]
            self.cur_i += N_rand
        return results

    def __repr__(self):
        return '{}:sample a batch of rays from all rays'.format(self.__class__.__name__)


@PIPELINES.register_module()
class RandomBGColor:
    """the targets composited over a random background, the background kept (augment.py:290-317); results['bg_color'], when present,
    replaces the draw (torch's generator on the data's device, not numpy's)"""

    def __init__(self, enable=True, **kwargs):
        self.enable, self.kwargs = enable, kwargs

    def __call__(self, results):
        if self.enable:
            alpha, target_s = results['alpha'], results['target_s']
            bg = results.get('bg_color')
            if bg is None:
                bg = torch.rand(target_s.shape, device=target_s.device)
            results['target_s'], results['bg_color'] = (target_s * alpha + bg * (1 - alpha)).float(), bg.float()
        return results

    def __repr__(self):
        return '{}:sample a batch of rays from all rays'.format(self.__class__.__name__)


@PIPELINES.register_module()
class HashGetRays:
    """the rays of every pixel of an NGP-space pose [4,3] (create.py:356-393, get_rays_np_hash): xr_gen_rays, as the ray table is made"""

    def __init__(self, enable=True, **kwargs):
        self.enable, self.kwargs = enable, kwargs

    def __call__(self, results):
        if self.enable:
            pose, H, W, K = results['pose'], self.kwargs['H'], self.kwargs['W'], self.kwargs['K']
            if not isinstance(pose, torch.Tensor):             # a host array: the rays are made where the library runs
                pose = torch.as_tensor(np.asarray(pose, dtype=np.float32), device='cuda:0' if torch.cuda.is_available() else 'cpu')
            dev, pose = pose.device, pose.cpu().numpy()           # xr_gen_rays takes the twelve floats as kernel arguments
            o, d = ops.gen_rays(pose, H, W, float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]), device=dev)
            results['rays_o'], results['rays_d'] = o.view(H, W, 3), d.view(H, W, 3)
        return results

    def __repr__(self):
        return "{}:get rays from pose and camera's params".format(self.__class__.__name__)


@PIPELINES.register_module()
class HashSetImgids:
    """img_ids = idx for every ray (create.py:397-425)"""

    def __init__(self, enable=True, **kwargs):
        self.enable, self.kwargs = enable, kwargs

    def __call__(self, results):
        if self.enable:
            o = results['rays_o']
            results['img_ids'] = torch.full(list(o.shape[:-1]) + [1], int(results['idx']), dtype=torch.int32, device=o.device)
        return results

    def __repr__(self):
        return '{}:get idx'.format(self.__class__.__name__)
