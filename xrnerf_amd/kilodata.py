"""KiloNeRF data: the NSVF loader, KiloNerfDataset, KiloNerfNodeDataset and ExampleSample -- the data side of
configs/kilonerf/kilonerf_{pretrain,distill,finetune}_*.py.  Host code over the existing kernels: the frames go through SceneBaseDataset
and xr_pipe_ray_front (KilonerfGetRays plans wherever GetRays does), the distillation examples through xr_kilo_distill_examples.

Mirrors, relative to the reference's tree:
  xrnerf/datasets/load_data/load_nsvf_dataset.py     load_nsvf_dataset (images read with PIL)
  xrnerf/utils/data_helper.py                        Node, calculate_volume, get_global_domain_min_and_max
  xrnerf/datasets/kilonerf_dataset.py                KiloNerfDataset
  xrnerf/datasets/kilonerf_node_dataset.py           KiloNerfNodeDataset
  xrnerf/datasets/pipelines/create.py:631-656        ExampleSample

Deviations from the reference:
  * the node dataset never holds the num_networks x num_examples_per_network x 10 float pool (20.5 GB for the shipped config): training
    item idx is kilo_distill.distill_examples(domain_mins, domain_maxs, train_batch_size, seed, idx), a function of (seed, idx) only; the
    val / test set [N, num_examples_per_network, 6] is generated once on the device.  The four target columns the reference leaves
    uninitialised are not carried
  * global_domain_min / global_domain_max of KiloNerfDataset items are fp32 tensors on the dataset's device
  * kd-tree splitting (SaveDistillResultsHook) is out of scope: the checkpoint dict is written by save_cp() and read back by batch_index > 0
"""
import os
from collections import deque

import numpy as np
import torch

from . import builder, kilo_distill
from .pipelines import DATASETS, PIPELINES, Compose, SceneBaseDataset


# ------------------------------------------------------------------------------------------ the NSVF loader
def load_matrix(path):
    with open(path) as fh:
        return np.array([[float(w) for w in line.strip().split()] for line in fh], dtype=np.float32)


def load_intrinsics(filepath):
    """a 3x3 or 4x4 matrix, or a first line `f cx cy _` (load_nsvf_dataset.py:7-32) -> [4,4]"""
    try:
        intrinsics = load_matrix(filepath)
        if intrinsics.shape[0] == 3 and intrinsics.shape[1] == 3:
            full = np.zeros((4, 4), np.float32)
            full[:3, :3] = intrinsics
            full[3, 3] = 1
            intrinsics = full
        return intrinsics
    except ValueError:                    # ragged rows: the one-line layout
        pass
    with open(filepath, 'r') as fh:
        f, cx, cy, _ = map(float, fh.readline().split())
    return np.array([[f, 0., cx, 0.], [0., f, cy, 0], [0., 0, 1, 0], [0, 0, 0, 1]])


class CameraIntrinsics:
    def __init__(self, H, W, fx, fy, cx, cy):
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = H, W, fx, fy, cx, cy


def _nsvf_pose(pose):
    """parse_extrinsics(world2camera=False) and the sign of columns 1-2"""
    if pose.shape[0] == 3 and pose.shape[1] == 4:
        pose = np.vstack([pose, np.array([[0, 0, 0, 1.0]])])
    if pose.shape[0] == 1 and pose.shape[1] == 16:
        pose = pose.reshape(4, 4)
    pose[:3, 1:3] = -pose[:3, 1:3]
    return pose


def _box_distances(point, domain_min, domain_max):
    """(distance to the closest point of the box, distance to its furthest corner) (load_nsvf_dataset.py:46-80)"""
    closest, furthest = np.array([0., 0., 0.]), np.array([0., 0., 0.])
    for dim in range(3):
        closest[dim] = domain_min[dim] if point[dim] < domain_min[dim] else (domain_max[dim] if domain_max[dim] < point[dim] else point[dim])
        furthest[dim] = domain_min[dim] if point[dim] > (domain_min[dim] + domain_max[dim]) / 2 else domain_max[dim]
    return np.linalg.norm(point - closest), np.linalg.norm(point - furthest)


def load_nsvf_dataset(path, testskip, test_traj_path=None):
    """-> (rgbs [N,H,W,C] fp32, poses [N,4,4], CameraIntrinsics, near, far, background_color or None, render_poses, [i_train, i_val, i_test])"""
    from PIL import Image
    rgb_base, pose_base = os.path.join(path, 'rgb'), os.path.join(path, 'pose')
    rgbs, poses, poses_unfiltered = [], [], []
    index, val_index, test_index = 0, 0, 0
    i_split = [[], [], []]
    for name in sorted(os.listdir(rgb_base)):
        prefix = int(name.split('_')[0])                          # 0 = train, 1 = val, 2 = test
        pose = _nsvf_pose(load_matrix(os.path.join(pose_base, name.split('.')[0] + '.txt')))
        poses_unfiltered.append(pose[None, :])
        if prefix == 0 or (prefix == 1 and val_index % testskip == 0) or (prefix == 2 and test_index % testskip == 0):
            i_split[prefix].append(index)
            with Image.open(os.path.join(rgb_base, name)) as im:
                rgbs.append((np.array(im) / 255.).astype(np.float32)[None, :])
            poses.append(pose[None, :])
            index += 1
        if prefix == 1:
            val_index += 1
        if prefix == 2:
            test_index += 1
    rgbs, poses, poses_unfiltered = np.concatenate(rgbs, 0), np.concatenate(poses, 0), np.concatenate(poses_unfiltered, 0)
    i_split = [np.array(x) for x in i_split]
    K = load_intrinsics(os.path.join(path, 'intrinsics.txt'))
    intrinsics = CameraIntrinsics(rgbs.shape[1], rgbs.shape[2], K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    near_and_far = os.path.join(path, 'near_and_far.txt')
    if os.path.isfile(near_and_far):
        near, far = load_matrix(near_and_far)[0]
    else:                                                          # from the box and ALL camera positions
        box = load_matrix(os.path.join(path, 'bbox.txt'))[0, :-1]
        near, far = float('inf'), 0.
        for position in poses_unfiltered[:, :3, -1]:
            closest, furthest = _box_distances(position, box[:3], box[3:])
            near, far = min(near, closest), max(far, furthest)
    background_color = None
    if os.path.isfile(os.path.join(path, 'background_color.txt')):
        background_color = load_matrix(os.path.join(path, 'background_color.txt'))[0]
    render_poses = np.array([])
    if test_traj_path is None:
        test_traj_path = os.path.join(path, 'test_traj.txt')
    if os.path.isfile(test_traj_path):
        render_poses = np.concatenate([_nsvf_pose(p)[None, :] for p in load_matrix(test_traj_path).reshape((-1, 4, 4))], 0)
    return rgbs, poses, intrinsics, near, far, background_color, render_poses, i_split


# ------------------------------------------------------------------------------------------ the scene dataset
def get_global_domain_min_and_max(cfg, device=None):
    """the scene's box from the cfg, or from bbox.txt of an NSVF directory (data_helper.py:35-55); fp32 tensors when a device is given"""
    if 'global_domain_min' in cfg and 'global_domain_max' in cfg:
        gmin, gmax = cfg['global_domain_min'], cfg['global_domain_max']
    elif 'datadir' in cfg and cfg['dataset_type'] == 'nsvf':
        box = load_matrix(os.path.join(cfg['datadir'], 'bbox.txt'))[0, :-1]
        gmin, gmax = box[:3], box[3:]
    else:
        raise ValueError('get_global_domain_min_and_max: the cfg has neither global_domain_min / _max nor an nsvf datadir')
    if device:
        return [torch.tensor(np.asarray(x), dtype=torch.float, device=device) for x in (gmin, gmax)]
    return gmin, gmax


@DATASETS.register_module()
class KiloNerfDataset(SceneBaseDataset):
    """SceneBaseDataset whose un-batched, val and test items carry the scene's box (kilonerf_dataset.py)"""

    def __init__(self, cfg, pipeline, device=None, seed=0):
        super().__init__(cfg, pipeline, device=device, seed=seed)
        self.global_domain_min, self.global_domain_max = get_global_domain_min_and_max(self.cfg, self.device)

    def _box(self):
        return {'global_domain_min': self.global_domain_min, 'global_domain_max': self.global_domain_max}

    def _fetch_train_data(self, idx):
        data = super()._fetch_train_data(idx)
        if not self.is_batching:
            data.update(self._box())
        return data

    def _fetch_val_data(self, idx):
        return dict(super()._fetch_val_data(idx), **self._box())

    def _fetch_test_data(self, idx):
        return dict(super()._fetch_test_data(idx), **self._box())


# ------------------------------------------------------------------------------------------ the node dataset
class Node:
    """a box of the distillation's tree (data_helper.py:7-10): domain_min, domain_max"""


def calculate_volume(domain_min, domain_max):
    return (domain_max[0] - domain_min[0]) * (domain_max[1] - domain_min[1]) * (domain_max[2] - domain_min[2])


@PIPELINES.register_module()
class ExampleSample:
    """train_batch_size examples of a materialised results['all_examples'] [N, P, .], the same slots for every network
    (create.py:631-656); results['example_indices'], when present, replaces the draw and is popped.  KiloNerfNodeDataset's own items
    carry batch_examples already and pass through."""

    def __init__(self, enable=True, train_batch_size=0, **kwargs):
        self.enable, self.train_batch_size = enable, train_batch_size

    def __call__(self, results):
        if self.enable and 'all_examples' in results:
            indices = results.pop('example_indices', None)
            if indices is None:
                indices = np.random.choice(results['all_examples'].size(1), size=(self.train_batch_size,))
            indices = torch.as_tensor(np.asarray(indices), dtype=torch.int64, device=results['all_examples'].device)
            results['batch_examples'] = results['all_examples'][:, indices]
        return results

    def __repr__(self):
        return '{}:slice a batch of examples from all examples'.format(self.__class__.__name__)


@DATASETS.register_module()
class KiloNerfNodeDataset:
    """the boxes of one distillation batch and their examples (kilonerf_node_dataset.py): cp, node_batch, domain_mins / domain_maxs"""
    mode = 'train'
    CP_KEYS = ('fitted_volume', 'num_networks_fitted', 'phase', 'root_nodes', 'nodes_to_process', 'saturated_nodes_to_process', 'total_volume')

    def __init__(self, cfg, pipeline, device=None, seed=0):
        self.iter_n = 0
        self.cfg = builder.ConfigDict.wrap(dict(cfg))
        if 'mode' in self.cfg: self.mode = self.cfg.mode
        self.device = torch.device(device) if device is not None else torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
        self.seed = seed
        self._init_load()
        self.pipeline = Compose(pipeline)
        self._init_examples()

    def _init_load(self):
        cfg = self.cfg
        if cfg.batch_index == 0:
            self.cp = {'fitted_volume': 0, 'num_networks_fitted': 0, 'phase': 'discovery'}
            self.global_domain_min, self.global_domain_max = get_global_domain_min_and_max(cfg)
            if 'fixed_resolution' not in cfg:
                root = Node()
                root.domain_min, root.domain_max = self.global_domain_min, self.global_domain_max
                self.cp['root_nodes'] = [root]
            else:
                mins, maxs = kilo_distill.fixed_resolution_domains(self.global_domain_min, self.global_domain_max, list(cfg.fixed_resolution))
                self.cp['root_nodes'] = []
                for lo, hi in zip(mins.tolist(), maxs.tolist()):
                    node = Node()
                    node.domain_min, node.domain_max = lo, hi
                    self.cp['root_nodes'].append(node)
            self.cp['nodes_to_process'] = deque(self.cp['root_nodes'])
            self.cp['saturated_nodes_to_process'] = deque([])
            self.cp['total_volume'] = calculate_volume(self.global_domain_min, self.global_domain_max)
        else:
            self.cp = torch.load(os.path.join(cfg.work_dir, 'checkpoint.pth'), weights_only=False)
        queue = self.cp['nodes_to_process'] if self.cp['nodes_to_process'] else self.cp['saturated_nodes_to_process']
        self.processing_saturated_nodes = not self.cp['nodes_to_process']
        self.node_batch = [queue.popleft() for _ in range(min(cfg.max_num_networks, len(queue)))]

    def _init_examples(self):
        self.domain_mins = [node.domain_min for node in self.node_batch]
        self.domain_maxs = [node.domain_max for node in self.node_batch]
        box = lambda xs: torch.tensor(np.asarray(xs, dtype=np.float32).reshape(-1, 3), dtype=torch.float32, device=self.device)
        self._mins, self._maxs = box(self.domain_mins), box(self.domain_maxs)
        self.all_examples = None
        if self.mode != 'train' and self.node_batch:              # one fixed set, generated once
            n = int(self.cfg.num_examples_per_network)
            self.all_examples = kilo_distill.distill_examples(self._mins, self._maxs, n, self.seed, 0, pool_size=n)

    def save_cp(self):
        """work_dir/checkpoint.pth: what batch_index > 0 reads"""
        os.makedirs(self.cfg.work_dir, exist_ok=True)
        path = os.path.join(self.cfg.work_dir, 'checkpoint.pth')
        torch.save(self.cp, path)
        return path

    def get_info(self):
        return {'cp': self.cp, 'processing_saturated_nodes': self.processing_saturated_nodes, 'node_batch': self.node_batch}

    def set_iter(self, iter_n):
        self.iter_n = iter_n

    def _fetch_train_data(self, idx):
        cfg = self.cfg
        batch = kilo_distill.distill_examples(self._mins, self._maxs, cfg.train_batch_size, self.seed, int(idx), pool_size=cfg.num_examples_per_network)
        return {'batch_examples': batch, 'domain_mins': self.domain_mins, 'domain_maxs': self.domain_maxs}

    def _fetch_val_data(self, idx):
        return {'batch_examples': self.all_examples, 'domain_mins': self.domain_mins, 'domain_maxs': self.domain_maxs}

    _fetch_test_data = _fetch_val_data

    def __getitem__(self, idx):
        return self.pipeline(self._fetch_train_data(idx) if self.mode == 'train' else self._fetch_val_data(idx))

    def __len__(self):
        return int(self.cfg.num_examples_per_network) // int(self.cfg.train_batch_size) if self.mode == 'train' else 1
