"""ZJU-MoCap / H36M human data on the device: NeuralBodyDataset, AniNeRFDataset, the seven transforms their configs list, the frame store
and the Compose planner that runs NBGetRays .. GetPts over a prepared picture -- the data side of
configs/neuralbody/nb_zjumocap_*.py and configs/animatable_nerf/an_*.py.

Mirrors, relative to the reference's tree:
  xrnerf/datasets/neuralbody_dataset.py, aninerf_dataset.py      NeuralBodyDataset, AniNeRFDataset
  xrnerf/datasets/pipelines/create.py:308-352,660-831            NBGetRays, LoadImageAndCamera, LoadSmplParam, LoadCamAndSmplParam
  xrnerf/datasets/pipelines/augment.py:84-257                    NBSelectRays
  xrnerf/datasets/pipelines/transforms.py:90-142                 CalculateSkelTransf, AninerfIdxConversion
  xrnerf/datasets/utils/aninerf.py, novel_view.py                batch_rodrigues, get_rigid_transformation, gen_spiral_path

The reference reads, undistorts and resizes a picture, makes float64 rays for every pixel, fills six polygons, runs two argwheres and
draws in a rejection loop, on the host, for every item.  Here a picture is prepared ONCE (FrameStore: image, mask, the two candidate
lists, resident on the device under a byte budget) and an item touches the pixels it drew (xrnerf_amd/csrc/xr_bodydata.hip).  Every
transform called on its own (Compose.fuse = False, device='cpu', or no library) runs the reference's numpy arithmetic on the host.

Deviations from the reference:
  * the draws of the fused run are ONE torch.randint [8, sel_n] from a generator on the data's device seeded `seed + rank` once (the
    documented deviation of SelectRays); results['ray_draws'], when present, replaces it and is popped.  The rejection loop is bounded
    to 8 rounds: an item that is still short has a NaN tail and counts in dataset.short_items
  * cv2 is not a dependency: undistortion, resizing, the polygon fill and Rodrigues are restated from OpenCV's documented behaviour
    (host_prepare, bound_mask, rodrigues); their equality with OpenCV is unverified.  1 / ratio must be an integer
  * a projected box corner with z <= 0 or a non-finite projection raises ValueError (the reference has no defined answer there)
  * items leave __getitem__ as tensors on the dataset's device (the reference yields numpy and lets the DataLoader collate)
  * mode == 'render' runs step by step on the host: its camera is float32, so the reference's rays are fp32 arithmetic there
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import builder, ops, pipelines
from .networks import get_dist_info
from .pipelines import DATASETS, PIPELINES, Compose, GetPts, GetZvals, PerturbZvals, ToTensor

BODY_KEY = 'body_picture'            # the results key a PreparedPicture travels under
STORE_KEY = 'frame_store'
ROUNDS = ops.BODY_ROUNDS
FACES = ((0, 1, 3, 2, 0), (4, 5, 7, 6, 5), (0, 1, 5, 4, 0), (2, 3, 7, 6, 2), (0, 2, 6, 4, 0), (1, 3, 7, 5, 1))     # augment.py:126-131, verbatim


# ------------------------------------------------------------------------------------------ numpy restatements
def batch_rodrigues(poses):
    """datasets/utils/aninerf.py:4-23, the same numpy calls"""
    batch_size = poses.shape[0]
    angle = np.linalg.norm(poses + 1e-8, axis=1, keepdims=True)
    rot_dir = poses / angle
    cos = np.cos(angle)[:, None]
    sin = np.sin(angle)[:, None]
    rx, ry, rz = np.split(rot_dir, 3, axis=1)
    zeros = np.zeros([batch_size, 1])
    K = np.concatenate([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], axis=1)
    K = K.reshape([batch_size, 3, 3])
    ident = np.eye(3)[None]
    return ident + sin * K + (1 - cos) * np.matmul(K, K)


def get_rigid_transformation(poses, joints, parents, return_joints=False):
    """datasets/utils/aninerf.py:26-63, the same numpy calls"""
    rot_mats = batch_rodrigues(poses)
    rel_joints = joints.copy()
    rel_joints[1:] -= joints[parents[1:]]
    transforms_mat = np.concatenate([rot_mats, rel_joints[..., None]], axis=2)
    padding = np.zeros([24, 1, 4])
    padding[..., 3] = 1
    transforms_mat = np.concatenate([transforms_mat, padding], axis=1)
    transform_chain = [transforms_mat[0]]
    for i in range(1, parents.shape[0]):
        transform_chain.append(np.dot(transform_chain[parents[i]], transforms_mat[i]))
    transforms = np.stack(transform_chain, axis=0)
    posed_joints = transforms[:, :3, 3].copy()
    padding = np.zeros([24, 1])
    joints_homogen = np.concatenate([joints, padding], axis=1)
    rel_joints = np.sum(transforms * joints_homogen[:, None], axis=2)
    transforms[..., 3] = transforms[..., 3] - rel_joints
    transforms = transforms.astype(np.float32)
    return (transforms, posed_joints) if return_joints else transforms


def rodrigues(rvec):
    """cv2.Rodrigues(rvec)[0] by its documented formula, in double: R = cos t I + (1 - cos t) r r^T + sin t [r]x, t = |rvec|, r = rvec / t"""
    r = np.asarray(rvec, np.float64).reshape(3)
    theta = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if theta < 2.220446049250313e-16:
        return np.eye(3)
    r = r / theta
    c, s = np.cos(theta), np.sin(theta)
    rx = np.array([[0., -r[2], r[1]], [r[2], 0., -r[0]], [-r[1], r[0], 0.]])
    return c * np.eye(3) + (1. - c) * np.outer(r, r) + s * rx


def _normalize(x):
    return x / np.linalg.norm(x)


def gen_spiral_path(R, T, num_render_views, center=None):
    """datasets/utils/novel_view.py:22-69, the same numpy calls"""
    lower_row = np.array([[0., 0., 0., 1.]])
    RT = np.concatenate([np.array(R), np.array(T) / 1000.], axis=2)
    RT = np.concatenate([RT, np.tile(lower_row[None], (len(RT), 1, 1))], axis=1)
    RT[:] = np.linalg.inv(RT[:])
    RT = np.concatenate([RT[:, :, 1:2], RT[:, :, 0:1], -RT[:, :, 2:3], RT[:, :, 3:4]], 2)
    up = _normalize(RT[:, :3, 0].sum(0))
    z = _normalize(RT[0, :3, 2])
    vec1 = _normalize(np.cross(z, up))
    vec2 = _normalize(np.cross(up, vec1))
    z_off = 0
    if center is None:
        center = RT[:, :3, 3].mean(0)
        z_off = 1.3
    c2w = np.stack([up, vec1, vec2, center], 1)
    tt = np.matmul(c2w[:3, :3].T, (RT[:, :3, 3] - c2w[:3, 3])[..., np.newaxis])[..., 0].T
    rads = np.percentile(np.abs(tt), 80, -1)
    rads = rads * 1.3
    rads = np.array(list(rads) + [1.])
    render_w2c = []
    for theta in np.linspace(0., 2 * np.pi, num_render_views + 1)[:-1]:
        cam_pos = np.array([0, np.sin(theta), np.cos(theta), 1] * rads)
        cam_pos_world = np.dot(c2w[:3, :4], cam_pos)
        z = _normalize(cam_pos_world - np.dot(c2w[:3, :4], np.array([z_off, 0, 0, 1.])))
        vec2_ = _normalize(z)
        vec1_ = _normalize(np.cross(vec2_, up))
        vec0_ = _normalize(np.cross(vec1_, vec2_))
        mat = np.stack([vec0_, vec1_, vec2_, cam_pos_world], 1)
        mat = np.concatenate([mat[:, 1:2], mat[:, 0:1], -mat[:, 2:3], mat[:, 3:4]], 1)
        mat = np.concatenate([mat, lower_row], 0)
        render_w2c.append(np.linalg.inv(mat))
    return render_w2c


def host_prepare(img8, msk8, K, D, ratio, white_bkgd):
    """LoadImageAndCamera's picture work (create.py:686-711) in numpy, with the arithmetic of k_body_prepare: -> (img [H,W,3] float32,
    msk [H,W] uint8).  xrnerf_mi355_bodydata.h states every step."""
    s = ops.body_shrink(ratio)
    img8, msk8 = np.asarray(img8, np.uint8), np.asarray(msk8, np.uint8)
    Hs, Ws = img8.shape[:2]
    if Hs % s or Ws % s:
        raise ValueError('host_prepare: a %d x %d picture cannot be shrunk by %d' % (Hs, Ws, s))
    Hm, Wm = msk8.shape[:2]
    K, D = np.asarray(K, np.float64), np.asarray(D, np.float64).reshape(-1)[:5]
    src = img8.astype(np.float32) / np.float32(255)
    vv, uu = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing='ij')
    msrc = lambda y, x: msk8[(y * Hm) // Hs, (x * Wm) // Ws] != 0
    if not D.any():
        und, mund = src, msrc(vv, uu)
    else:
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        k1, k2, p1, p2, k3 = D
        x, y = (uu.astype(np.float64) - cx) / fx, (vv.astype(np.float64) - cy) / fy
        r2 = x * x + y * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * kr + p1 * (2.0 * x * y)) + p2 * (r2 + 2.0 * x * x)
        yd = (y * kr + p1 * (r2 + 2.0 * y * y)) + p2 * (2.0 * x * y)
        us, vs = fx * xd + cx, fy * yd + cy
        near = (us > -2.0) & (us < Ws + 1.0) & (vs > -2.0) & (vs < Hs + 1.0)
        us, vs = np.where(near, us, -2.0), np.where(near, vs, -2.0)
        x0, y0 = np.floor(us), np.floor(vs)
        ax, ay = (us - x0).astype(np.float32)[..., None], (vs - y0).astype(np.float32)[..., None]
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        pad = np.zeros((Hs + 4, Ws + 4, 3), np.float32)
        pad[2:-2, 2:-2] = src
        tap = lambda yy, xx: pad[yy + 2, xx + 2]
        one = np.float32(1)
        top = tap(y0, x0) * (one - ax) + tap(y0, x0 + 1) * ax
        bot = tap(y0 + 1, x0) * (one - ax) + tap(y0 + 1, x0 + 1) * ax
        und = top * (one - ay) + bot * ay
        xn, yn = np.floor(us + 0.5).astype(np.int64), np.floor(vs + 0.5).astype(np.int64)
        ok = near & (xn >= 0) & (yn >= 0) & (xn < Ws) & (yn < Hs)
        mund = ok & msrc(np.clip(yn, 0, Hs - 1), np.clip(xn, 0, Ws - 1))
    H, W = Hs // s, Ws // s
    if s == 1:
        img = und.copy()
    else:
        blocks = und.reshape(H, s, W, s, 3)
        img = None
        for dy in range(s):
            for dx in range(s):
                img = blocks[:, dy, :, dx].copy() if img is None else img + blocks[:, dy, :, dx]
        img = img / np.float32(s * s)
    msk = mund[::s, ::s].astype(np.uint8)
    img[msk == 0] = 1 if white_bkgd else 0
    return np.ascontiguousarray(img, np.float32), np.ascontiguousarray(msk)


def body_bounds(smpl_verts):
    """augment.py:231-234: fp32 min / max of the vertices -+ 0.05, [2,3]"""
    smpl_verts = np.asarray(smpl_verts)
    return np.stack([np.min(smpl_verts, axis=0) - 0.05, np.max(smpl_verts, axis=0) + 0.05], axis=0)


def box_corners_2d(bounds, K, pose):
    """get_bound_2d_mask's eight projected corners (augment.py:103-123), int [8,2] (x, y); ValueError where the reference has no answer"""
    min_x, min_y, min_z = bounds[0]
    max_x, max_y, max_z = bounds[1]
    corners_3d = np.array([[min_x, min_y, min_z], [min_x, min_y, max_z], [min_x, max_y, min_z], [min_x, max_y, max_z],
                           [max_x, min_y, min_z], [max_x, min_y, max_z], [max_x, max_y, min_z], [max_x, max_y, max_z]])
    xyz = np.dot(corners_3d, pose[:, :3].T) + pose[:, 3:].T
    xyz = np.dot(xyz, K.T)
    if not np.all(np.isfinite(xyz)) or np.any(xyz[:, 2] <= 0):
        raise ValueError('a corner of the body box projects from z <= 0 or to a non-finite position: the box silhouette is undefined')
    xy = np.round(xyz[:, :2] / xyz[:, 2:])
    if not np.all(np.isfinite(xy)) or np.abs(xy).max() > (1 << 30):
        raise ValueError('a corner of the body box projects beyond +-2^30 pixels')
    return xy.astype(int)


def bound_mask(corners_2d, H, W):
    """the six fillPoly calls of get_bound_2d_mask as exact integer arithmetic: a pixel is set when it lies on an edge of one of the six
    closed polygons or inside it by the even-odd rule (int64 cross products) -> uint8 [H,W]"""
    c = np.asarray(corners_2d, np.int64)
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing='ij')
    mask = np.zeros((H, W), bool)
    for face in FACES:
        inside, on_edge = np.zeros((H, W), bool), np.zeros((H, W), bool)
        for e in range(5):
            (ax, ay), (bx, by) = c[face[e]], c[face[0 if e == 4 else e + 1]]
            cross = (bx - ax) * (y - ay) - (x - ax) * (by - ay)
            on_edge |= (cross == 0) & (x >= min(ax, bx)) & (x <= max(ax, bx)) & (y >= min(ay, by)) & (y <= max(ay, by))
            inside ^= ((ay > y) != (by > y)) & ((cross > 0) == (by > ay))
        mask |= inside | on_edge
    return mask.astype(np.uint8)


def nb_rays(K, R, T, H, W):
    """NBGetRays' arithmetic (create.py:331-343) -> (rays_o, rays_d) [H,W,3]"""
    rays_o = -np.dot(R.T, T).ravel()
    i, j = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing='xy')
    xy1 = np.stack([i, j, np.ones_like(i)], axis=2)
    pixel_camera = np.dot(xy1, np.linalg.inv(K).T)
    pixel_world = np.dot(pixel_camera - T.ravel(), R)
    rays_d = pixel_world - rays_o[None, None]
    rays_d = rays_d / np.linalg.norm(rays_d, axis=2, keepdims=True)
    return np.broadcast_to(rays_o, rays_d.shape), rays_d


def get_near_far(bounds, ray_o, ray_d):
    """augment.py:135-150"""
    norm_d = np.linalg.norm(ray_d, axis=-1, keepdims=True)
    viewdir = ray_d / norm_d
    viewdir[(viewdir < 1e-5) & (viewdir > -1e-10)] = 1e-5
    viewdir[(viewdir > -1e-5) & (viewdir < 1e-10)] = -1e-5
    tmin = (bounds[:1] - ray_o[:1]) / viewdir
    tmax = (bounds[1:2] - ray_o[:1]) / viewdir
    t1 = np.minimum(tmin, tmax)
    t2 = np.maximum(tmin, tmax)
    near = np.max(t1, axis=-1)
    far = np.min(t2, axis=-1)
    mask_at_box = near < far
    near = near[mask_at_box] / norm_d[mask_at_box, 0]
    far = far[mask_at_box] / norm_d[mask_at_box, 0]
    return near, far, mask_at_box


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


# ------------------------------------------------------------------------------------------ the frame store
class PreparedPicture:
    """what a picture contributes to its items, resident on `device`: the prepared image [H,W,3] fp32 and mask [H,W] uint8, the camera
    (K with rows 0-1 scaled by ratio, R, T / unit, inv(K) from np.linalg.inv, rays_o = -R^T T: host doubles) and, per body box, the 30
    camera doubles and the two candidate lists"""

    def __init__(self, img, msk, K, R, T, img_path=None):
        self.img, self.msk = img, msk
        self.H, self.W = int(msk.shape[0]), int(msk.shape[1])
        self.K, self.R, self.T = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(T, np.float64).reshape(3, 1)
        self.Kinv = np.linalg.inv(self.K)
        self.rays_o = -np.dot(self.R.T, self.T).ravel()
        self.img_path = img_path
        self._cam = self._lists = None

    @property
    def device(self):
        return self.msk.device

    @property
    def nbytes(self):
        n = self.img.numel() * 4 + self.msk.numel()
        if self._lists is not None:
            n += 4 * (self._lists[1].numel() + self._lists[2].numel())
        return n

    def cam(self, bounds):
        """the XR_BODY_CAM_DOUBLES doubles of this camera and this body box, on the device"""
        key = np.asarray(bounds, np.float32).tobytes()
        if self._cam is None or self._cam[0] != key:
            row = np.concatenate([self.Kinv.reshape(9), self.R.reshape(9), self.T.reshape(3), self.rays_o, np.asarray(bounds, np.float64).reshape(6)])
            self._cam = (key, torch.from_numpy(row).to(self.device))
        return self._cam[1]

    def corners(self, bounds):
        return box_corners_2d(np.asarray(bounds), self.K, np.concatenate([self.R, self.T], axis=1))

    def lists(self, bounds):
        """(bound_list, body_list) int32 on the device, and their host lengths: made once per body box"""
        key = np.asarray(bounds, np.float32).tobytes()
        if self._lists is None or self._lists[0] != key:
            bound, body = ops.body_masks(self.msk, self.corners(bounds))
            self._lists = (key, bound, body)
        return self._lists[1], self._lists[2]


class FrameStore:
    """the prepared pictures of a split, made the first time a picture is used and kept under a byte budget, oldest evicted first"""

    def __init__(self, device, budget=16 << 30):
        self.device, self.budget = torch.device(device), int(budget)
        self.entries = OrderedDict()
        self.prepared = 0           # pictures made so far (a cache hit does not count)

    @property
    def native(self):
        return ops._on_device(torch.empty(0, device=self.device)) and ops.bodydata_kernels_available()

    def nbytes(self):
        return sum(p.nbytes for p in self.entries.values())

    def get(self, key, load):
        """load() -> (img8 [Hs,Ws,3] uint8, msk8 [Hm,Wm] uint8, K unscaled, D, R, T / unit, ratio, white_bkgd, img_path), all host"""
        pic = self.entries.get(key)
        if pic is None:
            img8, msk8, K, D, R, T, ratio, white_bkgd, img_path = load()
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(self.device)
            img, msk = ops.body_prepare(up(img8), up(msk8), K, D, ratio, white_bkgd)
            K = np.array(K, np.float64)
            K[:2] = K[:2] * ratio
            pic = self.entries[key] = PreparedPicture(img, msk, K, R, T, img_path)
            self.prepared += 1
            self.trim(keep=key)
        return pic

    def trim(self, keep=None):
        while len(self.entries) > 1 and self.nbytes() > self.budget:
            k = next(iter(self.entries))
            if k == keep:
                break
            del self.entries[k]


# ------------------------------------------------------------------------------------------ the transforms
def _read_picture(results):
    """create.py:672-693 up to the bytes: (img8, msk8, K, D, R, T / unit, ratio, white_bkgd, img_path)"""
    from PIL import Image
    data_root, ims, cams, idx, cfg = results['data_root'], results['ims'], results['cams'], results['idx'], results['cfg']
    img_path = os.path.join(data_root, ims[idx])
    cam_ind = results['cam_inds'][idx]
    K, D, R = np.array(cams['K'][cam_ind]), np.array(cams['D'][cam_ind]), np.array(cams['R'][cam_ind])
    T = np.array(cams['T'][cam_ind]) / cfg.unit
    img8 = np.array(Image.open(img_path).convert('RGB'), dtype=np.uint8)
    msk_path = os.path.join(data_root, 'mask', ims[idx])[:-4] + '.png'
    if not os.path.exists(msk_path):
        msk_path = os.path.join(data_root, 'mask_cihp', ims[idx])[:-4] + '.png'
    msk8 = np.array(Image.open(msk_path))
    if msk8.ndim == 3:
        msk8 = msk8[..., 0]
    return img8, (msk8 != 0).astype(np.uint8), K, D, R, T, cfg.ratio, cfg.white_bkgd, img_path


@PIPELINES.register_module()
class LoadImageAndCamera:
    """the picture, its mask and its camera (create.py:660-726).  With the dataset's FrameStore on the device the picture is prepared
    once by k_body_prepare and stays there (results['body_picture']); otherwise host_prepare runs on the host for this item."""

    def __init__(self, enable=True, **kwargs):
        self.enable = enable

    def __call__(self, results):
        if self.enable:
            store = results.get(STORE_KEY)
            if isinstance(store, FrameStore) and store.native:
                pic = store.get(int(results['idx']), lambda: _read_picture(results))
                results.update({'img': pic.img, 'msk': pic.msk, 'cam_K': pic.K.copy(), 'cam_R': pic.R.copy(), 'cam_T': pic.T.copy(),
                                'img_path': pic.img_path, BODY_KEY: pic})
            else:
                img8, msk8, K, D, R, T, ratio, white_bkgd, img_path = _read_picture(results)
                img, msk = host_prepare(img8, msk8, K, D, ratio, white_bkgd)
                K = K.astype(np.float64)
                K[:2] = K[:2] * ratio
                results.update({'img': img, 'msk': msk, 'cam_K': K, 'cam_R': R, 'cam_T': T, 'img_path': img_path})
        return results

    def __repr__(self):
        return '{}:load the image and camera parameter'.format(self.__class__.__name__)


def _load_smpl(data_root, cfg, smpl_idx):
    """create.py:750-760"""
    smpl_verts = np.load(os.path.join(data_root, cfg.smpl_vertices_dir, '{}.npy'.format(smpl_idx))).astype(np.float32)
    params = np.load(os.path.join(data_root, cfg.smpl_params_dir, '{}.npy'.format(smpl_idx)), allow_pickle=True).item()
    return {'smpl_verts': smpl_verts, 'smpl_R': rodrigues(params['Rh']).astype(np.float32), 'smpl_T': params['Th'].astype(np.float32),
            'smpl_pose': params['poses'].astype(np.float32)}


@PIPELINES.register_module()
class LoadSmplParam:
    def __init__(self, enable=True, **kwargs):
        self.enable = enable

    def __call__(self, results):
        if self.enable:
            cfg, img_path = results['cfg'], results['img_path']
            results.update(_load_smpl(results['data_root'], cfg, cfg.img_path_to_smpl_idx(img_path)))
            frame_idx = cfg.img_path_to_frame_idx(img_path)     # (unused in the reference as well)
            results['latent_idx'] = np.array([results['idx'] // results['num_cams']])
        return results

    def __repr__(self):
        return '{}:load the SMPL parameter'.format(self.__class__.__name__)


@PIPELINES.register_module()
class LoadCamAndSmplParam:
    def __init__(self, enable=True, **kwargs):
        self.enable = enable

    def __call__(self, results):
        if self.enable:
            cfg, idx = results['cfg'], results['idx']
            K = results['K'].astype(np.float32)
            K[:2] = K[:2] * cfg['ratio']
            RT = results['spiral_poses'][idx].astype(np.float32)
            results.update({'cam_K': K, 'cam_R': RT[:3, :3], 'cam_T': RT[:3, 3:]})
            results.update(_load_smpl(results['data_root'], cfg, cfg.frame_idx_to_smpl_idx(cfg.frame_idx)))
            results['latent_idx'] = np.array([cfg.frame_idx_to_latent_idx(cfg.frame_idx)])
        return results

    def __repr__(self):
        return '{}:load the Camera and SMPL parameters'.format(self.__class__.__name__)


@PIPELINES.register_module()
class CalculateSkelTransf:
    def __init__(self, enable=True, **kwargs):
        self.enable = enable

    def __call__(self, results):
        if self.enable:
            results['A'] = get_rigid_transformation(_host(results['smpl_pose']).reshape(-1, 3), _host(results['joints']), _host(results['parents']))
        return results

    def __repr__(self):
        return '{}:calculate the skeletal transformation'.format(self.__class__.__name__)


@PIPELINES.register_module()
class AninerfIdxConversion:
    def __init__(self, enable=True, **kwargs):
        self.enable = enable

    def __call__(self, results):
        if self.enable:
            results['bw_latent_idx'] = results['latent_idx'].copy()
            results['color_latent_idx'] = results['latent_idx'].copy()
            if results['cfg'].phase == 'novel_pose':
                results['color_latent_idx'][:] = 0
        return results

    def __repr__(self):
        return '{}:convert the aninerf index'.format(self.__class__.__name__)


def _frame_size(results):
    cfg = results['cfg']
    if cfg.mode == 'render':
        return cfg.render_H, cfg.render_W
    return tuple(results['img'].shape[:2])


@PIPELINES.register_module()
class NBGetRays:
    """float64 rays of every pixel (create.py:308-352), numpy on the host"""

    def __init__(self, enable=True, **kwargs):
        self.enable, self.kwargs = enable, kwargs

    def __call__(self, results):
        if self.enable:
            H, W = _frame_size(results)
            results['rays_o'], results['rays_d'] = nb_rays(_host(results['cam_K']), _host(results['cam_R']), _host(results['cam_T']), H, W)
        return results

    def __repr__(self):
        return "{}:get rays from pose and camera's params".format(self.__class__.__name__)


@PIPELINES.register_module()
class NBSelectRays:
    """sel_n rays that hit the body's box, half of them drawn on the body (augment.py:84-257), numpy on the host.  With
    results['ray_draws'] (int [8, sel_n], popped) the rounds take their pixels from that table as xr_body_sample does -- entry
    draws[r, j] mod the list's length, at most 8 rounds, a NaN tail when short -- instead of np.random.randint."""

    def __init__(self, enable=True, sel_n=1024, sel_all=False, sel_rgb=True, seed=0, **kwargs):
        self.enable, self.kwargs, self.sel_n, self.sel_all, self.sel_rgb, self.seed = enable, kwargs, sel_n, sel_all, sel_rgb, seed
        self._generators = {}

    get_near_far = staticmethod(get_near_far)

    @staticmethod
    def get_bound_2d_mask(bounds, K, pose, H, W):
        return bound_mask(box_corners_2d(bounds, K, pose), H, W)

    def draw(self, results, device):
        """int64 [8, sel_n] on `device`; pops results['ray_draws']"""
        draws = results.pop('ray_draws', None)
        if draws is None:
            device = torch.device(device)
            if device not in self._generators:
                self._generators[device] = torch.Generator(device=device).manual_seed(self.seed + get_dist_info()[0])
            return torch.randint(0, 1 << 62, (ROUNDS, self.sel_n), device=device, generator=self._generators[device])
        return torch.as_tensor(_host(draws)).to(device=device, dtype=torch.int64).contiguous()

    def sample_rays(self, results, bounds, bound_mask_, human_mask):
        draws = results.pop('ray_draws', None)
        draws = None if draws is None else np.asarray(_host(draws), np.int64)
        img = _host(results['img'])
        lists = {'o': [], 'd': [], 'rgb': [], 'near': [], 'far': []}
        coord_body_all, coord_all = np.argwhere(human_mask != 0), np.argwhere(bound_mask_ == 1)
        nsampled_rays, rounds = 0, 0
        while nsampled_rays < self.sel_n and (draws is None or rounds < ROUNDS):
            n_body = int((self.sel_n - nsampled_rays) * 0.5)
            n_rand = self.sel_n - nsampled_rays - n_body
            if draws is None:
                coord_body = coord_body_all[np.random.randint(0, len(coord_body_all), n_body)]
                coord = coord_all[np.random.randint(0, len(coord_all), n_rand)]
            else:
                if len(coord_body_all) == 0 or len(coord_all) == 0:
                    raise ValueError('NBSelectRays: an empty candidate list (body %d, bound %d)' % (len(coord_body_all), len(coord_all)))
                coord_body = coord_body_all[draws[rounds, :n_body] % len(coord_body_all)]
                coord = coord_all[draws[rounds, n_body:n_body + n_rand] % len(coord_all)]
            coord = np.concatenate([coord_body, coord], axis=0)
            ray_o_ = results['rays_o'][coord[:, 0], coord[:, 1]]
            ray_d_ = results['rays_d'][coord[:, 0], coord[:, 1]]
            near_, far_, mask_at_box = get_near_far(bounds, ray_o_, ray_d_)
            lists['o'].append(ray_o_[mask_at_box])
            lists['d'].append(ray_d_[mask_at_box])
            if self.sel_rgb:
                lists['rgb'].append(img[coord[:, 0], coord[:, 1]][mask_at_box])
            lists['near'].append(near_)
            lists['far'].append(far_)
            nsampled_rays += len(near_)
            rounds += 1
        short = self.sel_n - nsampled_rays
        tail = lambda x, w: np.concatenate([x, np.full((short,) + (() if w is None else (w,)), np.nan, np.float32)], 0) if short > 0 else x
        results['rays_o'] = tail(np.concatenate(lists['o']).astype(np.float32), 3)
        results['rays_d'] = tail(np.concatenate(lists['d']).astype(np.float32), 3)
        if self.sel_rgb:
            results['target_s'] = tail(np.concatenate(lists['rgb']).astype(np.float32), 3)
        results['near'] = tail(np.concatenate(lists['near']).astype(np.float32), None)[:, None]
        results['far'] = tail(np.concatenate(lists['far']).astype(np.float32), None)[:, None]
        return results

    def select_all_rays(self, results, bounds):
        results['src_shape'] = torch.tensor(results['rays_d'].shape)
        ray_o = results['rays_o'].reshape(-1, 3).astype(np.float32)
        ray_d = results['rays_d'].reshape(-1, 3).astype(np.float32)
        near, far, mask_at_box = get_near_far(bounds, ray_o, ray_d)
        results['rays_o'], results['rays_d'] = ray_o[mask_at_box].astype(np.float32), ray_d[mask_at_box].astype(np.float32)
        if self.sel_rgb:
            results['target_s'] = _host(results['img']).reshape(-1, 3).astype(np.float32)[mask_at_box]
        results['near'], results['far'] = near.astype(np.float32)[:, None], far.astype(np.float32)[:, None]
        results['mask_at_box'] = mask_at_box
        return results

    def __call__(self, results):
        if self.enable:
            bounds = body_bounds(_host(results['smpl_verts']))
            if self.sel_all:                   # (the reference fills the bound mask here too, and never reads it)
                results = self.select_all_rays(results, bounds)
            else:
                H, W = _frame_size(results)
                pose = np.concatenate([_host(results['cam_R']), _host(results['cam_T'])], axis=1)
                bmask = self.get_bound_2d_mask(bounds, _host(results['cam_K']), pose, H, W)
                results = self.sample_rays(results, bounds, bmask, _host(results['msk']) * bmask)
        return results

    def __repr__(self):
        return '{}:random select rays when training'.format(self.__class__.__name__)


# ------------------------------------------------------------------------------------------ the fused run
class BodyRun:
    """Compose's third planner: [NBGetRays, NBSelectRays, ToTensor.., GetZvals, (PerturbZvals,) (GetPts)] over a PreparedPicture.
    Train: xr_body_sample (the rounds inside one workgroup) and xr_body_points -- two launches, nothing read back (`fused_points`: one).
    Frame (sel_all): xr_body_frame_count, one read of the survivor count, xr_body_frame_write, xr_body_points."""
    fused_points = False        # which of the two variants is the default, and why

    def __init__(self, start, end, select, zvals, perturb, pts, side):
        self.start, self.end, self.select, self.zvals, self.perturb, self.pts, self.side = start, end, select, zvals, perturb, pts, side

    @staticmethod
    def plan(transforms):
        enabled = lambda t: getattr(t, 'enable', True)
        start = next((i for i, t in enumerate(transforms) if type(t) is NBGetRays and enabled(t)), None)
        if start is None:
            return None
        live = [(i, t) for i, t in enumerate(transforms) if i > start and enabled(t)]
        if not live or type(live[0][1]) is not NBSelectRays:
            return None
        select, side, zvals, perturb, pts, end = live[0][1], [], None, False, False, live[0][0]
        for i, t in live[1:]:
            if type(t) is ToTensor and not pts:
                side.append(t)
            elif type(t) is GetZvals and zvals is None:
                zvals = t
            elif type(t) is PerturbZvals and zvals is not None and not perturb and not pts:
                perturb = True
            elif type(t) is GetPts and zvals is not None and not pts:
                pts = True
            else:
                break
            end = i
        if any(type(t) in (NBGetRays, NBSelectRays) for _, t in live[1:]):
            return None
        if zvals is not None and (zvals.randomized or zvals.lindisp):
            return None
        if not select.sel_all and not select.sel_rgb:          # (the reference's sample_rays cannot run without the colours either)
            return None
        return BodyRun(start, end, select, zvals, perturb, pts, side)

    def ready(self, results):
        pic, cfg = results.get(BODY_KEY), results.get('cfg')
        return isinstance(pic, PreparedPicture) and ops._on_device(pic.msk) and ops.bodydata_kernels_available() and \
            cfg is not None and cfg.mode != 'render' and 'smpl_verts' in results

    def __call__(self, results):
        pic, sel, z = results[BODY_KEY], self.select, self.zvals
        bounds = body_bounds(_host(results['smpl_verts']))
        cam, S = pic.cam(bounds), (z.N_samples if z is not None else 0)
        if sel.sel_all:
            out = ops.body_frame(cam, pic.H, pic.W, pic.img if sel.sel_rgb else None)
            results['src_shape'] = torch.tensor((pic.H, pic.W, 3))
            if S:
                t_rand = self._t_rand(results, out['rays_o'].shape[0], S, pic.device)
                out.update(ops.body_points(out['rays_o'], out['rays_d'], out['near'], out['far'], S, t_rand))
        else:
            bound, body = pic.lists(bounds)
            if bound.numel() == 0 or body.numel() == 0:
                raise ValueError('NBSelectRays: an empty candidate list (body %d, bound %d) in %s' % (body.numel(), bound.numel(), pic.img_path))
            draws = sel.draw(results, pic.device)
            out = ops.body_sample(cam, pic.H, pic.W, pic.img, body, bound, draws, results['short_items'], S=S,
                                  t_rand=self._t_rand(results, draws.shape[1], S, pic.device), fused_points=self.fused_points)
        if not self.pts:
            out.pop('pts', None)
        results.update(out)
        for t in self.side:
            for k in t.keys:
                if k in results:
                    results[k] = pipelines.to_tensor(results[k])
        return results

    def _t_rand(self, results, n, S, device):
        if not self.perturb or not S:
            return None
        t_rand = results.pop('t_rand', None)
        return torch.rand((n, S), device=device) if t_rand is None else t_rand.to(device)


# ------------------------------------------------------------------------------------------ the datasets
@DATASETS.register_module()
class NeuralBodyDataset:
    """the reference's NeuralBodyDataset (neuralbody_dataset.py): view / frame selection from annots.npy, one picture per item.  On the
    device its pictures live in a FrameStore (cfg.cache_bytes, default 16 GiB); `short_items` counts the training items whose eight
    rounds did not fill sel_n (a device counter: read it when you want to know, nothing reads it on the hot path)."""

    def __init__(self, cfg, pipeline, device=None, seed=0):
        self.cfg = builder.ConfigDict.wrap(dict(cfg))
        cfg = self.cfg
        self.is_train = cfg.mode == 'train'
        self.data_root, self.ratio, self.white_bkgd = cfg.datadir, cfg.ratio, cfg.white_bkgd
        self.smpl_vertices_dir, self.smpl_params_dir = cfg.smpl_vertices_dir, cfg.smpl_params_dir
        self.img_path_to_smpl_idx, self.img_path_to_frame_idx = cfg.img_path_to_smpl_idx, cfg.img_path_to_frame_idx
        self.iter_n, self.seed = 0, seed
        self.device = torch.device(device) if device is not None else torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
        ops.body_shrink(cfg.ratio)
        self.store = FrameStore(self.device, cfg.get('cache_bytes', 16 << 30))
        self._short = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._init_load()
        self.pipeline = Compose(pipeline)
        for t in self.pipeline.transforms:
            if isinstance(t, NBSelectRays):
                t.seed = seed

    @property
    def short_items(self):
        """training items so far that ran short after eight rounds (one blocking read)"""
        return int(self._short.item())

    def _init_load(self):
        cfg = self.cfg
        annots = np.load(os.path.join(cfg.datadir, 'annots.npy'), allow_pickle=True).item()
        self.cams = annots['cams']
        self.spiral_poses = gen_spiral_path(self.cams['R'], self.cams['T'], cfg.get('num_render_views', 50))
        num_cams = len(self.cams['K'])
        test_view = [i for i in range(num_cams) if i not in cfg.training_view] if len(cfg.test_view) == 0 else cfg.test_view
        view = cfg.training_view if cfg.mode == 'train' else test_view
        if len(view) == 0:
            view = [0]
        view = list(view)
        begin_frame, end_frame = cfg.training_frame
        frame_interval = cfg.frame_interval
        if cfg.get('phase', 'train_pose') == 'novel_pose':
            begin_frame, end_frame = cfg.novel_pose_frame
        if cfg.mode != 'train':
            frame_interval = cfg.get('val_frame_interval', 1)
        frames = annots['ims'][begin_frame:end_frame][::frame_interval]
        self.ims = np.array([np.array(ims_data['ims'])[view] for ims_data in frames]).ravel()
        self.cam_inds = np.array([np.arange(len(ims_data['ims']))[view] for ims_data in frames]).ravel()
        self.num_cams = len(view)

    def _fetch_train_data(self, idx):
        if self.cfg.mode == 'render':
            return {'data_root': self.data_root, 'idx': idx, 'K': np.array(self.cams['K'][0]), 'spiral_poses': self.spiral_poses, 'cfg': self.cfg}
        return {'data_root': self.data_root, 'idx': idx, 'cams': self.cams, 'cam_inds': self.cam_inds, 'ims': self.ims, 'cfg': self.cfg,
                'num_cams': self.num_cams}

    def set_iter(self, iter_n):
        self.iter_n = iter_n

    def __getitem__(self, idx):
        if self.cfg.mode == 'val' or self.cfg.mode == 'test':
            idx = 0
        datas = self._fetch_train_data(idx)
        datas['iter_n'] = self.iter_n
        datas[STORE_KEY], datas['short_items'] = self.store, self._short
        datas = self.pipeline(datas)
        if datas is None:
            return None
        for k in (STORE_KEY, 'short_items', BODY_KEY, 'img', 'msk'):
            datas.pop(k, None)
        for k, v in list(datas.items()):          # items leave as tensors on the dataset's device
            if isinstance(v, np.ndarray) and v.dtype != object:
                v = torch.from_numpy(np.ascontiguousarray(v))
            if isinstance(v, torch.Tensor):
                datas[k] = v.to(self.device)
        return datas

    def __len__(self):
        return len(self.spiral_poses) if self.cfg.mode == 'render' else len(self.ims)


@DATASETS.register_module()
class AniNeRFDataset(NeuralBodyDataset):
    """the reference's AniNeRFDataset (aninerf_dataset.py): NeuralBodyDataset plus lbs/{joints, parents, weights, bigpose_vertices}.npy and
    the big pose's transforms"""

    def _init_load(self):
        super()._init_load()
        self.lbs_root = os.path.join(self.data_root, 'lbs')
        self.joints = np.load(os.path.join(self.lbs_root, 'joints.npy')).astype(np.float32)
        self.parents = np.load(os.path.join(self.lbs_root, 'parents.npy'))
        self.weights = np.load(os.path.join(self.lbs_root, 'weights.npy')).astype(np.float32)
        self.canonical_smpl_verts = np.load(os.path.join(self.lbs_root, 'bigpose_vertices.npy')).astype(np.float32)
        self.big_A = self.load_bigpose()

    def load_bigpose(self):
        big_poses = np.zeros([len(self.joints), 3]).astype(np.float32).ravel()
        angle = 30
        big_poses[5] = np.deg2rad(angle)
        big_poses[8] = np.deg2rad(-angle)
        template_pose_path = os.path.join(self.lbs_root, 'template_pose.npy')
        if os.path.exists(template_pose_path):
            big_poses = np.load(template_pose_path)
        return get_rigid_transformation(big_poses.reshape(-1, 3), self.joints, self.parents).astype(np.float32)

    def _fetch_train_data(self, idx):
        datas = super()._fetch_train_data(idx)
        datas.update({'big_A': self.big_A, 'canonical_smpl_verts': self.canonical_smpl_verts, 'smpl_bw': self.weights, 'joints': self.joints,
                      'parents': self.parents})
        return datas
