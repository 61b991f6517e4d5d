"""GeneBody data on the device: GeneBodyDataset and the view store behind it -- the data side of
configs/gnr/gnr_genebody.py, whose three `data` dicts name it.

Mirrors, relative to the reference's tree:
  xrnerf/datasets/genebody_dataset.py        GeneBodyDataset (constructor, get_frames, __len__, __getitem__, get_image)
  xrnerf/datasets/utils/genebody.py          load_obj_mesh, load_ply -- restated for their (vertices, faces) use only

The reference decodes, crops, resizes (cv2), normalises and masks 5 views per training item and 4 + 48 per evaluation item on the host,
2448 x 2048 pictures each, and measures the body against every camera.  Here the host lists and decodes files (PIL) and parses the
body; a view is cropped and resized ONCE on the device (xrnerf_amd/csrc/xr_genebody.hip: crop box, OpenCV's nearest and 8-bit cubic
resize) and stays there under a byte budget (ViewStore); an item whose views are resident is two launches (assemble, calib).

Deviations from the reference:
  * cv2, imageio and torchvision are not dependencies.  The two resizes and Rodrigues are restated from OpenCV's documented / remembered
    behaviour (tests/genebody_restatement.py is the specification); their equality with OpenCV itself is unverified
  * items leave __getitem__ as tensors on the dataset's device; `bbox` is a float64 tensor of 4 and `spatial_freq` a float64 scalar
    tensor there, so nothing is read back per item (GnrNetwork.prepare_data's .cpu() is the item's one read)
  * near / far / spatial_freq come from fp32 products in a fixed order, not from BLAS: equal to the reference within its own rounding
  * phase='render' and move_cam > 0 raise NotImplementedError (the reference indexes annots['K'][25] on the `cams` dict there)
  * masks must be single-channel uint8 and a crop must lie inside its picture: ValueError where the reference fails inside cv2.resize
  * of several files whose name contains the frame's, the first in sorted order is taken (the reference: the first os.listdir returns)
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import builder, ops
from .pipelines import DATASETS, Compose

_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'byte': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'long': 'i4', 'uint': 'u4', 'uint32': 'u4', 'ulong': 'u4', 'float': 'f4', 'float32': 'f4', 'single': 'f4',
              'double': 'f8', 'float64': 'f8'}


# ------------------------------------------------------------------------------------------ the body's files
def load_obj_mesh(path):
    """(vertices [N,3] float64, faces [F,3] int64, 0-based) of a Wavefront .obj: `v` and `f` lines, the index before the first '/', a face
    of more than three corners split as (1 2 3) (3 4 1) -- datasets/utils/genebody.py:238-367 without normals and textures"""
    verts, faces = [], []
    with open(path, 'r') as f:
        for line in f:
            if line.startswith('#'):
                continue
            v = line.split()
            if not v:
                continue
            if v[0] == 'v':
                verts.append([float(x) for x in v[1:4]])
            elif v[0] == 'f':
                i = [int(x.split('/')[0]) for x in v[1:]]
                faces.append(i[:3])
                if len(i) > 3:
                    faces.append([i[2], i[3], i[0]])
    return np.array(verts), np.array(faces) - 1


def load_ply(path):
    """(vertices [N,3], faces [F,k]) of a .ply: ASCII, binary_little_endian or binary_big_endian; the first three properties of `vertex`
    and the list property of `face` (datasets/utils/genebody.py:370-429 for this use)"""
    with open(path, 'rb') as f:
        raw = f.read()
    end = raw.find(b'end_header\n')
    if not raw.startswith(b'ply') or end < 0:
        raise ValueError('%s is not a PLY file' % path)
    form, elems = 'ascii', []
    for line in raw[:end].decode('ascii', 'replace').split('\n'):
        t = line.split()
        if len(t) >= 2 and t[0] == 'format':
            form = t[1].lower()
        elif len(t) >= 3 and t[0] == 'element':
            elems.append((t[1], int(t[2]), []))
        elif len(t) >= 3 and t[0] == 'property' and elems:
            elems[-1][2].append((_PLY_TYPES[t[2]], _PLY_TYPES[t[3]]) if t[1] == 'list' else _PLY_TYPES[t[1]])
    body, out = raw[end + 11:], {}
    if form == 'ascii':
        lines = body.decode('ascii').split('\n')
        at = 0
        for name, count, props in elems:
            rows = []
            for line in lines[at:at + count]:
                s, j, row = line.split(), 0, []
                for p in props:
                    if isinstance(p, tuple):
                        n = int(s[j])
                        row.append([float(x) if p[1][0] == 'f' else int(x) for x in s[j + 1:j + 1 + n]])
                        j += n + 1
                    else:
                        row.append(float(s[j]) if p[0] == 'f' else int(s[j]))
                        j += 1
                rows.append(row)
            at += count
            out[name] = (rows, props)
    else:
        e = {'binary_little_endian': '<', 'binary_big_endian': '>'}[form]
        at = 0
        for name, count, props in elems:
            if not any(isinstance(p, tuple) for p in props):
                dt = np.dtype([('p%d' % i, e + p) for i, p in enumerate(props)])
                a = np.frombuffer(body, dt, count, at)
                at += dt.itemsize * count
                out[name] = ([[a[n][i] for n in a.dtype.names] for i in range(count)], props)
                continue
            rows = []
            for _ in range(count):
                row = []
                for p in props:
                    if isinstance(p, tuple):
                        cd, ed = np.dtype(e + p[0]), np.dtype(e + p[1])
                        n = int(np.frombuffer(body, cd, 1, at)[0])
                        at += cd.itemsize
                        row.append(np.frombuffer(body, ed, n, at).tolist())
                        at += ed.itemsize * n
                    else:
                        d = np.dtype(e + p)
                        row.append(np.frombuffer(body, d, 1, at)[0].item())
                        at += d.itemsize
                rows.append(row)
            out[name] = (rows, props)
    rows, props = out['vertex']
    wide = any(p == 'f8' for p in props if not isinstance(p, tuple))
    verts = np.array([r[:3] for r in rows], dtype=np.float64 if wide else np.float32).reshape(-1, 3)
    rows, props = out['face']
    k = [i for i, p in enumerate(props) if isinstance(p, tuple)][0]
    faces = np.array([r[k] for r in rows], dtype=np.dtype(props[k][1]))
    return verts, faces.reshape(len(rows), -1)


def read_image(path):
    """a PNG / JPEG through PIL: uint8 as stored, 16-bit PNGs as uint16"""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.dtype == np.int32 and a.size and a.min() >= 0 and a.max() <= 65535:          # mode 'I': a 16-bit PNG PIL widened
        a = a.astype(np.uint16)
    return a


# ------------------------------------------------------------------------------------------ the view store
class PreparedView:
    """what a view contributes whatever its role: the resized 8-bit picture [S,S,3], the resized mask byte [S,S] (before the > 128
    threshold), the resized depth [S,S] fp32 when the view has one, the crop box (top, left, bottom, right) as 4 int32 -- on the device"""

    def __init__(self, rgb, m8, depth, box):
        self.rgb, self.m8, self.depth, self.box = rgb, m8, depth, box

    @property
    def nbytes(self):
        return self.rgb.numel() + self.m8.numel() + (self.depth.numel() * 4 if self.depth is not None else 0) + 16


class _Resident:
    def __init__(self, tensors):
        self.tensors = tensors
        self.nbytes = sum(t.numel() * t.element_size() for t in tensors)


class ViewStore:
    """prepared views keyed by (subject, frame, view) -- and a frame's body under (subject, frame, 'smpl') -- made the first time they are
    used and kept under a byte budget, oldest evicted first"""

    def __init__(self, device, S, budget=16 << 30):
        self.device, self.S, self.budget = torch.device(device), int(S), int(budget)
        self.entries = OrderedDict()
        self.prepared = 0           # views made so far (a cache hit does not count)

    def nbytes(self):
        return sum(e.nbytes for e in self.entries.values())

    def trim(self):
        while len(self.entries) > 1 and self.nbytes() > self.budget:
            self.entries.popitem(last=False)

    def resident(self, key, make):
        e = self.entries.get(key)
        if e is None:
            e = self.entries[key] = _Resident([t.to(self.device) for t in make()])
        return e.tensors

    def prepare(self, loaded):
        """loaded: [(img [h,w,3] uint8, mask [h,w] uint8, depth [h,w] uint16 or None)] on the host -> [PreparedView]: two uploads and two
        launches per XR_GB_MAX_VIEWS views, and ONE read of the crop boxes (to refuse a crop that leaves its picture)"""
        out = []
        for at in range(0, len(loaded), ops.GB_MAX_VIEWS):
            chunk = loaded[at:at + ops.GB_MAX_VIEWS]
            for img, mask, depth in chunk:
                if mask.dtype != np.uint8 or mask.ndim != 2:
                    raise ValueError('a mask must be single-channel uint8 (got %s %r)' % (mask.dtype, mask.shape))
                if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[:2] != mask.shape:
                    raise ValueError('a picture must be [h, w, 3] uint8 of its mask\'s size (got %s %r, mask %r)' % (img.dtype, img.shape, mask.shape))
                if depth is not None and (depth.dtype != np.uint16 or depth.shape != mask.shape):
                    raise ValueError('a depth map must be 16-bit of its mask\'s size (got %s %r)' % (depth.dtype, depth.shape))
            imgs, io = ops.gb_pack([c[0] for c in chunk], np.uint8, self.device)
            masks, mo = ops.gb_pack([c[1] for c in chunk], np.uint8, self.device)
            with_depth = [c[2] for c in chunk if c[2] is not None]
            depths, do = ops.gb_pack(with_depth, np.uint16, self.device) if with_depth else (None, [])
            do = iter(do)
            boxes = ops.gb_crop_box((masks, [(o, c[1].shape[0], c[1].shape[1]) for o, c in zip(mo, chunk)]))
            entries = [(i, m, next(do) if c[2] is not None else -1, c[1].shape[0], c[1].shape[1]) for i, m, c in zip(io, mo, chunk)]
            for (top, left, bottom, right), c in zip(boxes.cpu().tolist(), chunk):
                h, w = c[1].shape
                if top < 0 or left < 0 or bottom > h or right > w or bottom <= top or right <= left:
                    raise ValueError('crop (%d, %d, %d, %d) does not lie inside the %d x %d picture: its side exceeds the other dimension'
                                     % (top, left, bottom, right, h, w))
            rgb, m8, depth = ops.gb_resize(imgs, masks, depths, entries, boxes, self.S)
            for i, c in enumerate(chunk):       # every view owns its tensors, so that evicting it frees them
                out.append(PreparedView(rgb[i].clone(), m8[i].clone(), depth[i].clone() if c[2] is not None else None, boxes[i].clone()))
        self.prepared += len(out)
        return out

    def get_many(self, keys, load):
        """the views under `keys` (in order, repeats allowed); load(key) -> (img, mask, depth or None) on the host for a missing one"""
        missing = [k for k in OrderedDict.fromkeys(keys) if k not in self.entries]
        if missing:
            for k, view in zip(missing, self.prepare([load(k) for k in missing])):
                self.entries[k] = view
        views = [self.entries[k] for k in keys]
        self.trim()
        return views


# ------------------------------------------------------------------------------------------ the dataset
MISSING_VIEWS = {'wuwenyan': (34, 36), 'dannier': (32,), 'Tichinah_jervier': (32,), 'joseph_matanda': (39, 40, 42, 43, 44, 45, 46, 47)}


@DATASETS.register_module()
class GeneBodyDataset:
    """the reference's GeneBodyDataset: `opt` is the config's basedata_cfg, `phase` 'train' or an evaluation phase.  `opt.cache_bytes`
    bounds the views kept on the device (default 16 GiB)."""

    def __init__(self, opt, pipeline, phase='eval', root=None, move_cam=0, device=None):
        self.opt = opt = builder.ConfigDict.wrap(dict(opt))
        self.is_train = phase == 'train'
        self.is_render = phase == 'render'
        self.projection_mode = 'perspective'
        self.eval_skip, self.train_skip = opt.eval_skip, opt.train_skip
        self.genebody_seq_len = 150
        self.root = root if root is not None else opt.dataroot
        self.phase = 'val'
        self.load_size = opt.loadSize
        self.B_MIN, self.B_MAX = np.array([-128, -28, -128]), np.array([128, 228, 128])
        self.num_views = opt.num_views
        self.input_views = [1, 13, 25, 37]
        self.test_views = sorted(list(range(0, 48)))
        self.move_cam = move_cam if not self.is_train else 0
        if self.is_render or self.move_cam > 0:
            raise NotImplementedError('GeneBodyDataset: phase=\'render\' and move_cam > 0 are not built (the reference indexes annots[\'K\'][25] '
                                      'on the `cams` dict there)')
        self.split = np.load(os.path.join(self.root, 'genebody_split.npy'), allow_pickle=True).item()
        self.sequences = self.split['train'] if self.is_train else self.split['test']
        self.frames, self.cam_names, self.subjects, self.frames_id = self.get_frames()
        self.load_smpl_param = any([opt.use_smpl_sdf, opt.use_t_pose])
        self.load_smpl_mesh = any([opt.use_smpl_sdf, opt.use_t_pose])
        self.smpl_type = opt.smpl_type
        self.smpl_t_pose = load_obj_mesh(os.path.join(opt.t_pose_path, '%s.obj' % self.smpl_type))
        self.use_smpl_depth = opt.use_smpl_depth
        self.use_white_bkgd = opt.use_white_bkgd
        self.pipeline = Compose(pipeline)
        self.device = torch.device(device) if device is not None else torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
        self.store = ViewStore(self.device, self.load_size, opt.get('cache_bytes', 16 << 30))
        self._cams, self._cam_rows, self._dirs, self._t_pose = {}, {}, {}, None

    def get_frames(self, i=0):
        frames, subjects, cam_names, frames_id = [], [], [], []
        for seq in self.sequences:
            if os.path.exists(os.path.join(self.root, seq)):
                files = sorted(f for f in os.listdir(os.path.join(self.root, seq, 'param')) if f[-4:] == '.npy')
                cam_names += ['%02d'] * len(files)
                subjects += [seq] * len(files)
                frames_id += list(range(len(files)))
                frames += [f[:-4] for f in files]
        return frames, cam_names, subjects, frames_id

    def __len__(self):
        if self.is_train:
            return len(self.frames) * len(self.test_views) // self.train_skip
        return len(self.frames) // self.eval_skip

    # ---- the host's part
    def _find(self, folder, frame):
        names = self._dirs.get(folder)
        if names is None:
            names = self._dirs[folder] = sorted(os.listdir(folder))
        return os.path.join(folder, [f for f in names if frame in f][0])

    def cameras(self, subject):
        """per view of a subject, once: K, D, c2w and w2c = np.linalg.inv(c2w) in float32, by the reference's own expressions"""
        cams = self._cams.get(subject)
        if cams is None:
            annots = np.load(os.path.join(self.root, subject, 'annots.npy'), allow_pickle=True).item()['cams']
            cams = self._cams[subject] = {}
            for view, a in annots.items():
                c2w = np.array(a['c2w'], dtype=np.float32)
                cams[view] = {'K': np.array(a['K'], dtype=np.float32), 'D': np.array(a['D'], dtype=np.float32).reshape(-1), 'c2w': c2w,
                              'w2c': np.linalg.inv(c2w)}
        return cams

    def _camera_rows(self, subject, view_ids):
        """(K [V,3,3], D [V,nd], w2c [V,4,4]) of these views on the device, uploaded once"""
        key = (subject, tuple(view_ids))
        rows = self._cam_rows.get(key)
        if rows is None:
            cams = [self.cameras(subject)['%02d' % v] for v in view_ids]
            rows = self._cam_rows[key] = tuple(torch.from_numpy(np.ascontiguousarray(np.stack([c[k] for c in cams]))).to(self.device) for k in ('K', 'D', 'w2c'))
        return rows

    def view_ids(self, sid, view_id=None, random_sample=False):
        subject = self.subjects[sid]
        # some sequences have views missing (genebody_dataset.py:193-202; joseph_matanda's list starts from all 48, as there)
        base = range(48) if subject == 'joseph_matanda' else self.test_views
        test_views = sorted(set(base) - set(MISSING_VIEWS.get(subject, ())))
        if not self.is_train:
            return self.input_views + test_views
        if view_id is None or random_sample:
            view_id = test_views[np.random.randint(len(test_views))]
        else:
            view_id = test_views[view_id % len(test_views)]
        return self.input_views + [view_id]

    def _load_view(self, key):
        subject, frame, vid = key
        folder = lambda kind: os.path.join(self.root, subject, kind, '%02d' % vid)
        img, mask = read_image(self._find(folder('image'), frame)), read_image(self._find(folder('mask'), frame))
        depth = None
        if self.use_smpl_depth and vid in self.input_views[:self.num_views]:
            depth = read_image(self._find(folder('smpl_depth'), frame))
        return img, mask, depth

    def _load_body(self, subject, frame):
        path = self._find(os.path.join(self.root, subject, 'smpl'), frame)
        vert, face = load_obj_mesh(path) if path[-4:] == '.obj' else load_ply(path)
        return torch.from_numpy(np.ascontiguousarray(vert[:, :3].astype(np.float32))), torch.from_numpy(np.ascontiguousarray(face.astype(np.int32)))

    # ---- an item
    def get_image(self, sid, num_views, view_id=None, random_sample=False, smpl_verts=None):
        frame, subject = self.frames[sid], self.subjects[sid]
        view_ids = self.view_ids(sid, view_id, random_sample)
        views = self.store.get_many([(subject, frame, v) for v in view_ids], self._load_view)
        S = self.load_size
        depth = [v.depth for v in views[:self.num_views]] if self.use_smpl_depth else None
        img, mask, smpl_depth, acc = ops.gb_assemble([v.rgb for v in views], [v.m8 for v in views], depth, self.num_views, S, self.use_white_bkgd)
        K, D, w2c = self._camera_rows(subject, view_ids)
        c = ops.gb_calib(smpl_verts, K, D, w2c, [v.box for v in views], acc, self.num_views, S)
        empty = torch.empty(0, device=self.device)
        return {'img': img if self.is_train else img[:num_views], 'mask': mask[:num_views], 'persps': c['persps'], 'calib': w2c, 'bbox': c['bbox'],
                'render_gt': empty if self.is_train else img[num_views:], 'smpl_depth': smpl_depth if self.use_smpl_depth else empty,
                'spatial_freq': c['spatial_freq'], 'center': c['center']}

    def _fetch_train_data(self, index):
        sid = index % len(self.frames)
        vid = (index // len(self.frames)) % len(self.test_views)
        frame, subject = self.frames[sid], self.subjects[sid]
        res = {}
        param = np.load(self._find(os.path.join(self.root, subject, 'param'), frame), allow_pickle=True).item()
        scale, param = param['smplx_scale'], param['smplx']
        res['body_scale'] = scale
        param = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in param.items()}
        vert, face = self.store.resident((subject, frame, 'smpl'), lambda: self._load_body(subject, frame))
        res.update(self.get_image(sid, num_views=self.num_views, view_id=vid, random_sample=self.opt.random_multiview, smpl_verts=vert))
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        from .bodydata import rodrigues         # cv2.Rodrigues' documented formula in double (imported here: bodydata imports pipelines, which imports this module)
        T = rodrigues(np.asarray(param['global_orient']).reshape(-1, 3)[:1])
        res['smpl_rot'] = up(T, np.float32) if self.load_smpl_mesh else []
        res['smpl_verts'] = vert if self.load_smpl_mesh else []
        res['smpl_faces'] = face if self.load_smpl_mesh else []
        res['smpl_betas'] = up(np.asarray(param['betas']).reshape(-1), np.float32) if self.load_smpl_param else []
        if self.opt.use_t_pose:
            if self._t_pose is None:
                self._t_pose = (up(self.smpl_t_pose[0], np.float32), up(self.smpl_t_pose[1], np.int32))
            res['smpl_t_verts'], res['smpl_t_faces'] = self._t_pose
        else:
            res['smpl_t_verts'], res['smpl_t_faces'] = [], []
        res['idx'] = index
        return res

    def __getitem__(self, index):
        if not self.is_train:
            index *= self.eval_skip
        return self._fetch_train_data(index)
