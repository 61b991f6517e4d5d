"""The bodies of the GeneBody data tests (xrnerf_amd/genebody.py over xrnerf_amd/csrc/xr_genebody.hip), shared by the three tiers:
tests/test_genebody_host.py (no GPU), tests/test_emu_genebody.py (the host build of the kernels) and tests/test_gpu_genebody.py (the
MI355X).  Also the layout of the generated GeneBody tree the fixture tests/golden/ref_genebody.npz records
(tests/golden/make_golden_genebody.py generates its arrays and runs the reference's own GeneBodyDataset on it); `write_tree` rebuilds the
tree from the npz with PIL, `coverage` asserts that the fixture still holds every case it was made for."""
import os
import struct

import numpy as np
import torch

import genebody_restatement as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'ref_genebody.npz')
SUBJECTS = {'dannier': ('0001', '0002'), 'amanda': ('0005',)}       # 'dannier' is on the reference's missing-view lists
N_CAM, INPUT_VIEWS, NUM_VIEWS = 6, [1, 4], 2
S_MAIN, S_ALT = 16, 20
OPT = dict(dataset_type='blender', eval_skip=1, train_skip=1, loadSize=S_MAIN, num_views=NUM_VIEWS, use_smpl_sdf=True, use_t_pose=True, smpl_type='smplx',
           use_smpl_depth=True, use_white_bkgd=False, random_multiview=False)
ITEM_KEYS = ('body_scale', 'img', 'mask', 'persps', 'calib', 'bbox', 'render_gt', 'smpl_depth', 'spatial_freq', 'center', 'smpl_rot', 'smpl_verts',
             'smpl_faces', 'smpl_betas', 'smpl_t_verts', 'smpl_t_faces', 'idx')       # the reference's own order
BIT_KEYS = ('img', 'mask', 'calib', 'bbox', 'render_gt', 'smpl_depth', 'center', 'smpl_rot', 'smpl_verts', 'smpl_faces', 'smpl_betas', 'smpl_t_verts',
            'smpl_t_faces')
# recorded items: name -> (phase, loadSize, white, eval_skip / train_skip, index, random_multiview)
ITEMS = {'val0': ('val', S_MAIN, False, 1, 0, False), 'val1': ('val', S_MAIN, False, 1, 1, False), 'val2': ('val', S_MAIN, False, 1, 2, False),
         'val2_s20': ('val', S_ALT, False, 1, 2, False), 'val_skip2': ('val', S_MAIN, False, 2, 1, False), 'test0_white': ('test', S_MAIN, True, 1, 0, False),
         'train0': ('train', S_MAIN, False, 1, 0, False), 'train4': ('train', S_MAIN, False, 1, 4, False), 'train11': ('train', S_MAIN, False, 1, 11, False),
         'train17_white': ('train', S_MAIN, True, 1, 17, False), 'train_skip2': ('train', S_MAIN, False, 2, 5, False),
         'train_random': ('train', S_MAIN, False, 1, 7, True)}
RANDOM_SEED = 77
_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(GOLD, allow_pickle=False))
    return _gold


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    assert a.shape == b.shape and a.dtype == b.dtype, '%s: %r %s against %r %s' % (what, a.shape, a.dtype, b.shape, b.dtype)
    eq = (a.view(np.uint8) == b.view(np.uint8))
    assert eq.all(), '%s: the bits differ in %d of %d bytes' % (what, int((~eq).sum()), eq.size)


# ------------------------------------------------------------------------------------------ the tree
def views(g=None):
    """[(subject, frame, view)] of the fixture, in a fixed order"""
    return [(s, f, v) for s, frames in SUBJECTS.items() for f in frames for v in range(N_CAM)]


def vkey(s, f, v, what):
    return 'tree.%s.%s.%02d.%s' % (s, f, v, what)


def write_obj(path, verts, faces, quad=None):
    with open(path, 'w') as f:
        f.write('# generated\n')
        for v in verts:
            f.write('v %r %r %r\n' % tuple(float(x) for x in v))
        if quad is not None:
            f.write('f %d/1/1 %d/2/2 %d/3/3 %d/4/4\n' % tuple(int(i) + 1 for i in quad))
        for t in faces:
            f.write('f %d %d %d\n' % tuple(int(i) + 1 for i in t))


def write_ply(path, verts, faces, form='binary_little_endian'):
    head = 'ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n' % (
        form, len(verts), len(faces))
    with open(path, 'wb') as f:
        f.write(head.encode('ascii'))
        if form == 'ascii':
            for v in verts:
                f.write(('%r %r %r\n' % tuple(float(x) for x in v)).encode('ascii'))
            for t in faces:
                f.write(('3 %d %d %d\n' % tuple(int(i) for i in t)).encode('ascii'))
        else:
            e = '<' if form == 'binary_little_endian' else '>'
            for v in verts:
                f.write(struct.pack(e + 'fff', *[float(x) for x in v]))
            for t in faces:
                f.write(struct.pack(e + 'Biii', 3, *[int(i) for i in t]))


def write_tree(root, g=None):
    """the GeneBody tree of the fixture under `root` (data in root/data, the T-pose body in root/t_pose) -> the `opt` dict for it"""
    from PIL import Image
    g = g or gold()
    data, tpose = os.path.join(root, 'data'), os.path.join(root, 't_pose')
    os.makedirs(tpose, exist_ok=True)
    write_obj(os.path.join(tpose, 'smplx.obj'), g['tree.t_pose.verts'], g['tree.t_pose.faces'])
    os.makedirs(data, exist_ok=True)
    np.save(os.path.join(data, 'genebody_split.npy'), {'train': list(SUBJECTS), 'test': list(SUBJECTS) + ['absent']}, allow_pickle=True)
    for s, frames in SUBJECTS.items():
        for d in ('param', 'smpl'):
            os.makedirs(os.path.join(data, s, d), exist_ok=True)
        cams = {'%02d' % v: {'K': g['tree.%s.K' % s][v], 'D': g['tree.%s.D' % s][v], 'c2w': g['tree.%s.c2w' % s][v]} for v in range(N_CAM)}
        np.save(os.path.join(data, s, 'annots.npy'), {'cams': cams}, allow_pickle=True)
        for f in frames:
            p = 'tree.%s.%s.' % (s, f)
            np.save(os.path.join(data, s, 'param', f + '.npy'), {'smplx_scale': float(g[p + 'scale']), 'smplx': {'global_orient': g[p + 'orient'], 'betas': g[p + 'betas']}},
                    allow_pickle=True)
            if s == 'dannier':
                write_obj(os.path.join(data, s, 'smpl', f + '.obj'), g[p + 'verts'], g[p + 'faces'][2:], quad=g[p + 'quad'])
            else:
                write_ply(os.path.join(data, s, 'smpl', f + '.ply'), g[p + 'verts'], g[p + 'faces'])
            for v in range(N_CAM):
                for kind in ('image', 'mask', 'smpl_depth'):
                    k = vkey(s, f, v, kind)
                    if k in g:
                        os.makedirs(os.path.join(data, s, kind, '%02d' % v), exist_ok=True)
                        Image.fromarray(g[k]).save(os.path.join(data, s, kind, '%02d' % v, f + '.png'))
    return dict(OPT, dataroot=data, t_pose_path=tpose)


def crop_branch(mask):
    """('x' | 'y', 'low' | 'high' | 'mid') of image_cropping's square-up on this mask, or None for an empty one"""
    h, w = mask.shape
    rows, cols = np.nonzero(mask)
    if len(rows) == 0:
        return None
    top, left, bottom, right = int(rows.min()), int(cols.min()), int(rows.max()), int(cols.max())
    bh = bottom - top
    bottom, top = min(int(bh * 0.1 + bottom), h), max(int(top - bh * 0.1), 0)
    right, left = min(int((right - left) * 0.1 + right), w), max(int(left - bh * 0.1), 0)
    bh, bw = bottom - top, right - left
    c, size, lim, ax = ((left + right) / 2, bh, w, 'x') if bh >= bw else ((top + bottom) / 2, bw, h, 'y')
    return ax, 'low' if c - size / 2 < 0 else ('high' if c + size / 2 >= lim else 'mid')


def coverage(g=None):
    """the cases the fixture was made for, asserted on the fixture itself"""
    g = g or gold()
    branches, sides, shapes, values, empty, tall, wide, depth_case = set(), set(), set(), set(), 0, 0, 0, 0
    for s, f, v in views():
        m = g[vkey(s, f, v, 'mask')]
        assert m.dtype == np.uint8 and m.ndim == 2
        shapes.add(m.shape)
        values |= set(np.unique(m).tolist())
        t, l, b, r = RS.crop_box(m)
        RS.check_box((t, l, b, r), *m.shape)
        br = crop_branch(m)
        if br is None:
            empty += 1
            assert b - t != r - l and not (RS.resize_nearest(m, S_MAIN) > 128).any()
            continue
        branches.add(br)
        sides.add(b - t)
        rows, cols = np.nonzero(m)
        tall += (rows.max() - rows.min()) > (cols.max() - cols.min())
        wide += (rows.max() - rows.min()) < (cols.max() - cols.min())
        k = vkey(s, f, v, 'smpl_depth')
        if k in g:
            assert g[k].dtype == np.uint16
            depth_case += bool(((g[k] == 0) & (m > 128)).any() and ((g[k] > 0) & (m == 0)).any())
    assert branches == {(a, b) for a in 'xy' for b in ('low', 'high', 'mid')}, branches
    assert {7, 16, 37, 20} <= sides, sides
    assert shapes == {(48, 40), (40, 48)} and {0, 128, 129, 255} <= values and empty >= 1 and tall and wide and depth_case, (shapes, values, empty, depth_case)
    assert any(s in ('wuwenyan', 'dannier', 'Tichinah_jervier', 'joseph_matanda') for s in SUBJECTS)


# ------------------------------------------------------------------------------------------ the kernels against the specification
def view_arrays(s, f, v, g=None):
    g = g or gold()
    return g[vkey(s, f, v, 'image')], g[vkey(s, f, v, 'mask')], g.get(vkey(s, f, v, 'smpl_depth'))


def OPS():
    from xrnerf_amd import ops
    return ops


def prepare_all(dev, S, which=None):
    """every fixture view through crop_box + resize in ONE launch each -> (list of keys, boxes, rgb, m8, depth, has_depth)"""
    ops = OPS()
    keys = which or views()
    arrs = [view_arrays(*k) for k in keys]
    imgs, io = ops.gb_pack([a[0] for a in arrs], np.uint8, dev)
    masks, mo = ops.gb_pack([a[1] for a in arrs], np.uint8, dev)
    wd = [a[2] for a in arrs if a[2] is not None]
    depths, do = ops.gb_pack(wd, np.uint16, dev)
    do = iter(do)
    boxes = ops.gb_crop_box((masks, [(o, a[1].shape[0], a[1].shape[1]) for o, a in zip(mo, arrs)]))
    entries = [(i, m, next(do) if a[2] is not None else -1, a[1].shape[0], a[1].shape[1]) for i, m, a in zip(io, mo, arrs)]
    rgb, m8, depth = ops.gb_resize(imgs, masks, depths, entries, boxes, S)
    return keys, arrs, boxes, rgb, m8, depth


def check_crop_box(dev):
    """the fixture's masks, and generated masks of odd sizes (the byte path) and of sizes that are multiples of 8 (the 8-byte path)"""
    ops = OPS()
    keys, arrs, boxes, _, _, _ = prepare_all(dev, S_MAIN)
    want = np.array([RS.crop_box(a[1]) for a in arrs], np.int32)
    same_bits(boxes, want, 'crop boxes of the fixture')
    rng = np.random.default_rng(5)
    masks = []
    for h, w in ((13, 21), (16, 24), (1, 1), (9, 8), (300, 7), (31, 64)):
        for fill in (0.0, 0.02, 0.5):
            m = (rng.uniform(0, 1, (h, w)) < fill).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)
            masks.append(m)
    one = np.zeros((40, 48), np.uint8)
    one[17, 47] = 1                                                             # a single pixel in the last byte of a word
    masks.append(one)
    got = ops.gb_crop_box(masks, dev)
    same_bits(got, np.array([RS.crop_box(m) for m in masks], np.int32), 'crop boxes of generated masks')
    same_bits(ops.gb_crop_box(masks, dev), got, 'crop boxes, second run')


def check_resize(dev):
    for S in (S_MAIN, S_ALT):
        keys, arrs, boxes, rgb, m8, depth = prepare_all(dev, S)
        n_depth = 0
        for i, (k, a) in enumerate(zip(keys, arrs)):
            w_rgb, w_m8, w_depth, _ = RS.prepare_view(a[0], a[1], a[2], S)
            same_bits(rgb[i], w_rgb, 'cubic picture of %r at %d' % (k, S))
            same_bits(m8[i], w_m8, 'nearest mask of %r at %d' % (k, S))
            if w_depth is not None:
                same_bits(depth[i], w_depth, 'nearest depth of %r at %d' % (k, S))
                n_depth += 1
        assert n_depth == 6
        keys2, _, _, rgb2, m82, depth2 = prepare_all(dev, S)
        same_bits(rgb2, rgb, 'resize, second run')
        same_bits(depth2, depth, 'resize depth, second run')
    # a box that leaves its picture is clipped: nothing is read outside (the dataset refuses it before it gets here)
    ops = OPS()
    img, mask = arrs[0][0], arrs[0][1]
    imgs, _ = ops.gb_pack([img], np.uint8, dev)
    masks, _ = ops.gb_pack([mask], np.uint8, dev)
    for bad in ((-5, -3, 60, 70), (10, 10, 10, 30)):
        box = torch.tensor([bad], dtype=torch.int32).to(dev)
        rgb, m8, _ = ops.gb_resize(imgs, masks, None, [(0, 0, -1, mask.shape[0], mask.shape[1])], box, 8)
        t, l, b, r = max(bad[0], 0), max(bad[1], 0), min(bad[2], mask.shape[0]), min(bad[3], mask.shape[1])
        want = RS.resize_cubic_u8(img[t:b, l:r], 8) if b > t and r > l else np.zeros((8, 8, 3), np.uint8)
        same_bits(rgb[0], want, 'clipped box %r' % (bad,))


def item_views(name):
    """(subject, frame, view ids, S, white, is_train) of a recorded item, from the recorded view ids"""
    g = gold()
    phase, S, white, skip, index, rnd = ITEMS[name]
    s, f = str(g['item.%s.subject' % name]), str(g['item.%s.frame' % name])
    return s, f, [int(v) for v in g['item.%s.view_ids' % name]], S, white, phase == 'train'


def spec_item(name):
    """the restatement's item from the tree's arrays"""
    g = gold()
    s, f, vids, S, white, is_train = item_views(name)
    verts = g['tree.%s.%s.verts' % (s, f)].astype(np.float32)
    out = {'img': [], 'mask': [], 'depth': [], 'vboxes': [], 'persps': [], 'sf': [], 'near_bound': [], 'rel': []}
    for i, v in enumerate(vids):
        img, mask, d16 = view_arrays(s, f, v)
        rgb, m8, depth, box = RS.prepare_view(img, mask, d16 if i < NUM_VIEWS else None, S)
        x, mf, vb = RS.assemble_view(rgb, m8, depth, i < NUM_VIEWS, white)
        out['img'].append(x)
        out['vboxes'].append(vb)
        if i < NUM_VIEWS:
            out['mask'].append(mf[None])
            out['depth'].append(depth)
        K = RS.adjusted_K(g['tree.%s.K' % s][v], box, S)
        w2c = np.linalg.inv(np.array(g['tree.%s.c2w' % s][v], dtype=np.float32))
        near, far, bound = RS.near_far64(verts, w2c)
        out['persps'].append(np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.array(g['tree.%s.D' % s][v], np.float32).reshape(-1), [near, far]]))
        out['near_bound'].append(bound)
        if i < NUM_VIEWS:
            sf, rel = RS.spatial_freq64(verts, vb, w2c, K)
            out['sf'].append(sf)
            out['rel'].append(rel)
    out['bbox'] = RS.item_bbox(out['vboxes'][NUM_VIEWS:], S)
    out['center'] = RS.center(verts)
    return out


def check_scalars(got_persps, got_sf, name, spec, what):
    """near / far within 4 x 2^-24 x (sum |a b| + |t|), the largest over the vertices' z, of the float64 restatement; spatial_freq within
    1e-5 relative of it and of the recorded reference value"""
    g = gold()
    want = np.stack(spec['persps'])
    got = host(got_persps).astype(np.float64)
    nd = want.shape[1] - 6
    same_bits(host(got_persps)[:, :4 + nd], want[:, :4 + nd].astype(np.float32), '%s: K entries and D of %s' % (what, name))
    for i in range(want.shape[0]):
        for j in (4 + nd, 5 + nd):
            err, bound = abs(got[i, j] - want[i, j]), spec['near_bound'][i]
            print('%s %s view %d %s: |got - float64| %.3e, bound %.3e' % (what, name, i, 'near' if j == 4 + nd else 'far', err, bound))
            assert err <= bound, (what, name, i, j, err, bound)
    assert min(spec['rel']) >= 0.25, 'the fixture\'s extents must be at least a quarter of the coordinates (got %r)' % (spec['rel'],)
    sf = float(host(got_sf))
    print('%s %s spatial_freq: relative to float64 %.3e, to the reference %.3e' % (what, name, abs(sf / min(spec['sf']) - 1), abs(sf / float(g['item.%s.spatial_freq' % name]) - 1)))
    assert abs(sf / min(spec['sf']) - 1) <= 1e-5 and abs(sf / float(g['item.%s.spatial_freq' % name]) - 1) <= 1e-5


def run_item(dev, name):
    """a recorded item through assemble + calib from freshly prepared views -> (spec, img, mask, smpl_depth, calib dict)"""
    ops, g = OPS(), gold()
    s, f, vids, S, white, is_train = item_views(name)
    uniq = list(dict.fromkeys(vids))
    keys, arrs, boxes, rgb, m8, depth = prepare_all(dev, S, [(s, f, v) for v in uniq])
    at = [uniq.index(v) for v in vids]
    img, mask, smpl_depth, acc = ops.gb_assemble([rgb[i] for i in at], [m8[i] for i in at], [depth[i] for i in at[:NUM_VIEWS]], NUM_VIEWS, S, white)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    K, D = up(np.stack([g['tree.%s.K' % s][v] for v in vids])), up(np.stack([g['tree.%s.D' % s][v] for v in vids]).reshape(len(vids), -1))
    w2c = up(np.stack([np.linalg.inv(np.array(g['tree.%s.c2w' % s][v], dtype=np.float32)) for v in vids]))
    c = ops.gb_calib(up(g['tree.%s.%s.verts' % (s, f)]), K, D, w2c, [boxes[i] for i in at], acc, NUM_VIEWS, S)
    return img, mask, smpl_depth, c, w2c


def check_assemble_and_calib(dev, names=('val0', 'val2_s20', 'test0_white', 'train4', 'train17_white')):
    g = gold()
    for name in names:
        spec = spec_item(name)
        img, mask, smpl_depth, c, w2c = run_item(dev, name)
        same_bits(img, np.stack(spec['img']), 'img of ' + name)
        same_bits(mask, np.stack(spec['mask']), 'mask of ' + name)
        same_bits(smpl_depth, np.stack(spec['depth']), 'smpl_depth of ' + name)
        same_bits(c['vboxes'], np.array(spec['vboxes'], np.int32).reshape(-1, 4), 'mask boxes of ' + name)
        same_bits(c['bbox'], spec['bbox'], 'bbox of ' + name)
        same_bits(c['center'], spec['center'], 'center of ' + name)
        same_bits(w2c, g['item.%s.calib' % name], 'calib of ' + name)
        check_scalars(c['persps'], c['spatial_freq'], name, spec, 'kernels')
        assert float(host(c['sf_views']).min()) == float(host(c['spatial_freq']))
        img2, mask2, depth2, c2, _ = run_item(dev, name)                                   # run to run: identical bits, the scalars included
        for a, b, what in ((img, img2, 'img'), (mask, mask2, 'mask'), (c['persps'], c2['persps'], 'persps'), (c['spatial_freq'], c2['spatial_freq'], 'spatial_freq'),
                           (c['bbox'], c2['bbox'], 'bbox'), (c['vboxes'], c2['vboxes'], 'vboxes')):
            same_bits(a, b, '%s of %s, second run' % (what, name))


# ------------------------------------------------------------------------------------------ the dataset against the recorded reference items
def build(root, name, dev=None, **extra):
    """the dataset a recorded item came from, through build_dataset, with the fixture's views patched on the instance"""
    from xrnerf_amd.pipelines import build_dataset
    phase, S, white, skip, index, rnd = ITEMS[name]
    opt = dict(write_tree(root), loadSize=S, use_white_bkgd=white, random_multiview=rnd, **extra)
    opt['train_skip' if phase == 'train' else 'eval_skip'] = skip
    if phase != 'train':
        opt['mode'] = 'val'
    ds = build_dataset(dict(type='GeneBodyDataset', opt=opt, phase=phase, pipeline=[]), dict(device=dev) if dev is not None else None)
    ds.input_views, ds.test_views = list(INPUT_VIEWS), list(range(N_CAM))
    return ds, index


def check_item(item, name, dev, what='dataset'):
    g = gold()
    assert tuple(item.keys()) == ITEM_KEYS, item.keys()
    for k in BIT_KEYS:
        want = g['item.%s.%s' % (name, k)]
        got = item[k]
        assert isinstance(got, torch.Tensor) and got.device.type == torch.device(dev).type, (k, type(got))
        same_bits(got, want, '%s: %s of %s' % (what, k, name))
    assert item['bbox'].dtype == torch.float64 and item['spatial_freq'].dtype == torch.float64 and item['spatial_freq'].dim() == 0
    assert item['idx'] == int(g['item.%s.idx' % name]) and float(item['body_scale']) == float(g['item.%s.body_scale' % name])
    spec = spec_item(name)
    want = g['item.%s.persps' % name]
    nd = want.shape[1] - 6
    same_bits(host(item['persps'])[:, :4 + nd], want[:, :4 + nd], '%s: K entries and D of %s (reference)' % (what, name))
    check_scalars(item['persps'], item['spatial_freq'], name, spec, what)
    ref = want.astype(np.float64)
    for i in range(ref.shape[0]):                   # and the recorded reference: its own fp32 evaluation lies within the same bound of float64,
        for j in (4 + nd, 5 + nd):                  # so the two fp32 evaluations are within twice the bound of each other
            assert abs(float(host(item['persps'])[i, j]) - ref[i, j]) <= 2 * spec['near_bound'][i], (name, i, j)


def check_dataset(dev, root, names=('val0', 'val1', 'val2', 'val2_s20', 'val_skip2', 'test0_white', 'train0', 'train4', 'train11', 'train17_white', 'train_skip2',
                                    'train_random')):
    """items equal to the recorded reference items; a second pass (every view resident) and a pass under a budget of one view (every
    view evicted) give the same bits"""
    made = {}
    for name in names:
        ds, index = build(root, name, dev)
        if ITEMS[name][5]:
            np.random.seed(RANDOM_SEED)
        item = ds[index]
        check_item(item, name, dev)
        made[name] = (ds, index, item)
    for name in ('val0', 'train4'):
        ds, index, first = made[name]
        n = ds.store.prepared
        again = ds[index]
        assert ds.store.prepared == n, 'a second pass prepared views again'
        small, _ = build(root, name, dev, cache_bytes=ITEMS[name][1] ** 2 * 4 + 16)      # one view without depth: all but the newest entry leave
        tight = small[index]
        tight2 = small[index]
        assert len(small.store.entries) == 1 and small.store.prepared == 2 * len(set(item_views(name)[2])) - 1
        for k in BIT_KEYS + ('persps', 'spatial_freq'):
            same_bits(again[k], first[k], 'second pass: %s of %s' % (k, name))
            same_bits(tight[k], first[k], 'budget of one view: %s of %s' % (k, name))
            same_bits(tight2[k], first[k], 'budget of one view, second pass: %s of %s' % (k, name))
    return made


def check_store_chunks(dev):
    """more views than one launch takes (XR_GB_MAX_VIEWS): the store prepares them in chunks, every view as the specification has it"""
    from xrnerf_amd import genebody
    ops = OPS()
    rng = np.random.default_rng(9)
    loaded = []
    for i in range(ops.GB_MAX_VIEWS + 6):
        h, w = (12, 9) if i % 2 else (8, 16)
        m = np.zeros((h, w), np.uint8)
        r0, c0 = rng.integers(0, h - 3), rng.integers(0, w - 3)
        m[r0:r0 + 3, c0:c0 + 3] = 255
        loaded.append((rng.integers(0, 256, (h, w, 3)).astype(np.uint8), m, rng.integers(0, 3000, (h, w)).astype(np.uint16) if i % 3 == 0 else None))
    store = genebody.ViewStore(dev, 5)
    views_ = store.prepare(loaded)
    assert len(views_) == len(loaded) and store.prepared == len(loaded)
    for v, (img, m, d) in zip(views_, loaded):
        rgb, m8, depth, box = RS.prepare_view(img, m, d, 5)
        same_bits(v.rgb, rgb, 'chunked picture')
        same_bits(v.m8, m8, 'chunked mask')
        same_bits(v.box, np.array(box, np.int32), 'chunked box')
        assert (v.depth is None) == (d is None)
        if d is not None:
            same_bits(v.depth, depth, 'chunked depth')


def check_lengths(root, dev='cpu'):
    n_frames = sum(len(f) for f in SUBJECTS.values())
    for name, want in (('val0', n_frames), ('val_skip2', n_frames // 2), ('train0', n_frames * N_CAM), ('train_skip2', n_frames * N_CAM // 2)):
        ds, _ = build(root, name, dev)
        assert len(ds) == want, (name, len(ds), want)
        assert ds.frames == ['0005', '0001', '0002'] or ds.frames == ['0001', '0002', '0005'], ds.frames
    ds, _ = build(root, 'train0', dev)
    ds.test_views = list(range(48))
    by_subject = {s: ds.view_ids(ds.subjects.index(s), 40) for s in SUBJECTS}
    assert by_subject['amanda'][-1] == 40 and by_subject['dannier'][-1] == sorted(set(range(48)) - {32})[40] == 41


def check_prepare_data(dev, root):
    """GnrNetwork.prepare_data takes next(iterate(dataset)) as it is"""
    import types
    from xrnerf_amd.gnr_network import GnrNetwork
    from xrnerf_amd.pipelines import iterate
    from xrnerf_amd.builder import ConfigDict
    model_opt = ConfigDict(use_smpl_sdf=True, use_t_pose=True, use_smpl_depth=True, projection_mode='perspective')     # the model cfg's switches
    for name, V in (('train0', NUM_VIEWS + 1), ('val0', NUM_VIEWS)):
        ds, _ = build(root, name, dev)
        batch = next(iterate(ds))
        out = GnrNetwork.prepare_data(types.SimpleNamespace(num_views=NUM_VIEWS), model_opt, batch, local_rank=torch.device(dev).index or 0)
        S = ITEMS[name][1]
        assert tuple(out['images'].shape) == (V, 3, S, S) and tuple(out['masks'].shape) == (NUM_VIEWS, 1, S, S)
        n_all = NUM_VIEWS + (1 if name == 'train0' else N_CAM)
        assert tuple(out['calibs'].shape) == (n_all, 4, 4) and tuple(out['persps'].shape) == (n_all, 4 + 5 + 2)
        assert isinstance(out['bbox'], list) and len(out['bbox']) == 4 and all(isinstance(b, np.int32) for b in out['bbox'])
        assert isinstance(out['mesh_param']['spatial_freq'], float) and tuple(out['mesh_param']['center'].shape) == (3,)
        assert set(out['smpl']) == {'rot', 'verts', 'faces', 't_verts', 't_faces', 'depth'} and tuple(out['smpl']['depth'].shape) == (NUM_VIEWS, 1, S, S)
        assert tuple(out['smpl']['rot'].shape) == (1, 3, 3) and out['scan'] is None
        if name == 'val0':
            assert tuple(batch['render_gt'].shape) == (1, N_CAM, 3, S, S)


def check_symbols():
    """the header, the ctypes table and the library name the same entry points"""
    import re
    from xrnerf_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_genebody.h')).read()
    declared = set(re.findall(r'^(?:int|size_t)\s+(xr_gb_\w+)\(', text, re.M))
    assert declared == set(_lib.GENEBODY_SIGNATURES), (declared, set(_lib.GENEBODY_SIGNATURES))
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    for name, (res, args) in _lib.GENEBODY_SIGNATURES.items():
        decl = re.search(r'%s\((.*?)\);' % name, text, re.S).group(1)
        assert len(decl.split(',')) == len(args), name
