"""The GeneBody data side at the shapes of configs/gnr/gnr_genebody.py: 2448 x 2048 pictures cropped and resized to 512, a training item
(4 + 1 views) and an evaluation item (4 + 48 views) over a body of 10 475 vertices, on generated pictures.

Reported apart, because they are paid at different times:
  decode     host: PIL's decode of one view's picture, mask and 16-bit depth PNG (paid once per view, on the host, whatever the device does)
  upload     the raw views packed and copied to the device (once per view)
  prepare    xr_gb_crop_box + xr_gb_resize over the uploaded views (once per view; csrc/xr_genebody.hip)
  item       xr_gb_assemble + xr_gb_calib over resident views: what a warm item costs
  host       the same item in numpy on the host (tests/genebody_restatement.py: crop rule, both resizes, roles, K, near / far,
             spatial_freq), which is the arithmetic the reference runs per item through cv2 -- outputs compared for equality first
Device rows alternate window by window in one process; a host clock around work that ends in a device synchronise.

  python tools/microbench_genebody.py [--out profiles/genebody_microbench.txt] [--size 512] [--height 2048] [--width 2448]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from microbench_pipeline import windows  # noqa: E402


def picture(rng, h, w, shift):
    """a person-sized blob on a textured background: picture, mask (0 / 255 with a 128 / 129 rim), depth in millimetres inside the body"""
    yy, xx = np.mgrid[:h, :w]
    body = ((xx - (0.5 + 0.02 * shift) * w) / (0.12 * w)) ** 2 + ((yy - 0.5 * h) / (0.4 * h)) ** 2
    img = (np.stack([xx % 256, yy % 256, (xx + yy) % 256], axis=-1) ^ rng.integers(0, 32, (h, w, 1))).astype(np.uint8)
    mask = np.where(body < 1, 255, np.where(body < 1.02, 129, np.where(body < 1.04, 128, 0))).astype(np.uint8)
    depth = np.where(body < 0.9, 2500 + 200 * body, 0).astype(np.uint16)
    return img, mask, depth


def host_ms(f, n=3):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--height', type=int, default=2048)
    ap.add_argument('--width', type=int, default=2448)
    args = ap.parse_args()
    from PIL import Image
    import genebody_restatement as RS
    from xrnerf_amd import genebody, ops
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')
    S, h, w, nv = args.size, args.height, args.width, 4
    rng = np.random.default_rng(0)
    lines = ['GeneBody data on %s: %d x %d pictures -> %d, %d input views, 10475 vertices (device rows: median of 5 alternating windows, ms; min .. max)'
             % (torch.cuda.get_device_name(0), w, h, S, nv)]
    pics = [picture(rng, h, w, i) for i in range(5)]                        # four input views and a target
    # ---- decode (host)
    with tempfile.TemporaryDirectory() as tmp:
        for name, a in zip(('image', 'mask', 'depth'), pics[0]):
            Image.fromarray(a).save(os.path.join(tmp, name + '.png'))
        dec = {name: host_ms(lambda name=name: genebody.read_image(os.path.join(tmp, name + '.png'))) for name in ('image', 'mask', 'depth')}
        assert genebody.read_image(os.path.join(tmp, 'depth.png')).dtype == np.uint16
    per_view = dec['image'][0] + dec['mask'][0]
    lines.append('decode (host, PIL, per view): picture %.1f ms (%.1f .. %.1f), mask %.1f ms, 16-bit depth %.1f ms -> train item %d views + %d depths: %.0f ms, evaluation item 48 views + %d depths: %.0f ms'
                 % (dec['image'] + (dec['mask'][0], dec['depth'][0], 5, nv, 5 * per_view + nv * dec['depth'][0], nv, 48 * per_view + nv * dec['depth'][0])))

    # ---- upload and prepare
    def views(n):
        return [(pics[i % 5][0], pics[i % 5][1], pics[i % 5][2] if i < nv else None) for i in range(n)]

    def upload(vs):
        imgs, io = ops.gb_pack([v[0] for v in vs], np.uint8, dev)
        masks, mo = ops.gb_pack([v[1] for v in vs], np.uint8, dev)
        depths, do = ops.gb_pack([v[2] for v in vs if v[2] is not None], np.uint16, dev)
        do = iter(do)
        entries = [(i, m, next(do) if v[2] is not None else -1, h, w) for i, m, v in zip(io, mo, vs)]
        return imgs, masks, depths, entries

    def prepare(up):
        imgs, masks, depths, entries = up
        boxes = ops.gb_crop_box((masks, [(e[1], h, w) for e in entries]))
        return (boxes,) + ops.gb_resize(imgs, masks, depths, entries, boxes, S)
    for n, what in ((5, 'train item, 5 views'), (48, 'evaluation item, 48 views')):
        vs = views(n)
        t_up = host_ms(lambda: (upload(vs), torch.cuda.synchronize()))
        up = upload(vs)
        res = windows({'prepare': (lambda: prepare(up), 5)})
        mb = sum(v[0].nbytes + v[1].nbytes + (v[2].nbytes if v[2] is not None else 0) for v in vs) / 1e6
        lines.append('%s: upload of %.0f MB (pack on the host + copy) %.1f ms (%.1f .. %.1f); prepare (crop_box + resize, 2 launches) %.3f ms (%.3f .. %.3f)'
                     % ((what, mb) + t_up + res['prepare']))
        del up
    # ---- warm items
    boxes, rgb, m8, depth = prepare(upload(views(5)))
    verts_np = rng.uniform([-0.45, -0.9, -0.2], [0.45, 0.9, 0.2], (10475, 3)).astype(np.float32)
    verts = torch.from_numpy(verts_np).to(dev)

    def cams(V):
        K = np.tile(np.array([[2200., 0, 0.5 * w], [0, 2200., 0.5 * h], [0, 0, 1]], np.float32), (V, 1, 1))
        w2c = np.tile(np.eye(4, dtype=np.float32), (V, 1, 1))
        w2c[:, 2, 3] = 3.0
        w2c[:, 0, 3] = np.linspace(-0.1, 0.1, V)
        return K, np.zeros((V, 5), np.float32), w2c

    def item(V, cam):
        at = list(range(nv)) + [4 if V == 5 else i % 5 for i in range(V - nv)]
        img, mask, sd, acc = ops.gb_assemble([rgb[i] for i in at], [m8[i] for i in at], [depth[i] for i in range(nv)], nv, S, False)
        return img, mask, sd, ops.gb_calib(verts, cam[0], cam[1], cam[2], [boxes[i] for i in at], acc, nv, S)
    cam5, cam52 = [tuple(torch.from_numpy(a).to(dev) for a in cams(V)) for V in (5, 52)]
    # the host's train item, compared first
    K5, D5, w2c5 = cams(5)

    def host_item():
        out = []
        for i in range(5):
            r, m, d, box = RS.prepare_view(pics[i][0], pics[i][1], pics[i][2] if i < nv else None, S)
            x, mf, vb = RS.assemble_view(r, m, d, i < nv, False)
            Ka = RS.adjusted_K(K5[i], box, S)
            out.append((x, mf, vb, RS.near_far64(verts_np, w2c5[i]), RS.spatial_freq64(verts_np, vb, w2c5[i], Ka) if i < nv else None))
        return out
    t_host = host_ms(host_item, 2)
    ref = host_item()
    img, mask, sd, c = item(5, cam5)
    torch.cuda.synchronize()
    assert np.array_equal(img.cpu().numpy(), np.stack([r[0] for r in ref])) and np.array_equal(mask.cpu().numpy()[:, 0], np.stack([r[1] for r in ref[:nv]]))
    assert np.array_equal(c['vboxes'].cpu().numpy(), np.array([r[2] for r in ref], np.int32).reshape(-1, 4))
    sf = min(r[4][0] for r in ref[:nv])
    assert abs(float(c['spatial_freq']) / sf - 1) <= 1e-5
    lines.append('train item, device against the host: img, mask and the mask boxes identical; spatial_freq relative difference %.1e' % abs(float(c['spatial_freq']) / sf - 1))
    res = windows({'train item (5 views)': (lambda: item(5, cam5), 50), 'evaluation item (52 views)': (lambda: item(52, cam52), 20)})
    for k, (med, lo, hi) in res.items():
        lines.append('warm %-27s assemble + calib (2 launches, 2 memsets): %.3f ms (%.3f .. %.3f)' % (k + ':', med, lo, hi))
    lines.append('host, numpy restatement of the train item (5 views: crop, cubic + nearest resize, roles, K, near / far, spatial_freq): %.0f ms (%.0f .. %.0f), %.0f ms per view'
                 % (t_host + (t_host[0] / 5,)))
    lines.append('    an evaluation item of 52 views at that rate: %.0f ms (52 x per view, not run)' % (52 * t_host[0] / 5))
    lines.append('    host / device, train item: cold (upload + prepare + item, decode apart) see above; warm %.0f x' % (t_host[0] / res['train item (5 views)'][0]))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
