"""The shared bodies of the evaluation tests (xrnerf_amd/evaluate.py, xrnerf_amd/csrc/xr_eval.hip).  Every check_* takes the device, so
tests/test_gpu_eval.py runs it on the MI355X, tests/test_emu_eval.py on the kernels' host build and tests/test_eval_host.py on the
tensor-op path.

References (tests/golden/ref_eval.npz, made by tests/golden/make_golden_eval.py):
  truth     tests/eval_restatement.py's direct sum in np.longdouble, rounded to double
  scipy64   skimage's documented algorithm composed from scipy.ndimage.uniform_filter / gaussian_filter in float64
  direct64  the same direct sum run in float64 (computed here, once per case)
Bars (none of them a hard-coded number):
  S map     |got - truth| <= 4 max(|scipy64 - truth|, |direct64 - truth|), maxima over the case -- 4 is the project's factor, and both
            float64 witnesses count because the kernels' summation order (rows, then columns) is neither's
  SSIM      the same rule on the means, with a floor of N 2^-53, N = H W C: the bound of an ordered sum of N terms of magnitude <= 1,
            divided by N
  MSE       |got - ref64| <= max(4 |ref32 - ref64|, 2^-22 ref64): numpy's own fp32 result is the witness; 2^-22 covers the difference
            rounded to fp32 (2^-24 relative, doubled by the square) twice over
  to8b      byte for byte; a second run of any call: the same bits"""
import json
import logging
import math
import os
import re
import sys
import tempfile
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')

import eval_restatement as RS  # noqa: E402

DATA_RANGE = 2.0                # evaluate.REFERENCE_SSIM_DATA_RANGE, the hooks' reading (the fixture is made with it)
# name, B, H, W, C, gaussian: the smallest shapes at which it can go wrong -- 7 x 7: every window reflects on both sides of both axes;
# 11 x 11 the same for the Gaussian window; 37 x 70: a ragged last tile on both axes (tiles are 8 x 32); 130 x 67: 17 x 3 tiles, so
# the fold adds runs of several partials; const: a flat white gt, the variance cancellation on every pixel
CASES = (('7x7', 1, 7, 7, 3, False), ('7x9', 1, 7, 9, 1, False), ('11x11g', 1, 11, 11, 3, True), ('9x13', 3, 9, 13, 4, False),
         ('37x70', 1, 37, 70, 3, False), ('130x67', 1, 130, 67, 1, False), ('37x70g', 1, 37, 70, 3, True), ('const', 1, 9, 12, 3, False))
CASE_NAMES = tuple(c[0] for c in CASES)


def generate(name):
    """(rgb, gt) [B,H,W,C] fp32: gt is U(0,1) with one half set to exactly 1.0 -- a flat white background, which drives the variance
    cancellation to zero -- and rgb = gt + 0.05 N(0,1)"""
    _, B, H, W, C, _ = next(c for c in CASES if c[0] == name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    gt = rng.uniform(0, 1, (B, H, W, C)).astype(np.float32)
    if name == 'const':
        gt[:] = 1.0
    else:
        for b in range(B):
            if b % 2 == 0:
                gt[b, :, W // 2:] = 1.0
            else:
                gt[b, H // 2:] = 1.0
    rgb = (gt + 0.05 * rng.normal(0, 1, gt.shape)).astype(np.float32)
    return rgb, gt


_cache = {}


def gold():
    if 'gold' not in _cache:
        _cache['gold'] = np.load(os.path.join(G, 'ref_eval.npz'))
    return _cache['gold']


def case(name):
    """the stored inputs and references of one case, with the float64 direct sum and the bars (computed once)"""
    if name not in _cache:
        g = gold()
        _, B, H, W, C, gauss = next(c for c in CASES if c[0] == name)
        k = lambda what: g['%s.%s' % (name, what)]
        rgb, gt, truth, scipy64 = k('rgb'), k('gt'), k('map_truth'), k('map_scipy64')
        direct64 = np.stack([RS.ssim_map(rgb[b], gt[b], 7, gauss, DATA_RANGE, np.float64) for b in range(B)])
        N = H * W * C
        mean_direct = direct64.reshape(B, -1).mean(1)
        map_bar = 4 * max(np.abs(scipy64 - truth).max(), np.abs(direct64 - truth).max())
        mean_bar = np.maximum(4 * np.maximum(np.abs(k('mean_scipy64') - k('mean_truth')), np.abs(mean_direct - k('mean_truth'))), N * 2.0 ** -53)
        mse_bar = np.maximum(4 * np.abs(k('mse32').astype(np.float64) - k('mse64')), 2.0 ** -22 * k('mse64'))
        _cache[name] = dict(B=B, H=H, W=W, C=C, gauss=gauss, rgb=rgb, gt=gt, truth=truth, scipy64=scipy64, direct64=direct64, mean_truth=k('mean_truth'),
                            mse64=k('mse64'), to8b=k('to8b'), map_bar=float(map_bar), mean_bar=mean_bar, mse_bar=mse_bar,
                            witness=(float(np.abs(scipy64 - truth).max()), float(np.abs(direct64 - truth).max())))
    return _cache[name]


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    assert a.shape == b.shape and a.dtype == b.dtype, '%s: %r %s against %r %s' % (what, a.shape, a.dtype, b.shape, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), '%s: the bits differ' % what


def E():
    from xrnerf_amd import evaluate
    return evaluate


# ------------------------------------------------------------------------------------------ the fixture
def check_fixture(dev, name):
    """map, mean, MSE and the 8-bit pair of one case against the stored references under their bars; every figure is printed before
    it is asserted; a second run gives the same bits; [H,W,C] and [H,W] inputs are the batch's images"""
    ev, c = E(), case(name)
    x, y = torch.from_numpy(c['rgb']).to(dev), torch.from_numpy(c['gt']).to(dev)
    kw = dict(data_range=DATA_RANGE, gaussian_weights=c['gauss'])
    mean, smap = ev.calculate_ssim(x, y, full=True, **kw)
    again = ev.calculate_ssim(x, y, full=True, **kw)
    sync()
    assert mean.dtype == torch.float64 and smap.dtype == torch.float64 and tuple(mean.shape) == (c['B'],) and tuple(smap.shape) == x.shape
    assert mean.device.type == dev.type and smap.device.type == dev.type
    same_bits(mean, again[0], '%s second run mean' % name)
    same_bits(smap, again[1], '%s second run map' % name)
    map_err = float(np.abs(host(smap) - c['truth']).max())
    mean_err = np.abs(host(mean) - c['mean_truth'])
    print('EVAL %s %s map |got-truth| %.3e bar %.3e (scipy64 %.3e direct64 %.3e) mean %.3e bar %.3e'
          % (dev.type, name, map_err, c['map_bar'], c['witness'][0], c['witness'][1], mean_err.max(), c['mean_bar'].min()))
    mses = torch.stack([ev.img2mse(x[b], y[b]) for b in range(c['B'])])
    mse_err = np.abs(host(mses) - c['mse64'])
    print('EVAL %s %s mse |got-ref64| %.3e bar %.3e' % (dev.type, name, mse_err.max(), c['mse_bar'].min()))
    assert 0.5 < float(mean.min()) and float(mean.max()) < 1.0
    assert map_err <= c['map_bar'], (name, map_err, c['map_bar'])
    assert (mean_err <= c['mean_bar']).all(), (name, mean_err, c['mean_bar'])
    assert mses.dtype == torch.float64 and (mse_err <= c['mse_bar']).all(), (name, mse_err, c['mse_bar'])
    for b in range(c['B']):
        m1, s1 = ev.calculate_ssim(x[b], y[b], full=True, **kw)
        assert m1.dim() == 0 and tuple(s1.shape) == tuple(x[b].shape)
        same_bits(m1, mean[b], '%s image %d alone: mean' % (name, b))
        same_bits(s1, smap[b], '%s image %d alone: map' % (name, b))
        same_bits(ev.to8b_pair(x[b], y[b]), c['to8b'][b], '%s to8b pair %d' % (name, b))
        same_bits(host(ev.to8b(x[b])), c['to8b'][b][:, :c['W']], '%s to8b %d' % (name, b))
    if c['C'] == 1:
        m2, s2 = ev.calculate_ssim(x[0, :, :, 0], y[0, :, :, 0], full=True, **kw)
        same_bits(m2, mean[0], '%s [H,W]: mean' % name)
        same_bits(s2, smap[0, :, :, 0], '%s [H,W]: map' % name)
    psnr = ev.mse2psnr(mses)
    assert np.allclose(host(psnr), [RS.mse2psnr(float(m)) for m in c['mse64']], rtol=0, atol=1e-5)
    return map_err, float(mean_err.max()), float(mse_err.max())


# ------------------------------------------------------------------------------------------ layouts
def check_views_and_slices(dev):
    """a [3,H,W] channel-first view through psnr_metric / ssim_metric, and a slice of a wider buffer whose neighbouring columns hold
    NaN: both give the bits of the contiguous channel-last image, and the buffers are as they were"""
    ev, c = E(), case('37x70')
    x, y = torch.from_numpy(c['rgb'][0]).to(dev), torch.from_numpy(c['gt'][0]).to(dev)
    mean = ev.calculate_ssim(x, y, data_range=DATA_RANGE)
    mse = ev.img2mse(x, y)
    xc, yc = x.permute(2, 0, 1).contiguous(), y.permute(2, 0, 1).contiguous()          # [3,H,W]
    same_bits(ev.ssim_metric(xc, yc), mean, 'ssim_metric on [3,H,W]')
    same_bits(ev.psnr_metric(xc, yc), ev.mse2psnr(mse), 'psnr_metric on [3,H,W]')
    assert ev.ssim_metric(xc, yc).dim() == 0 and abs(float(mean) - float(c['mean_truth'][0])) <= c['mean_bar'][0]
    H, W = c['H'], c['W']
    wide_x = torch.full((H, W + 11, 3), float('nan'), device=dev)
    wide_y = torch.full((H, W + 11, 3), float('nan'), device=dev)
    wide_x[:, 4:4 + W], wide_y[:, 4:4 + W] = x, y
    keep_x, keep_y = wide_x.clone(), wide_y.clone()
    sx, sy = wide_x[:, 4:4 + W], wide_y[:, 4:4 + W]
    assert not sx.is_contiguous()
    m2, s2 = ev.calculate_ssim(sx, sy, data_range=DATA_RANGE, full=True)
    same_bits(m2, mean, 'slice of a wider buffer: mean')
    same_bits(s2, ev.calculate_ssim(x, y, data_range=DATA_RANGE, full=True)[1], 'slice of a wider buffer: map')
    same_bits(ev.img2mse(sx, sy), mse, 'slice of a wider buffer: mse')
    same_bits(ev.to8b_pair(sx, sy), c['to8b'][0], 'slice of a wider buffer: to8b pair')
    sync()
    same_bits(wide_x, keep_x, 'the wider buffer of x')
    same_bits(wide_y, keep_y, 'the wider buffer of y')
    # the batch of a sliced buffer and images whose strides differ
    c3 = case('9x13')
    xb, yb = torch.from_numpy(c3['rgb']).to(dev), torch.from_numpy(c3['gt']).to(dev)
    want = ev.calculate_ssim(xb, yb, data_range=DATA_RANGE)
    big = torch.zeros((5, 9, 13, 4), device=dev)
    big[1:4] = xb
    same_bits(ev.calculate_ssim(big[1:4], yb, data_range=DATA_RANGE), want, 'batch slice')
    same_bits(ev.calculate_ssim(xb.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), yb, data_range=DATA_RANGE), want, 'differing strides')


def check_degenerate(dev):
    """identical images: mse exactly 0, psnr inf, ssim within the floor of 1; NaN and out-of-range values through to8b"""
    ev, c = E(), case('37x70')
    x = torch.from_numpy(c['rgb'][0]).to(dev)
    mse = ev.img2mse(x, x.clone())
    mean, smap = ev.calculate_ssim(x, x.clone(), data_range=DATA_RANGE, full=True)
    assert float(mse) == 0.0 and math.isinf(float(ev.mse2psnr(mse))) and float(ev.mse2psnr(mse)) > 0
    assert abs(float(mean) - 1.0) <= x.numel() * 2.0 ** -53 and float(np.abs(host(smap) - 1.0).max()) <= x.numel() * 2.0 ** -53
    assert math.isinf(float(ev.mse2psnr(0.0)))
    odd = torch.tensor([[[float('nan'), -0.0, -3.0], [1.0, 1.5, 0.999999], [0.5, 0.25, 0.75]]], device=dev)
    got = host(ev.to8b(odd))
    assert got.dtype == np.uint8 and got.tolist() == [[[0, 0, 0], [255, 255, 254], [127, 63, 191]]], got.tolist()
    same_bits(ev.to8b_pair(odd, odd), np.concatenate([got, got], 1), 'to8b pair of odd values')


# ------------------------------------------------------------------------------------------ refusals
def check_refusals(dev):
    """H < win, an even window, a radius above 5: ValueError in Python, as skimage refuses them"""
    ev = E()
    x = torch.zeros((6, 9, 3), device=dev)
    with pytest.raises(ValueError, match='win_size exceeds image extent'):
        ev.calculate_ssim(x, x)
    with pytest.raises(ValueError, match='win_size exceeds image extent'):
        ev.calculate_ssim(x.permute(1, 0, 2), x.permute(1, 0, 2))
    with pytest.raises(ValueError, match='win_size exceeds image extent'):
        ev.calculate_ssim(torch.zeros((10, 12, 3), device=dev), torch.zeros((10, 12, 3), device=dev), gaussian_weights=True)
    big = torch.zeros((16, 16, 3), device=dev)
    with pytest.raises(ValueError, match='odd'):
        ev.calculate_ssim(big, big, win_size=8)
    with pytest.raises(ValueError):
        ev.calculate_ssim(big, big, win_size=13)
    with pytest.raises(ValueError):
        ev.calculate_ssim(big, big[:, :15])
    assert float(ev.calculate_ssim(big, big, win_size=11)) == 1.0 and float(ev.calculate_ssim(big, big, win_size=3)) == 1.0


def check_kernel_refusals(dev):
    """ops.* and the C entry points: a radius above 5, C outside 1 .. 4, H or W below 2 r + 1, null pointers, a small or misaligned
    workspace are refused (-22 / -12), launch nothing and leave every output untouched"""
    import ctypes as C
    from xrnerf_amd import _lib, ops
    x = torch.rand((1, 9, 9, 3), device=dev)
    with pytest.raises(_lib.XrError):
        ops.eval_ssim(x, x, [1.0 / 13] * 13, 1.0, 1e-4, 9e-4)
    with pytest.raises(_lib.XrError):
        ops.eval_ssim(x, x, [0.5, 0.5], 1.0, 1e-4, 9e-4)
    with pytest.raises(_lib.XrError):
        ops.eval_ssim(x, x, [1.0 / 11] * 11, 1.0, 1e-4, 9e-4)                    # 9 < 11
    five = torch.rand((1, 9, 9, 5), device=dev)
    with pytest.raises(_lib.XrError):
        ops.eval_ssim(five, five, [1.0 / 7] * 7, 1.0, 1e-4, 9e-4)
    with pytest.raises(_lib.XrError):
        ops.eval_ssim(x.double(), x.double(), [1.0 / 7] * 7, 1.0, 1e-4, 9e-4)
    with pytest.raises(_lib.XrError):
        ops.eval_to8b_pair(five[0])
    assert ops.eval_workspace_bytes(1, 8, 32, 3) == 16 and ops.eval_workspace_bytes(1, 9, 9, 3) == 32 and ops.eval_workspace_bytes(3, 130, 67, 1) == 3 * 17 * 3 * 16
    assert ops.eval_workspace_bytes(1, 9, 9, 5) == 0 and ops.eval_workspace_bytes(0, 9, 9, 3) == 0 and ops.eval_workspace_bytes(4, 32768, 32768, 1) == 0
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    taps = (C.c_double * 13)(*([1.0 / 7] * 13))
    sums, sq = torch.full((1,), 7.0, dtype=torch.float64, device=dev), torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    smap = torch.full((1, 9, 9, 3), 7.0, dtype=torch.float64, device=dev)
    ws = torch.zeros(64, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 8
    xc = x.contiguous()

    def call(H=9, W=9, Cn=3, B=1, r=3, px=p(xc), py=p(xc), pt=taps, ps=p(sums), stride=27, nbytes=32, shift=0):
        return lib.xr_eval_ssim(px, py, B, H, W, Cn, 243, stride, 3, 1, pt, r, 49.0 / 48, 1e-4, 9e-4, ps, p(sq), p(smap),
                                C.c_void_p(ws.data_ptr() + off + shift), nbytes, None)
    assert call(H=6) == -22 and call(W=6) == -22 and call(r=6) == -22 and call(Cn=0) == -22 and call(Cn=5) == -22 and call(B=0) == -22
    assert call(px=None) == -22 and call(py=None) == -22 and call(pt=None) == -22 and call(ps=None) == -22 and call(stride=-27) == -22
    assert call(shift=4) == -22 and call(nbytes=16) == -12
    assert call(H=6) == -22 and 'win_size exceeds image extent' in (lib.last_errors() if hasattr(lib, 'last_errors') else lib.xr_last_error().decode())
    out8 = torch.full((9, 18, 3), 7, dtype=torch.uint8, device=dev)
    to8 = lambda H=9, W=9, Cn=3, a=p(xc), o=p(out8), s=27: lib.xr_eval_to8b_pair(a, p(xc), H, W, Cn, s, 3, 1, o, None)
    assert to8(H=0) == -22 and to8(W=0) == -22 and to8(Cn=5) == -22 and to8(a=None) == -22 and to8(o=None) == -22 and to8(s=-1) == -22
    sync()
    assert bool((sums == 7).all()) and bool((sq == 7).all()) and bool((smap == 7).all()) and bool((out8 == 7).all())
    assert call() == 0 and to8() == 0
    sync()
    assert not bool((smap == 7).any()) and float(sums[0]) != 7.0 and not bool((out8 == 7).all())


def check_symbols():
    """the header, the ctypes table and the library name the same xr_eval_* entry points; the table is disjoint from every other"""
    from xrnerf_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_eval.h')).read()
    declared = set(re.findall(r'^(?:int|size_t) (xr_eval_\w+)\(', header, re.M))
    assert declared == set(_lib.EVAL_SIGNATURES) and len(declared) == 3
    lib = _lib.load()
    for name, (res, args) in _lib.EVAL_SIGNATURES.items():
        text = header[header.index(' %s(' % name):]
        text = text[:text.index(');')]
        assert text.count(',') + 1 == len(args), name
        assert hasattr(lib, name), name
    others = [v for k, v in vars(_lib).items() if k.endswith('SIGNATURES') and k != 'EVAL_SIGNATURES']
    assert len(others) >= 10 and not any(set(t) & set(_lib.EVAL_SIGNATURES) for t in others)
    assert not any(k.startswith('xr_eval') for t in others for k in t)
    assert 'xr_eval' not in open(os.path.join(ROOT, 'include', 'xrnerf_mi355.h')).read()
    assert ops.eval_kernels_available()
    from xrnerf_amd import build
    assert build.SOURCES['xr_eval.hip'] == ['-ffp-contract=off']


# ------------------------------------------------------------------------------------------ hooks
class Runner:
    """what the hooks take: .outputs, .iter, .work_dir, .logger"""

    def __init__(self, work_dir, outputs, it=500):
        self.outputs, self.iter, self.work_dir, self.lines = outputs, it, work_dir, []
        self.logger = logging.getLogger('eval_cases.%d' % id(self))
        self.logger.setLevel(logging.INFO)
        self.logger.propagate = False
        runner = self

        class Keep(logging.Handler):
            def emit(self, record):
                runner.lines.append(record.getMessage())
        self.logger.addHandler(Keep())


def frames(dev, kind):
    """the three 9 x 13 RGBA frames of the fixture as numpy arrays, or as tensors on the device"""
    c = case('9x13')
    if kind == 'numpy':
        return c, [a for a in c['rgb']], [a for a in c['gt']]
    return c, [torch.from_numpy(a).to(dev) for a in c['rgb']], [torch.from_numpy(a).to(dev) for a in c['gt']]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def check_validate_hook(dev, kind):
    """the log line equals the literal derived from the fixture's scalars; the PNGs read back are the stored 8-bit pairs; the two
    early returns write nothing"""
    ev = E()
    c, rgbs, gts = frames(dev, kind)
    psnr64 = [RS.mse2psnr(float(m)) for m in c['mse64']]
    want = 'On testset, mse is {:.5f}, psnr is {:.5f}, ssim is {:.5f}'.format(float(c['mse64'].mean()), sum(psnr64) / 3, float(c['mean_truth'].mean()))
    with tempfile.TemporaryDirectory() as tmp:
        run = Runner(tmp, {'rgbs': rgbs, 'gt_imgs': gts, 'elapsed_time': [0.004, 0.006]})
        ev.ValidateHook().after_val_iter(run)
        assert run.lines == [want], (run.lines, want)
        names = sorted(os.listdir(os.path.join(tmp, 'validation', '500')))
        assert names == ['000.png', '001.png', '002.png']
        for i, n in enumerate(names):
            same_bits(_png(os.path.join(tmp, 'validation', '500', n)), c['to8b'][i], 'ValidateHook %s' % n)
        ev.CalElapsedTimeHook().after_val_iter(run)
        assert run.lines[1] == 'On testset, elapsed_time is    5.00 ms'
        for outputs in ({'rgbs': [], 'gt_imgs': []}, {'rgbs': rgbs, 'gt_imgs': [g[:, :12] for g in gts]}):
            quiet = Runner(os.path.join(tmp, 'quiet'), outputs)
            ev.ValidateHook('other').after_val_iter(quiet)
            ev.CalElapsedTimeHook().after_val_iter(quiet)
            assert quiet.lines == [] and not os.path.exists(os.path.join(tmp, 'quiet'))
    assert ev.REFERENCE_SSIM_DATA_RANGE == DATA_RANGE


def check_test_hook(dev, kind):
    """three frames at ndown = 2: scales 0, 1, 0; the log's numbers are the fixture's within the bars; test_results.json has the
    reference's keys; the saved PNGs are to8b(rgb)"""
    ev = E()
    c, rgbs, gts = frames(dev, kind)
    psnr64 = [RS.mse2psnr(float(m)) for m in c['mse64']]
    with tempfile.TemporaryDirectory() as tmp:
        run = Runner(tmp, {})
        run._epoch = 0
        hook = ev.TestHook(ndown=2, save_img=True, dump_json=True)
        hook.before_val_epoch(run)
        for i in range(3):
            run.outputs = {'rgb': rgbs[i], 'gt_img': gts[i], 'idx': i}
            hook.after_val_iter(run)
        hook.after_val_epoch(run)
        assert run._epoch == 1 and len(run.lines) == 1
        line = run.lines[0]
        assert line.startswith('In test phase on whole testset, \n   for scale 0, mse is ') and line.endswith('. \n')
        got = re.findall(r' for scale (\d), mse is (\S+), psnr is (\S+), ssim is (\S+)\. \n', line)
        assert [g[0] for g in got] == ['0', '1']
        for (_, mse, psnr, ssim), idx in zip(got, ((0, 2), (1,))):
            ix = list(idx)
            assert abs(float(mse) - c['mse64'][ix].mean()) <= c['mse_bar'][ix].max()
            assert abs(float(ssim) - c['mean_truth'][ix].mean()) <= c['mean_bar'][ix].max()
            assert abs(float(psnr) - sum(psnr64[i] for i in ix) / len(ix)) <= 1e-5
        res = json.load(open(os.path.join(tmp, 'test', 'test_results.json')))
        assert sorted(res) == ['psnrs', 'results', 'ssims'] and res['results'] == line
        assert sorted(res['psnrs']) == ['0', '1'] and len(res['psnrs']['0']) == 2 and len(res['ssims']['1']) == 1
        assert res['ssims']['0'] == hook.ssim[0] and res['psnrs']['1'] == hook.psnr[1]
        for i in range(3):
            same_bits(_png(os.path.join(tmp, 'test', '%03d.png' % i)), c['to8b'][i][:, :c['W']], 'TestHook %03d.png' % i)
        hook = ev.TestHook()
        hook.before_val_epoch(run)
        assert hook.psnr == {0: []} and hook.ndown == 1 and not hook.save_img and not hook.dump_json and hook.save_folder == 'test'


# ------------------------------------------------------------------------------------------ evaluate_frames
class ReadCounter:
    """counts the reads of a tensor's values by the host -- Tensor.cpu / item / tolist / numpy / __float__ and evaluate._read_back, a
    nested call counting once -- made outside `paused` spans"""

    def __init__(self):
        self.count, self.paused = 0, False

    def __enter__(self):
        T = torch.Tensor
        self.saved = {k: getattr(T, k) for k in ('cpu', 'item', 'tolist', 'numpy', '__float__')}
        ev = E()
        self.saved_rb, counter, depth = ev._read_back, self, [0]

        def wrap(fn):
            def inner(t, *a, **k):
                outer = depth[0] == 0 and not counter.paused
                depth[0] += 1
                try:
                    out = fn(t, *a, **k)
                finally:
                    depth[0] -= 1
                counter.count += int(outer)
                return out
            return inner
        for k, fn in self.saved.items():
            setattr(T, k, wrap(fn))
        ev._read_back = wrap(self.saved_rb)
        return self

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(torch.Tensor, k, fn)
        E()._read_back = self.saved_rb
        return False


def check_evaluate_frames(dev, render, poses, gts_rgba):
    """evaluate_frames equals the hooks run on the host on the same (alpha-masked) frames within the bars, the bars taken from the
    long-double truth and the two float64 witnesses of these very frames; it makes exactly one blocking read outside the renderer"""
    ev = E()
    rendered = []
    counter = ReadCounter()

    def traced(pose):
        counter.paused = True
        try:
            out = render(pose)
        finally:
            counter.paused = False
        rendered.append((out[0] if isinstance(out, (tuple, list)) else out).clone())
        return out
    with counter:
        res = ev.evaluate_frames(traced, poses, gts_rgba)
    assert counter.count == 1, 'evaluate_frames made %d blocking reads' % counter.count
    n = len(poses)
    assert len(rendered) == n and [len(res[k]) for k in ('mse', 'psnr', 'ssim')] == [n, n, n]
    rgbs, gt_imgs = [], []
    for i in range(n):
        img = host(gts_rgba[i]).astype(np.float32)
        alpha = img[:, :, 3:]
        rgbs.append(host(rendered[i]) * alpha)
        gt_imgs.append(img[:, :, :3] * alpha)
    with tempfile.TemporaryDirectory() as tmp:
        run = Runner(tmp, {'rgbs': rgbs, 'gt_imgs': gt_imgs})
        ev.ValidateHook().after_val_iter(run)
    hooks = [float(v) for v in re.findall(r'is (\S+?)(?:,|$)', run.lines[0])]
    for i in range(n):
        truth = RS.ssim_map(rgbs[i], gt_imgs[i], 7, False, DATA_RANGE, np.longdouble)
        wit = [RS.ssim_map(rgbs[i], gt_imgs[i], 7, False, DATA_RANGE, np.float64), RS.scipy_ssim_map(rgbs[i], gt_imgs[i], 7, False, DATA_RANGE)]
        mean_truth = float(truth.mean())
        bar = max(4 * max(abs(float(w.mean()) - mean_truth) for w in wit), truth.size * 2.0 ** -53)
        m64, m32 = float(RS.img2mse64(rgbs[i], gt_imgs[i])), float(RS.img2mse32(rgbs[i], gt_imgs[i]))
        mbar = max(4 * abs(m32 - m64), 2.0 ** -22 * m64)
        host_row = host(ev.frame_metrics(rgbs[i], gt_imgs[i]))
        print('EVAL %s evaluate_frames %d ssim |got-truth| %.3e (host %.3e) bar %.3e mse |got-ref64| %.3e bar %.3e'
              % (dev.type, i, abs(res['ssim'][i] - mean_truth), abs(host_row[2] - mean_truth), bar, abs(res['mse'][i] - m64), mbar))
        assert abs(res['ssim'][i] - mean_truth) <= bar and abs(host_row[2] - mean_truth) <= bar
        assert abs(res['mse'][i] - m64) <= mbar and abs(host_row[0] - m64) <= mbar
        assert abs(res['psnr'][i] - RS.mse2psnr(m64)) <= 1e-5
    assert res['log'].startswith('On testset, mse is ')
    got = [float(v) for v in re.findall(r'is (\S+?)(?:,|$)', res['log'])]
    assert len(got) == 3 and len(hooks) == 3 and all(abs(a - b) <= 1.01e-5 for a, b in zip(got, hooks)), (res['log'], run.lines[0])
    assert ev.evaluate_frames(traced, [], [])['log'] is None


def fixture_renderer(dev):
    """a renderer that hands out the fixture's 37 x 70 frame and a shifted copy, with RGBA ground truths (a flat alpha of 0 / 0.5 / 1)"""
    c = case('37x70')
    rgb = torch.from_numpy(c['rgb'][0]).to(dev)
    outs = [rgb, (rgb * 0.9 + 0.03).contiguous()]
    rng = np.random.default_rng(11)
    gts = []
    for i in range(2):
        alpha = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), (37, 70, 1))
        gts.append(torch.from_numpy(np.concatenate([c['gt'][0], alpha], -1)))
    return (lambda pose: (outs[int(pose)], None)), [0, 1], gts
