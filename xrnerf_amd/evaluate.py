"""Test-set evaluation: MSE / PSNR / SSIM and the validate / test hooks of the reference (core/hooks/utils.py, validation_hooks.py:96-177,
test_hooks.py:13-94), with the frame measured where it was rendered.

Device float32 tensors run the kernels of csrc/xr_eval.hip (ops.eval_ssim, ops.eval_to8b_pair); host tensors, numpy arrays and tensors
of another dtype take a tensor-op path in torch float64 that performs the kernels' operations in the kernels' order.  SSIM is skimage's
structural_similarity as documented -- separable window, scipy's mode='reflect' boundary, S = ((2 ux uy + C1)(2 vxy + C2)) /
((ux^2 + uy^2 + C1)(vx + vy + C2)) -- and its value is the mean of the WHOLE map, which is what the reference's calculate_ssim takes
(`structural_similarity(..., full=True)[1].mean()`), not skimage's cropped mean.  Neither skimage nor scipy is imported here."""
import json
import math
import os

import numpy as np
import torch

from . import ops

# The reference's hooks call structural_similarity(im1, im2, val_range=gt.max() - gt.min(), multichannel=True, full=True).  `val_range`
# is not a parameter of skimage's function: in skimage 0.16-0.19, as remembered, the unknown keyword is swallowed by **kwargs, data_range
# stays None, and for float images it becomes dtype_range's max - min = 2.0 -- not the gt.max() - gt.min() the caller meant.  skimage is
# not installed where this was written, so this reading is UNVERIFIED; the hooks pass it through this one constant, calculate_ssim
# itself takes data_range honestly.  DESIGN.md section 19 shows one frame under both readings.
REFERENCE_SSIM_DATA_RANGE = 2.0

GAUSSIAN_SIGMA = 1.5
GAUSSIAN_RADIUS = int(3.5 * GAUSSIAN_SIGMA + 0.5)        # scipy's truncate = 3.5: radius 5, an 11 x 11 window


def _is_kernel_input(*ts):
    return all(isinstance(t, torch.Tensor) and ops._on_device(t) and t.dtype == torch.float32 for t in ts)


def _tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def _pair(x, y):
    """both images as tensors on one device: a device tensor pulls a host array over to it"""
    x, y = _tensor(x), _tensor(y)
    if x.device != y.device:
        dev = x.device if x.is_cuda else y.device
        x, y = x.to(dev), y.to(dev)
    return x, y


def window(win_size=7, gaussian_weights=False):
    """(taps, cov_norm) of skimage's two windows: uniform taps 1 / win with the sample-covariance factor win^2 / (win^2 - 1), or the
    Gaussian of sigma 1.5 truncated at radius 5, normalised to sum 1, with factor 1"""
    if gaussian_weights:
        t = [math.exp(-0.5 * (k / GAUSSIAN_SIGMA) ** 2) for k in range(-GAUSSIAN_RADIUS, GAUSSIAN_RADIUS + 1)]
        s = sum(t)
        return [v / s for v in t], 1.0
    win_size = int(win_size)
    if win_size % 2 != 1:
        raise ValueError('Window size must be odd.')
    if win_size < 1 or (win_size - 1) // 2 > ops.EVAL_MAX_RADIUS:
        raise ValueError('win_size is 1 .. %d (got %d)' % (2 * ops.EVAL_MAX_RADIUS + 1, win_size))
    return [1.0 / win_size] * win_size, (win_size * win_size / (win_size * win_size - 1.0)) if win_size > 1 else 1.0


# ------------------------------------------------------------------------------------------ the reference's utils
def img2mse(x, y):
    """mean((x - y)^2) as a 0-d float64 tensor on the images' device: the difference is rounded in the images' dtype (fp32 as numpy
    rounds it), squared and added in double.  Nothing is read back."""
    x, y = _pair(x, y)
    if _is_kernel_input(x, y) and 2 <= x.dim() <= 3 and (x.dim() == 2 or x.shape[-1] <= ops.EVAL_MAX_CHANNELS) and min(x.shape[:2]) >= 1:
        x4 = x[None, :, :, None] if x.dim() == 2 else x[None]
        y4 = y[None, :, :, None] if y.dim() == 2 else y[None]
        return ops.eval_ssim(x4, y4, [1.0], 1.0, 1.0, 1.0)[1][0] / x.numel()
    return ((x - y).double() ** 2).mean()


def mse2psnr(mse):
    """-10 ln(mse) / ln(10); mse2psnr(0) is inf, as numpy gives"""
    mse = mse if isinstance(mse, torch.Tensor) else torch.as_tensor(mse, dtype=torch.float64)
    return -10.0 * torch.log(mse) / math.log(10.0)


def to8b(x):
    """(255 clip(x, 0, 1)) truncated to uint8 -- the fp32 product first, NaN -> 0; an array gives an array, a tensor a tensor"""
    if isinstance(x, np.ndarray):
        return np.nan_to_num(255 * np.clip(x, 0, 1), nan=0.0).astype(np.uint8)
    if _is_kernel_input(x) and x.dim() == 3 and x.shape[-1] <= ops.EVAL_MAX_CHANNELS:
        return ops.eval_to8b_pair(x)
    return torch.nan_to_num(255 * x.clamp(0, 1), nan=0.0).to(torch.uint8)


def to8b_pair(rgb, gt):
    """to8b(hstack(rgb, gt)), the image ValidateHook saves, as a host uint8 array [H, 2 W, C]: a quarter of the frames' bytes cross"""
    rgb, gt = _pair(rgb, gt)
    if _is_kernel_input(rgb, gt) and rgb.dim() == 3 and rgb.shape[-1] <= ops.EVAL_MAX_CHANNELS:
        return ops.eval_to8b_pair(rgb, gt).cpu().numpy()
    return to8b(torch.cat([rgb, gt], 1)).cpu().numpy()


def _reflect_index(n, r, device):
    """scipy's mode='reflect' (numpy's 'symmetric', NOT torch's 'reflect'): -1 -> 0, -2 -> 1, n -> n-1"""
    i = torch.arange(-r, n + r, device=device)
    i = torch.where(i < 0, -i - 1, i)
    return torch.where(i >= n, 2 * n - 1 - i, i)


def _ssim_tensor_ops(x, y, taps, cov_norm, C1, C2):
    """the kernels' operations in the kernels' order on [B,H,W,C] tensors of any device, in float64: rows first, then columns, taps in
    ascending order -> (sum of S per image [B], S [B,H,W,C])"""
    x, y = x.double(), y.double()
    H, W = x.shape[1], x.shape[2]
    r = (len(taps) - 1) // 2
    iy, ix = _reflect_index(H, r, x.device), _reflect_index(W, r, x.device)
    xp, yp = x[:, iy][:, :, ix], y[:, iy][:, :, ix]

    def filt(v):
        rows = None
        for k, w in enumerate(taps):
            term = w * v[:, :, k:k + W]
            rows = term if rows is None else rows + term
        out = None
        for k, w in enumerate(taps):
            term = w * rows[:, k:k + H]
            out = term if out is None else out + term
        return out
    ux, uy, uxx, uyy, uxy = filt(xp), filt(yp), filt(xp * xp), filt(yp * yp), filt(xp * yp)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return torch.stack([S[b].sum() for b in range(S.shape[0])]), S          # (per image: an image alone gives the bits it gives in a batch)


def calculate_ssim(im1, im2, data_range=None, win_size=7, gaussian_weights=False, use_sample_covariance=True, K1=0.01, K2=0.03, full=False):
    """skimage's structural_similarity on [H,W,C], [H,W] or a batch [B,H,W,C]: the mean of the whole S map as a 0-d float64 tensor
    ([B] for a batch) on the images' device, with no blocking read; with `full` also the map (float64, the images' shape).
    data_range None is skimage's default for float images, 2.0 (dtype_range's max - min)."""
    x, y = _pair(im1, im2)
    if x.shape != y.shape:
        raise ValueError('Input images must have the same dimensions.')
    if x.dim() not in (2, 3, 4):
        raise ValueError('images are [H,W], [H,W,C] or [B,H,W,C]')
    taps, cov_norm = window(win_size, gaussian_weights)
    if not use_sample_covariance:
        cov_norm = 1.0
    shape = tuple(x.shape)
    x4 = x[None, :, :, None] if x.dim() == 2 else (x[None] if x.dim() == 3 else x)
    y4 = y[None, :, :, None] if y.dim() == 2 else (y[None] if y.dim() == 3 else y)
    if min(x4.shape[1], x4.shape[2]) < len(taps):
        raise ValueError('win_size exceeds image extent.')
    R = 2.0 if data_range is None else float(data_range)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    if _is_kernel_input(x4, y4) and 1 <= x4.shape[3] <= ops.EVAL_MAX_CHANNELS and x4.shape[0] >= 1:
        sums, _, smap = ops.eval_ssim(x4, y4, taps, cov_norm, C1, C2, want_map=full)
    else:
        sums, smap = _ssim_tensor_ops(x4, y4, taps, cov_norm, C1, C2)
    mean = sums / float(x4.shape[1] * x4.shape[2] * x4.shape[3])
    if len(shape) < 4:
        mean = mean[0]
    return (mean, smap.reshape(shape)) if full else mean


def psnr_metric(pred, gt):
    """(pred [3,H,W], gt [3,H,W]) -> 0-d tensor: the 'psnr' entry of the dict GnrNetwork.cal_metrics takes"""
    return mse2psnr(img2mse(pred.permute(1, 2, 0), gt.permute(1, 2, 0)))


def ssim_metric(pred, gt):
    """(pred [3,H,W], gt [3,H,W]) -> 0-d tensor: the 'ssim' entry of the dict GnrNetwork.cal_metrics takes (the hooks' SSIM)"""
    return calculate_ssim(pred.permute(1, 2, 0), gt.permute(1, 2, 0), data_range=REFERENCE_SSIM_DATA_RANGE)


def frame_metrics(rgb, gt):
    """[3] float64 tensor (mse, psnr, ssim) of one frame on the frames' device, as the hooks measure it; nothing is read back"""
    rgb, gt = _pair(rgb, gt)
    if _is_kernel_input(rgb, gt) and rgb.dim() == 3 and rgb.shape == gt.shape and 1 <= rgb.shape[-1] <= ops.EVAL_MAX_CHANNELS and \
            min(rgb.shape[:2]) >= 7:
        # one launch yields both sums (the same bits as img2mse's and calculate_ssim's own calls: the two sums do not meet)
        taps, cov_norm = window(7)
        R = REFERENCE_SSIM_DATA_RANGE
        ssim_sum, sq_sum, _ = ops.eval_ssim(rgb[None], gt[None], taps, cov_norm, (0.01 * R) ** 2, (0.03 * R) ** 2)
        mse = sq_sum[0] / rgb.numel()
        return torch.stack([mse, mse2psnr(mse), ssim_sum[0] / rgb.numel()])
    mse = img2mse(rgb, gt)
    return torch.stack([mse, mse2psnr(mse), calculate_ssim(rgb, gt, data_range=REFERENCE_SSIM_DATA_RANGE)])


def _read_back(t):
    """THE blocking read of this module: a small device tensor of scalars to host floats"""
    return t.detach().cpu().tolist()


def _save_png(filename, img8):
    from PIL import Image
    Image.fromarray(img8[..., 0] if img8.shape[-1] == 1 else img8).save(filename)


# ------------------------------------------------------------------------------------------ the reference's hooks
class ValidateHook:
    """core/hooks/validation_hooks.py:96-151: MSE / PSNR / SSIM over runner.outputs['rgbs'] against ['gt_imgs'], the side-by-side PNGs
    under work_dir/save_folder/<iter>/, one log line.  Frames may be numpy arrays, host tensors or device tensors."""

    def __init__(self, save_folder='validation'):
        self.save_folder = save_folder

    def after_val_iter(self, runner):
        rgbs, gt_imgs = runner.outputs['rgbs'], runner.outputs['gt_imgs']
        if len(rgbs) == 0:
            return
        if tuple(rgbs[0].shape) != tuple(gt_imgs[0].shape):
            return
        rows = _read_back(torch.stack([frame_metrics(rgb, gt_imgs[i]) for i, rgb in enumerate(rgbs)]))
        mse_list, psnr_list, ssim_list = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
        average_mse = sum(mse_list) / len(mse_list)
        average_psnr = sum(psnr_list) / len(psnr_list)
        average_ssim = sum(ssim_list) / len(ssim_list)
        testset_dir = os.path.join(runner.work_dir, self.save_folder, str(runner.iter))
        os.makedirs(testset_dir, exist_ok=True)
        for i, rgb in enumerate(rgbs):
            _save_png(os.path.join(testset_dir, '{:03d}.png'.format(i)), to8b_pair(rgb, gt_imgs[i]))
        metrics = 'On testset, mse is {:.5f}, psnr is {:.5f}, ssim is {:.5f}'.format(average_mse, average_psnr, average_ssim)
        runner.logger.info(metrics)


class CalElapsedTimeHook:
    """core/hooks/validation_hooks.py:154-177: the average of runner.outputs['elapsed_time'] in milliseconds"""

    def __init__(self, cfg=None):
        self.cfg = cfg

    def after_val_iter(self, runner):
        elapsed_time_list = runner.outputs['elapsed_time'] if 'elapsed_time' in runner.outputs else []
        if len(elapsed_time_list) == 0:
            return
        average_elapsed_time = 1000 * sum(elapsed_time_list) / len(elapsed_time_list)
        runner.logger.info('On testset, elapsed_time is {:7.2f} ms'.format(average_elapsed_time))


class TestHook:
    """core/hooks/test_hooks.py:13-94: per-scale lists of MSE / PSNR / SSIM over the whole test set (ndown scales for Mip-NeRF's
    multiscale set, 1 otherwise), optionally the rendered PNGs and test_results.json"""
    __test__ = False            # (not a pytest class)

    def __init__(self, ndown=1, save_img=False, dump_json=False, save_folder='test'):
        self.ndown = ndown
        self.dump_json = dump_json
        self.save_img = save_img
        self.save_folder = save_folder

    def before_val_epoch(self, runner):
        self.psnr, self.ssim, self.mse = {}, {}, {}
        for i in range(self.ndown):
            self.psnr[i], self.mse[i], self.ssim[i] = [], [], []

    def after_val_iter(self, runner):
        rgb, gt_img, idx = runner.outputs['rgb'], runner.outputs['gt_img'], runner.outputs['idx']
        if self.save_img:
            testset_dir = os.path.join(runner.work_dir, self.save_folder)
            os.makedirs(testset_dir, exist_ok=True)
            img8 = to8b(rgb)
            _save_png(os.path.join(testset_dir, '{:03d}.png'.format(idx)), img8.cpu().numpy() if isinstance(img8, torch.Tensor) else img8)
        mse, psnr, ssim = _read_back(frame_metrics(rgb, gt_img))
        scale = idx % self.ndown
        self.psnr[scale].append(float(psnr))
        self.mse[scale].append(float(mse))
        self.ssim[scale].append(float(ssim))

    def after_val_epoch(self, runner):
        metrics = 'In test phase on whole testset, \n  '
        for scale in range(self.ndown):
            average_mse = sum(self.mse[scale]) / len(self.mse[scale])
            average_psnr = sum(self.psnr[scale]) / len(self.psnr[scale])
            average_ssim = sum(self.ssim[scale]) / len(self.ssim[scale])
            metrics += f' for scale {scale}, mse is {average_mse}, psnr is {average_psnr}, ssim is {average_ssim}. \n'
        runner.logger.info(metrics)
        if self.dump_json:
            os.makedirs(os.path.join(runner.work_dir, self.save_folder), exist_ok=True)
            with open(os.path.join(runner.work_dir, self.save_folder, 'test_results.json'), 'w') as f:
                json.dump({'results': metrics, 'psnrs': self.psnr, 'ssims': self.ssim}, f)
        if hasattr(runner, '_epoch'):
            runner._epoch += 1          # (the reference's note: a test run is ('val', 1), which mmcv's runner does not count)


# ------------------------------------------------------------------------------------------ val_step + ValidateHook on the device
def evaluate_frames(render, poses, gts, white_bkgd_mask=True):
    """What HashNerfNetwork.val_step and ValidateHook do together, for any callable that returns a device frame: render(pose) -> rgb
    [H,W,3] (or a tuple whose first entry it is, as train.render_frame returns).  With `white_bkgd_mask` a gt of four channels is
    RGBA and both images are multiplied by its alpha (networks/hashnerf.py:78-83).  Every frame is measured where it was rendered,
    its three scalars go into one device buffer, and ONE blocking read ends the set.
    -> {'mse', 'psnr', 'ssim': lists, 'average_mse', 'average_psnr', 'average_ssim': floats, 'log': ValidateHook's line}"""
    n = len(poses)
    if n == 0:
        return {'mse': [], 'psnr': [], 'ssim': [], 'log': None}
    buf = None
    for i in range(n):
        rgb = render(poses[i])
        rgb = rgb[0] if isinstance(rgb, (tuple, list)) else rgb
        gt = _tensor(gts[i]).to(device=rgb.device, dtype=torch.float32)
        if white_bkgd_mask and gt.shape[-1] == 4:
            alpha = gt[..., 3:]
            rgb, gt = rgb * alpha, gt[..., :3] * alpha
        if buf is None:
            buf = torch.empty((n, 3), dtype=torch.float64, device=rgb.device)
        buf[i] = frame_metrics(rgb, gt)
    rows = _read_back(buf)
    out = {'mse': [r[0] for r in rows], 'psnr': [r[1] for r in rows], 'ssim': [r[2] for r in rows]}
    for k in ('mse', 'psnr', 'ssim'):
        out['average_' + k] = sum(out[k]) / n
    out['log'] = 'On testset, mse is {:.5f}, psnr is {:.5f}, ssim is {:.5f}'.format(out['average_mse'], out['average_psnr'], out['average_ssim'])
    return out


# ------------------------------------------------------------------------------------------ the spiral hooks
def imageio_module():
    """imageio where it is installed (a module that can write a clip), else None"""
    try:
        import imageio
    except ImportError:
        return None
    return imageio if hasattr(imageio, 'mimwrite') else None


def write_frames(folder, name, frames8, fps=30):
    """the frames of one clip: PNGs folder/<name>/000.png ..., and folder/<name>.mp4 as the reference writes it (imageio.mimwrite,
    quality 8) only where imageio imports"""
    clip = os.path.join(folder, name)
    os.makedirs(clip, exist_ok=True)
    for i, f in enumerate(frames8):
        _save_png(os.path.join(clip, '{:03d}.png'.format(i)), f if f.ndim == 3 else f[..., None])
    imageio = imageio_module()
    if imageio is None:
        return False
    imageio.mimwrite(clip + '.mp4', frames8, fps=fps, quality=8)
    return True


class SaveSpiralHook:
    """core/hooks/validation_hooks.py:24-51: the spiral frames of a validation, work_dir/save_folder/<iter>_rgb and <iter>_disp
    (to8b(rgb), to8b(disp / max disp))"""

    def __init__(self, save_folder='validation'):
        self.save_folder = save_folder

    def after_val_iter(self, runner):
        cur_iter = runner.iter
        spiral_rgbs = np.stack(runner.outputs['spiral_rgbs'], 0)
        spiral_disps = np.stack(runner.outputs['spiral_disps'], 0)
        spiral_dir = os.path.join(runner.work_dir, self.save_folder)
        os.makedirs(spiral_dir, exist_ok=True)
        write_frames(spiral_dir, '{}_rgb'.format(cur_iter), to8b(spiral_rgbs), fps=30)
        write_frames(spiral_dir, '{}_disp'.format(cur_iter), to8b(spiral_disps / np.max(spiral_disps)), fps=30)


class NBSaveSpiralHook:
    """core/hooks/validation_hooks.py:54-92: the first frame of every test item, collected over the epoch, as work_dir/save_folder/rgb
    and disp; the epoch counter moves on here (a ('val', 1) workflow never advances it)"""

    def __init__(self, save_folder='validation'):
        self.save_folder = save_folder
        self.rgbs, self.disps = [], []

    def after_val_iter(self, runner):
        self.rgbs.append(runner.outputs['rgbs'][0])
        self.disps.append(runner.outputs['disps'][0])

    def after_val_epoch(self, runner):
        spiral_dir = os.path.join(runner.work_dir, self.save_folder)
        os.makedirs(spiral_dir, exist_ok=True)
        spiral_rgbs, spiral_disps = np.array(self.rgbs), np.array(self.disps)
        write_frames(spiral_dir, 'rgb', to8b(spiral_rgbs), fps=30)
        write_frames(spiral_dir, 'disp', to8b(spiral_disps / np.max(spiral_disps)), fps=30)
        runner._epoch += 1


class HashSaveSpiralHook:
    """core/hooks/hash_hook.py:45-103: the instant-ngp test frames sorted by idx, white where alpha < 0.99, as
    work_dir/save_folder/<prefix>_rgb and <prefix>_alpha (prefix: the checkpoint's iteration, or 'latest')"""

    def __init__(self, save_folder='validation', cfg=None):
        self.save_folder = save_folder
        self.prefix = cfg.load_from.split('/')[-1].split('.')[-2].replace('iter_', '')
        self.prefix = 'latest' if len(self.prefix) == 0 else self.prefix

    def before_val_epoch(self, runner):
        self.spiral_data = []

    def after_val_iter(self, runner):
        self.spiral_data.append([runner.outputs['idx'], runner.outputs['spiral_rgb'], runner.outputs['spiral_alpha']])

    def after_val_epoch(self, runner):
        spiral_dir = os.path.join(runner.work_dir, self.save_folder)
        os.makedirs(spiral_dir, exist_ok=True)
        self.spiral_data = self.apply_mask(sorted(self.spiral_data, key=lambda x: x[0]))
        write_frames(spiral_dir, '{}_rgb'.format(self.prefix), to8b(np.stack([x[1] for x in self.spiral_data], 0)), fps=25)
        write_frames(spiral_dir, '{}_alpha'.format(self.prefix), to8b(np.stack([x[2] for x in self.spiral_data], 0)), fps=25)
        runner._epoch += 1

    def apply_mask(self, spiral_data):
        for i in range(len(spiral_data)):
            alpha, rgb = spiral_data[i][2], spiral_data[i][1]
            mask = (alpha >= 0.99).astype(np.float64)
            spiral_data[i][1] = rgb * mask + 1 * (1 - mask)
        return spiral_data
