"""Generates tests/golden/ref_eval.npz, the fixture of the evaluation tests:  python tests/golden/make_golden_eval.py

Needs numpy and scipy only.  The image pairs are generated (tests/eval_cases.py: gt U(0,1) with one half exactly 1.0, rgb = gt + 0.05
N(0,1), fp32).  Stored per case: the inputs; the SSIM map and per-image mean of skimage's documented algorithm composed from
scipy.ndimage.uniform_filter / gaussian_filter in float64 (the very calls skimage makes -- skimage itself is not installed where this
runs, so equality with skimage is unverified); the map and mean of tests/eval_restatement.py's direct sum in np.longdouble, rounded to
double (the truth); numpy's fp32 img2mse and the float64 one; to8b(hstack(rgb, gt)).  All with data_range = 2.0, the hooks' reading
(evaluate.REFERENCE_SSIM_DATA_RANGE).

The maker asserts that long double is wider than double here, that every mean lies in (0.5, 1) and that the float64 maps differ from the
long-double one.  It prints, per case, the distances of the two float64 witnesses from the truth -- the figures the tests' bars are made
of -- and one frame under both readings of the hooks' data range."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import eval_cases as K  # noqa: E402
import eval_restatement as RS  # noqa: E402


def main():
    assert np.finfo(np.longdouble).nmant >= 63, 'np.longdouble is no wider than double on this machine'
    out = {}
    for name, B, H, W, C, gauss in K.CASES:
        rgb, gt = K.generate(name)
        truth = np.stack([RS.ssim_map(rgb[b], gt[b], 7, gauss, K.DATA_RANGE, np.longdouble) for b in range(B)])
        scipy64 = np.stack([RS.scipy_ssim_map(rgb[b], gt[b], 7, gauss, K.DATA_RANGE) for b in range(B)])
        direct64 = np.stack([RS.ssim_map(rgb[b], gt[b], 7, gauss, K.DATA_RANGE, np.float64) for b in range(B)])
        mean_truth = truth.reshape(B, -1).mean(1)
        assert truth.dtype == np.longdouble and scipy64.dtype == np.float64 and direct64.dtype == np.float64
        assert ((mean_truth > 0.5) & (mean_truth < 1)).all(), (name, mean_truth)
        assert (scipy64 != truth).any() and (direct64 != truth).any(), name
        e_s, e_d = float(np.abs(scipy64 - truth).max()), float(np.abs(direct64 - truth).max())
        m_s = float(np.abs(scipy64.reshape(B, -1).mean(1) - mean_truth).max())
        m_d = float(np.abs(direct64.reshape(B, -1).mean(1) - mean_truth).max())
        mse32 = np.array([RS.img2mse32(rgb[b], gt[b]) for b in range(B)], np.float32)
        mse64 = np.array([RS.img2mse64(rgb[b], gt[b]) for b in range(B)], np.float64)
        print('%-8s B %d %3d x %3d x %d %s  map: scipy64 %.3e direct64 %.3e (bar %.3e)  mean: scipy64 %.3e direct64 %.3e floor %.3e  ssim %.6f  mse %.6e |ref32-ref64| %.3e'
              % (name, B, H, W, C, 'gauss  ' if gauss else 'uniform', e_s, e_d, 4 * max(e_s, e_d), m_s, m_d, H * W * C * 2.0 ** -53, float(mean_truth[0]),
                 mse64[0], float(np.abs(mse32.astype(np.float64) - mse64).max())))
        out[name + '.rgb'], out[name + '.gt'] = rgb, gt
        out[name + '.map_scipy64'], out[name + '.mean_scipy64'] = scipy64, scipy64.reshape(B, -1).mean(1)
        out[name + '.map_truth'], out[name + '.mean_truth'] = truth.astype(np.float64), mean_truth.astype(np.float64)
        out[name + '.mse32'], out[name + '.mse64'] = mse32, mse64
        out[name + '.to8b'] = np.stack([RS.to8b(np.hstack((rgb[b], gt[b]))) for b in range(B)])
    # the hooks' data range, both readings, on one frame
    rgb, gt = out['37x70.rgb'][0], out['37x70.gt'][0]
    for what, R in (('data_range = 2 (what skimage is remembered to use)', 2.0), ('data_range = gt.max() - gt.min() (what the caller meant)', float(gt.max() - gt.min()))):
        print('37x70 %-58s R %.6f  ssim %.6f' % (what, R, float(RS.ssim_map(rgb, gt, 7, False, R, np.longdouble).mean())))
    path = os.path.join(HERE, 'ref_eval.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
