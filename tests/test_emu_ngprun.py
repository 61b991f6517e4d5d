"""xr_ngp_log_add of xrnerf_amd/csrc/xr_ngprun.hip -- the SAME source the GPU library is built from -- compiled for the host and run lane by
lane by the HIP-on-CPU shim (tests/hip_emu), against numpy float64.  Both builds use -ffp-contract=off."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, ROOT)

SLOTS = 16
U = 2.0 ** -53                      # unit roundoff of float64


@pytest.fixture(scope='module')
def lib():
    import emulib as E
    from xrnerf_amd import _lib
    L = E.lib('xr_ngprun')
    res, args = _lib.NGPRUN_SIGNATURES['xr_ngp_log_add']
    L.xr_ngp_log_add.restype, L.xr_ngp_log_add.argtypes = res, args
    L.xr_last_error.restype = C.c_char_p
    return L


def add(L, lm, n, w, a, b):
    return L.xr_ngp_log_add(lm.ctypes.data_as(C.c_void_p) if lm is not None else None, n, w.ctypes.data_as(C.c_void_p) if w is not None else None,
                            a, b, None)


CALLS = [  # (loss, squared-error sum, n_rays): mse = sum / (3 n) from 2.4e-4 to 2.7, the three n_rays the issue names
    (0.73519, 3.0e-3 * 3 * 4096, 4096), (1.0e-3, 0.8, 1), (41.25, 2.4e-4 * 3 * (2 ** 29 - 1), 2 ** 29 - 1), (0.1234567, 2.7 * 3 * 4096, 4096),
    (7.0, 8.1, 1)]


def test_five_calls_into_two_non_adjacent_slots_against_numpy_float64(lib):
    s_loss, s_psnr = 3, 9
    rng = np.random.default_rng(5)
    w = rng.uniform(-4, 4, 2 * SLOTS)                           # every slot starts from a value of its own
    start = w.copy()
    ref_loss, ref_psnr, ref_n = start[s_loss], start[s_psnr], [start[SLOTS + s_loss], start[SLOTS + s_psnr]]
    bound = 0.0
    for loss, sq, n in CALLS:
        lm = np.array([loss, sq], np.float32)
        assert add(lib, lm, n, w, s_loss, s_psnr) == 0, lib.xr_last_error()
        nd = np.float64(n)
        ref_loss = ref_loss + np.float64(lm[0]) * nd           # the product is exact (24 + 29 bits); the sum rounds as the kernel's does
        p = np.float64(-10.0) * np.log10(np.float64(lm[1]) / (np.float64(3.0) * nd))
        ref_psnr = ref_psnr + p * nd
        ref_n = [ref_n[0] + nd, ref_n[1] + nd]
        # The psnr slot's bound.  x = sum / (3 n) is one IEEE division of the same operands on both sides (3 n is exact): no difference,
        # counted as one rounding (0.4343 u in log10) all the same.  log10: at most 3 ulp on the device (the OpenCL bound ocml's double
        # log10 is built to) + 1 ulp in numpy's libm = 4 ulp(L) <= 8 u |L|, times 10; the product by -10 rounds once on each side
        # (<= 2 u |p|); the product by n once on each side (<= 2 u |p| n); each side adds into its sum once (<= u |S| each).
        bound += nd * U * (4.35 + 10.0 * abs(p)) + 2.0 * U * abs(p) * nd + 2.0 * U * abs(ref_psnr)
        assert w[s_loss] == ref_loss and w[SLOTS + s_loss] == ref_n[0] and w[SLOTS + s_psnr] == ref_n[1]
        assert abs(w[s_psnr] - ref_psnr) <= bound, (w[s_psnr], ref_psnr, bound)
    print('psnr slot: %.17g against %.17g, difference %.3g, bound %.3g' % (w[s_psnr], ref_psnr, abs(w[s_psnr] - ref_psnr), bound))
    assert bound < 1e-12 * abs(ref_psnr)                        # (the bound itself is tight: a wrong weight or a float log10 is far outside)
    assert w[SLOTS + s_loss] == start[SLOTS + s_loss] + (4096 + 1 + 2 ** 29 - 1 + 4096 + 1)
    untouched = [i for i in range(2 * SLOTS) if i not in (s_loss, s_psnr, SLOTS + s_loss, SLOTS + s_psnr)]
    assert np.array_equal(w[untouched], start[untouched])
    # LogWindow.read's value of the two slots: the weighted averages
    w2 = np.zeros(2 * SLOTS)
    for loss, sq, n in CALLS[:2]:
        assert add(lib, np.array([loss, sq], np.float32), n, w2, 15, 0) == 0          # (the psnr slot below the loss slot, at the window's ends)
    l0, l1 = np.float64(np.float32(CALLS[0][0])), np.float64(np.float32(CALLS[1][0]))
    assert w2[15] / w2[SLOTS + 15] == (l0 * 4096 + l1 * 1) / 4097.0
    assert abs(w2[0] / w2[SLOTS] - (-10 * np.log10(3.0e-3) * 4096 - 10 * np.log10(0.8 / 3)) / 4097.0) < 1e-5      # (fp32 inputs: a sanity figure)


def test_refusals_launch_nothing(lib):
    w = np.arange(2 * SLOTS, dtype=np.float64)
    before = w.copy()
    lm = np.array([1.0, 2.0, 3.0], np.float32)
    raw = np.zeros(2 * SLOTS * 8 + 8, np.uint8)
    off = (-raw.ctypes.data) % 8
    odd = raw[off + 4:off + 4 + 2 * SLOTS * 8].view(np.float64)             # 4 bytes off an 8-byte boundary
    bad = [(None, 4096, w, 0, 1, 'null'), (lm, 4096, None, 0, 1, 'null'), (lm, 4096, w, 5, 5, 'slots'), (lm, 4096, w, SLOTS, 1, 'slots'),
           (lm, 4096, w, 1, SLOTS, 'slots'), (lm, 4096, w, 0xffffffff, 1, 'slots'), (lm, 0, w, 0, 1, 'n_rays'), (lm, 2 ** 29, w, 0, 1, 'n_rays'),
           (lm, 0xffffffff, w, 0, 1, 'n_rays'), (lm, 4096, odd, 0, 1, 'aligned')]
    for lm_, n, w_, a, b, word in bad:
        assert add(lib, lm_, n, w_, a, b) == -22, (n, a, b)
        assert word.encode() in lib.xr_last_error(), (word, lib.xr_last_error())
    assert lib.xr_ngp_log_add(C.c_void_p(lm.ctypes.data + 2), 4096, w.ctypes.data_as(C.c_void_p), 0, 1, None) == -22
    assert np.array_equal(w, before) and not odd.any()
    # the largest n_rays that is taken
    assert add(lib, lm, 2 ** 29 - 1, w, 0, 1) == 0 and w[SLOTS] == before[SLOTS] + (2 ** 29 - 1)
