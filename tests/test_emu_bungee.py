"""The BungeeNeRF kernels of xrnerf_amd/csrc/xr_bungee.hip -- the SAME source the GPU library is built from -- compiled for the host
and run lane by lane by the HIP-on-CPU shim (tests/hip_emu), against the reference fixture (tests/golden/ref_bungee.npz) and the
float64 restatement (tests/bungee_restatement.py): ragged ray counts, S < 64, S = 64 (one sweep) and S > 64.  The fixture checks are
the bodies of tests/test_gpu_bungee.py, run through the emulated ops, including the whole network's train_step and stage loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def E():
    import emulib
    return emulib


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_bungee.npz'))


@pytest.fixture(scope='module')
def edev(E):
    """emulib.emulated_ops with xr_bungee's host build added to the library handle"""
    from xrnerf_amd import _lib
    ctx = E.emulated_ops()
    dev = ctx.__enter__()
    ml = E.MultiLib(E.ALL_SOURCES + ('xr_bungee',))
    for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.BUNGEE_SIGNATURES.items()):
        try:
            fn = getattr(ml, name)
        except AttributeError:
            continue
        fn.restype, fn.argtypes = res, args
    _lib._lib = ml
    yield dev
    ctx.__exit__(None, None, None)


def test_fixture_zvals_encode_render_resample(edev, gold):
    import test_gpu_bungee as T
    T.check_zvals(edev, gold)
    T.check_encode(edev, gold)
    T.check_render(edev, gold)
    T.check_resample(edev, gold)


def test_fixture_network_train_step_and_stage_loop(edev, gold):
    import test_gpu_bungee as T
    T.check_network(edev, gold)
    T.check_stage_loop(edev, gold)


@pytest.mark.parametrize('R,S', [(5, 7), (3, 64), (9, 100), (1, 1), (66, 16)])
def test_kernels_against_restatement(E, edev, R, S):
    import bungee_restatement as RS
    import test_gpu_bungee as T
    L = E.lib('xr_bungee')
    for name, (res, args) in __import__('xrnerf_amd._lib', fromlist=['x']).BUNGEE_SIGNATURES.items():
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    sc = T.restatement_rays(R, S)
    s = T.SCALE
    o, d, vd, radii = sc['o'], sc['d'], sc['vd'], sc['radii']
    near, far = np.zeros(R, np.float32), np.zeros(R, np.float32)
    z = np.zeros((R, S + 1), np.float32)
    gc = (C.c_float * 3)(0., 0., -6371011.0 * s)
    E.check(L.xr_bungee_zvals(E.p(o), E.p(vd), E.p(near), E.p(far), R, S + 1, 1, C.cast(gc, C.c_void_p),
                              ((6371011.0 + 250) * s) ** 2, (6371011.0 * s) ** 2, s, E.p(z), None), L)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    n64, f64 = RS.bounds(t(o), t(vd), 'sphere', (0., 0., -6371011.0), s)
    assert np.abs(near - n64.numpy()[:, 0]).max() <= 5e-3 * np.abs(n64.numpy()).max()
    z64 = RS.zvals(t(near)[:, None], t(far)[:, None], S + 1).numpy()
    assert np.abs(z - z64).max() <= 1e-6 * np.abs(z64).max()
    cp, cd = 63, 27
    out = E.aligned((R * S, 96))
    E.check(L.xr_bungee_encode(E.p(o), E.p(d), E.p(radii), E.p(z), None, None, E.p(vd), R, S, 10, 4, 0, E.p(out), 96,
                               C.c_void_p(out.ctypes.data + 4 * cp), 96, None), L)
    means, covs = RS.gaussians(t(z), t(o), t(d), t(radii))
    e64 = RS.embed(means, covs, t(vd)).numpy()
    assert np.abs(out[:, :cp + cd] - e64).max() <= 1e-3            # arguments up to 512 |x| ~ 4e3: fp32 rounding of the mean
    T.check_render_restatement(edev, R, S)          # the renderer: the body of the GPU test, through the emulated ops
