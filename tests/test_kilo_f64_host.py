"""The float64 checks of the KiloNeRF tiny-MLP kernels (tests/kilo_f64_cases.py) on the host build of xrnerf_amd/csrc/xr_kilo.hip -- the SAME
source the GPU library is built from, run lane by lane by the HIP-on-CPU shim (tests/hip_emu) with v_mfma_f32_32x32x2_f32 emulated as the
fp32 fused-multiply-add chain it is.  Cut to what the emulator does in tens of seconds: the architectures (5, 3, 2) (P = 33: the one-row
second tile, odd frequency counts on both sides) and (10, 4, 2), per-network counts 0, 1, 33, 129 and batches 33, 129.  The full sets run on
the MI355X (tests/test_gpu_kilo_f64.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import kilo_f64_cases as K  # noqa: E402

ARCHS = ((5, 3, 2), (10, 4, 2))


@pytest.fixture(scope='module')
def edev():
    import emulib as E
    with E.emulated_ops() as dev:
        yield dev


@pytest.mark.parametrize('arch', ARCHS, ids=lambda a: '%d-%d-%d' % a)
def test_forward_every_row_within_its_bound(edev, arch):
    K.check_forward(edev, arch, counts=K.COUNTS_HOST)


def test_forward_with_an_occupancy_voxel_switched_off(edev):
    K.check_forward(edev, (10, 4, 2), counts=K.COUNTS_HOST, occupancy=True)


@pytest.mark.parametrize('arch', ARCHS, ids=lambda a: '%d-%d-%d' % a)
def test_backward_every_entry_within_its_bound(edev, arch):
    K.check_backward(edev, arch, counts=K.COUNTS_HOST)


def test_gradient_kernels_refuse_larger_architectures(edev):
    K.check_refusals(edev)


@pytest.mark.parametrize('arch', ARCHS, ids=lambda a: '%d-%d-%d' % a)
def test_student_step_forward_and_adam(edev, arch):
    K.check_student_arch(edev, arch, batches=K.BATCHES_HOST, combos=((1, 6), (3, 10)))


def test_mutated_references_fall_outside_the_bars(edev):
    K.check_mutations(edev, counts=K.COUNTS_HOST, batch2=129, fwd_archs=((10, 4, 2),))


def test_reference_adjoint_is_the_gradient_of_its_forward():
    """the float64 reference checks itself: central differences of sum(raw * draw) through ref64_kilo.forward against ref64_kilo.backward"""
    import numpy as np
    import ref64_kilo as R
    arch = (5, 3, 2)
    mn = K.make_network(arch, 1, 8)
    rng = np.random.default_rng(0)
    x, v = rng.uniform(-1, 1, (9, 3)).astype(np.float32), rng.normal(0, 1, (9, 3)).astype(np.float32)
    draw = rng.normal(0, 1, (9, 4))
    ts = [p.detach().numpy().astype(np.float64) for p in mn.ordered_parameters()]
    g, _ = R.backward(R.Net(ts, 0), R.forward(R.Net(ts, 0), x, v), draw)
    for k, t in enumerate(ts):
        flat = t[0].reshape(-1)
        for j in rng.choice(flat.size, min(6, flat.size), replace=False):
            old, h = flat[j], 1e-6
            flat[j] = old + h; up = (R.forward(R.Net(ts, 0), x, v)['raw'] * draw).sum()
            flat[j] = old - h; dn = (R.forward(R.Net(ts, 0), x, v)['raw'] * draw).sum()
            flat[j] = old
            assert abs((up - dn) / (2 * h) - g[k].reshape(-1)[j]) <= 1e-6 * max(1.0, abs(g[k].reshape(-1)[j])), (k, j)
