"""The list optimiser kernel and the log window of xrnerf_amd/csrc/xr_optim.hip -- the SAME source the GPU library is built from -- compiled
for the host and run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/optim_cases.py at the first three tensor
counts.  Both builds use -ffp-contract=off, so the bits seen here are the bits the MI355X produces.  Plus what needs no kernel: the
header, the ctypes table and the library agree, and FusedAdam.step keeps its launches of up to four tensors where the list kernel is
not there."""
import contextlib
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import optim_cases as K  # noqa: E402


def emulated_optim():
    """emulib.emulated_ops with the host build of xr_optim and its table on top"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_optim',))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.OPTIM_SIGNATURES.items()):
                try:
                    fn = getattr(ml, name)
                except AttributeError:
                    continue
                fn.restype, fn.argtypes = res, args
            _lib._lib = ml

            def check(rc, what=''):
                if rc != 0:
                    raise _lib.XrError('%s failed (%d): %s' % (what, rc, ml.last_errors()))
            _lib.check = check
            from xrnerf_amd import ops
            assert ops.optim_kernels_available(), 'the host build has no xr_optim entry point'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_optim() as dev:
        yield dev


def test_header_table_and_library_agree():
    from xrnerf_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_optim.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    names = sorted(set(re.findall(r'\b(xr_[a-z0-9_]+)\s*\(', src)))
    assert names == sorted(_lib.OPTIM_SIGNATURES) and len(names) == 3
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), 'missing export %s' % n
    assert not set(names) & set(_lib.SIGNATURES)
    cap = lib.xr_adam_list_capacity()
    assert cap >= 50 and 'XR_ADAM_LIST_CAPACITY %du' % cap in src                 # a NerfNetwork (coarse + fine: 48 tensors) is one launch
    # the by-value work list stays under HIP's 4-KiB argument block: 5 pointers, a length and a prefix entry per tensor, the mask, the constants
    assert cap * (5 * 8 + 4 + 4) + 4 + cap // 8 + 64 <= 4096
    # an invalid call fails with a message and launches nothing
    assert lib.xr_adam_step_list(0, None, None, None, None, None, None, 1, 0.1, 0.9, 0.99, 1e-8, 0.0, 0.0, 1.0, None) == -22
    assert b'xr_adam_step_list' in lib.xr_last_error()


@pytest.mark.parametrize('grad_scale', (1.0, 0.125))
@pytest.mark.parametrize('with_ema', (False, True))
@pytest.mark.parametrize('n_tensors', (1, 4, 5))
def test_list_kernel_against_adam_step_multi(edev, n_tensors, with_ema, grad_scale):
    assert n_tensors in K.counts()[:3]
    K.check_fused_adam(edev, n_tensors, with_ema, grad_scale)


@pytest.mark.parametrize('which', ('p', 'g', 'm', 'v', 'ema'))
def test_one_unaligned_buffer(edev, which):
    K.check_unaligned_each(edev, which)


def test_every_length_alone(edev):
    K.check_single_lengths(edev)


def test_refusals(edev):
    K.check_refusals(edev)


def test_log_window(edev):
    K.check_log_window(edev)


def test_step_without_the_list_kernel_keeps_the_launches_of_four():
    """a library handle without xr_adam_step_list (the emulator's stock set of sources): FusedAdam.step goes through xr_adam_step_multi,
    and the list kernel, where present, leaves the same bits"""
    import emulib as E
    from xrnerf_amd import ops
    from xrnerf_amd.train import FusedAdam

    def run(dev):
        ps = [torch.nn.Parameter(K._values(n, 10 + i, dev)) for i, n in enumerate((5, 255, 1025, 3, 4, 1))]
        opt = FusedAdam(ps, lr=1e-2, ema_momentum=0.05)
        for it in range(2):
            for i, p in enumerate(ps):
                p.grad = K._values(p.numel(), 100 + 10 * it + i, dev)
            opt.step()
        return [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps for k in ('m', 'v', 'ema')]

    with E.emulated_ops() as dev:
        assert not ops.optim_kernels_available()
        old = run(dev)
    with emulated_optim() as dev:
        new = run(dev)
    assert all(K.same_bits(a, b) for a, b in zip(old, new))


def test_log_window_host_values_need_no_library():
    from xrnerf_amd.runner import LogWindow
    w = LogWindow()
    w.update({'loss': 0.5, 'psnr': torch.tensor(20.0)}, 4)
    w.update({'loss': 1.5, 'psnr': torch.tensor(10.0)}, 12)
    assert w.read() == {'loss': (0.5 * 4 + 1.5 * 12) / 16, 'psnr': (20.0 * 4 + 10.0 * 12) / 16} and w.read() == {}
