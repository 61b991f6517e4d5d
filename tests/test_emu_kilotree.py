"""The validation-table kernel of xrnerf_amd/csrc/xr_kilotree.hip -- the SAME source the GPU library is built from -- compiled for the host
and run lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/kilotree_cases.py at the small shapes.  Both builds use
-ffp-contract=off, so the bits seen here are the bits the MI355X produces."""
import contextlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import kilotree_cases as K  # noqa: E402


def emulated_kilotree():
    """emulib.emulated_ops with the host build of xr_kilotree and its table on top"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_kilotree',))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.KILOTREE_SIGNATURES.items()):
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
            assert ops.kilotree_kernels_available(), 'the host build has no xr_kilotree entry point'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_kilotree() as dev:
        yield dev


@pytest.mark.parametrize('P', K.SMALL_P[:5] + (257,))
@pytest.mark.parametrize('N', (1, 5))
def test_small_shapes_against_the_restatement(edev, N, P):
    K.check_shape(edev, N, P)


def test_crafted_saturation_rows(edev):
    K.check_saturation(edev)


def test_tied_coordinates_and_tied_errors(edev):
    K.check_ties(edev)


def test_odd_values(edev):
    K.check_odd_values(edev)


def test_two_runs_and_permuted_points_give_the_same_bits(edev):
    K.check_repeat_and_permutation(edev)


def test_refusals(edev):
    K.check_refusals(edev)


# the discovery loop end to end on the host build (the bodies of tests/test_gpu_kilo_tree.py): datasets, fused student step, hooks, runner
def test_three_cycles_grow_the_longest_axis_tree(edev, tmp_path):
    import test_gpu_kilo_tree as G
    G.check_longest_axis_tree(edev, str(tmp_path))


def test_equal_error_split_threshold_is_the_kernels(edev, tmp_path):
    import test_gpu_kilo_tree as G
    G.check_equal_error_threshold(edev, str(tmp_path))


def test_max_error_of_the_shipped_configs_keeps_the_fixed_forest(edev, tmp_path):
    import test_gpu_kilo_tree as G
    G.check_fixed_forest(edev, str(tmp_path))
