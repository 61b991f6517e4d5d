"""The ray front end of xrnerf_amd/csrc/xr_pipeline.hip -- the SAME source the GPU library is built from -- compiled for the host and run
lane by lane by the HIP-on-CPU shim (tests/hip_emu): the bodies of tests/pipeline_cases.py through the emulated ops.  Both builds use
-ffp-contract=off, so the bits seen here are the bits the MI355X produces."""
import contextlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pipeline_cases as K  # noqa: E402
from xrnerf_amd import pipelines  # noqa: E402,F401  (every check here is about this module)


def emulated_pipeline():
    """emulib.emulated_ops with the host build of xr_pipeline and its table on top"""
    import emulib as E
    from xrnerf_amd import _lib

    @contextlib.contextmanager
    def cm():
        with E.emulated_ops() as dev:
            ml = E.MultiLib(E.ALL_SOURCES + ('xr_pipeline',))
            for name, (res, args) in list(_lib.SIGNATURES.items()) + list(_lib.PIPELINE_SIGNATURES.items()):
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
            assert ops.pipeline_kernels_available(), 'the host build has no xr_pipeline entry points'
            yield dev
    return cm()


@pytest.fixture(scope='module')
def edev():
    with emulated_pipeline() as dev:
        yield dev


@pytest.mark.parametrize('name', K.CASE_NAMES)
def test_fixture_cases_through_the_kernel(edev, name):
    K.check_fixture_kernel(edev, name)


@pytest.mark.parametrize('name', K.CASE_NAMES)
def test_fixture_cases_through_compose(edev, name):
    K.check_fixture_compose(edev, name)


@pytest.mark.parametrize('name', K.CASE_NAMES)
def test_fused_compose_equals_the_transforms_one_by_one(edev, name):
    K.check_fused_against_stepwise(edev, name)


def test_pieces_of_a_frame_concatenate_to_the_frame(edev):
    K.check_pieces(edev)


def test_nullable_outputs(edev):
    K.check_nullable_outputs(edev)


def test_refusals_and_empty_launch_nothing(edev):
    K.check_refusals_and_empty(edev)


def test_default_draws(edev):
    K.check_default_draws(edev)


def test_a_foreign_callable_inside_the_run_is_not_fused(edev):
    K.check_foreign_callable_is_not_fused(edev)


def test_header_table_and_host_build_agree(edev):
    K.check_symbols()
