"""The KiloNeRF tiny-MLP kernels on the MI355X against the float64 reference (tests/ref64_kilo.py), network by network and entry by entry:
the bodies of tests/kilo_f64_cases.py at the full set of per-network sample counts, batch sizes and architectures.  Every number is held
to its own derived bound; KILO_F64_LOG=<file> records the worst error / bound of every tensor (profiles/kilo_f64_gpu_tests.txt)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kilo_f64_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('arch', K.ARCH_FWD, ids=lambda a: '%d-%d-%d' % a)
def test_forward_every_row_within_its_bound(dev, arch):
    K.check_forward(dev, arch)


def test_forward_with_an_occupancy_voxel_switched_off(dev):
    K.check_forward(dev, (10, 4, 2), occupancy=True)


@pytest.mark.parametrize('arch', K.ARCH_BWD, ids=lambda a: '%d-%d-%d' % a)
def test_backward_every_entry_within_its_bound(dev, arch):
    K.check_backward(dev, arch)


def test_gradient_kernels_refuse_larger_architectures(dev):
    K.check_refusals(dev)


@pytest.mark.parametrize('arch', K.ARCH_BWD, ids=lambda a: '%d-%d-%d' % a)
def test_student_step_forward_and_adam(dev, arch):
    K.check_student_arch(dev, arch)


def test_mutated_references_fall_outside_the_bars(dev):
    K.check_mutations(dev)
