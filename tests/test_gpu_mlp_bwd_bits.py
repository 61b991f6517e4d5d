"""The fused MLP backward (k_nerf_mlp_bwd_1_2) computes the same BITS as the build the digests were recorded from: every arithmetic
whose dW runs on the bf16 matrix cores (XR_MLP_BWD_DW = b2, b2x, b2f, h2f) at 33, 1025, 40001 and 2^18 (230 000 valid) rows, over
all rows and with a live list; sha256 of the float32 bytes of dWd, dWc and dL/d(encoding) against tests/golden/mlp_bwd_digests.json.
The golden file names the commit whose binary produced it (tools/mlp_bwd_ab.py --record): it is never recorded from the code under
test.  A change that re-orders a sum on purpose has to show its error against float64 (tests/test_gpu_backward_f64.py) beside the
old one and record anew; anything else that fails here lost or moved an operand."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

pytestmark = pytest.mark.gpu


def test_mlp_backward_is_the_recorded_bits(dev):
    import mlp_bwd_ab as AB
    with open(AB.GOLDEN) as f:
        golden = json.load(f)
    want = golden['cases']
    assert len(want) == len(AB.MODES) * len(AB.GPU_SIZES) * 2, 'the golden file does not hold every case'
    got = AB.digests(dev)
    assert sorted(got) == sorted(want)
    diff = ['%s: %s' % (k, x) for k in sorted(want) for x in ('dwd', 'dwc', 'denc') if got[k][x] != want[k][x]]
    assert not diff, '%d arrays differ from %s:\n%s' % (len(diff), golden['recorded_with'], '\n'.join(diff))
