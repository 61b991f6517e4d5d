"""tests/test_gpu_backward_f64.py's bodies on the host build of the kernels (tests/hip_emu), at sizes the emulation finishes in
seconds: the MLP backward in every arithmetic, deeper topologies on both paths, live lists, device-side counts and row ranges
against float64; the table scatter in child processes with its row threshold lowered (XR_SC_TEST=min_n=256 is read once per
process), below and above the threshold, on every position layout.  The emulator's MFMA adds in another order than the matrix
cores, so these runs check the tests' mechanics and the kernels' logic; the bars are set by the GPU run."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


@pytest.fixture(scope='module')
def edev():
    import emulib
    ctx = emulib.emulated_ops()
    dev = ctx.__enter__()
    yield dev
    ctx.__exit__(None, None, None)


@pytest.mark.parametrize('arith', ['f32', 'b2', 'b2x', 'b2f', 'h2f'])
def test_mlp_backward_against_float64_on_the_host(edev, arith, monkeypatch):
    import test_gpu_backward_f64 as G
    monkeypatch.setenv('XR_MLP_BWD_DW', arith)
    for n in (1, 31, 33, 257):
        G.mlp_case(edev, n, arith, seed=n)
    G.mlp_case(edev, 1100, arith, n_valid=1030, seed=11)


@pytest.mark.parametrize('path', ['streamed', 'layered'])
def test_mlp_topologies_against_float64_on_the_host(edev, path, monkeypatch):
    import test_gpu_backward_f64 as G
    from xrnerf_amd import ops
    monkeypatch.delenv('XR_MLP_BWD_DW', raising=False)
    if path == 'layered':
        monkeypatch.setattr(ops, '_FUSED_FWD', ())
        monkeypatch.setattr(ops, '_FUSED_BWD', ())
    for nhd, nhc in ((1, 2), (1, 1), (2, 1), (3, 4), (5, 5), (8, 8)):
        G.mlp_case(edev, 65, G.topo_arith(nhd, nhc, path), nhd, nhc, seed=nhd * 10 + nhc)
    G.mlp_case(edev, 300, G.topo_arith(5, 5, path), 5, 5, n_valid=270, seed=3)


def test_mlp_backward_live_rows_and_row_ranges_on_the_host(edev, monkeypatch):
    import numpy as np
    import grad_bars as B
    import test_gpu_backward_f64 as G
    monkeypatch.delenv('XR_MLP_BWD_DW', raising=False)
    n = 2100
    for layout, dead in G.live_layouts(n, np.random.default_rng(3)).items():
        for live in (False, True):
            G.mlp_case(edev, n, B.mode(), dead=dead, live=live, seed=33, check_raw=False)
    G.mlp_case(edev, n, B.mode(), dead=G.live_layouts(n, np.random.default_rng(4))['half'], live=True, n_valid=1500, seed=34)
    for row0, count in ((0, 33), (1000, 100), (2047, 1)):
        G.mlp_case(edev, n, B.mode(), row0=row0, count=count, seed=row0 + count)


def run_case(*args):
    e = dict(os.environ, XR_SC_TEST='min_n=256')
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], env=e, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize('layout', ['uniform', 'rays', 'cluster', 'faces'])
def test_scatter_against_float64_on_the_host(layout):
    """255 rows: the atomic kernel; 256, 257, 3000: binned, run-length and overflow paths (min_n lowered to 256); the variants at 3000"""
    out = run_case(layout, 255, 256, 257, 3000)
    assert out.count('ok') == 5, out


def main(layout, sizes):
    import emulib
    import oracle as O
    import test_gpu_backward_f64 as G
    with emulib.emulated_ops() as dev:
        for n in sizes:
            G.scatter_case(O, dev, n, layout)
            print('scatter %s n=%d ok' % (layout, n))
        G.scatter_variants(O, dev, sizes[-1], layout)
        print('variants %s n=%d ok' % (layout, sizes[-1]))
    return 0


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    sys.exit(main(sys.argv[1], [int(a) for a in sys.argv[2:]]))
