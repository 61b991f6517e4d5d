"""Bit-identity A/B of the fused MLP backward (xr_nerf_mlp_bwd, k_nerf_mlp_bwd_1_2) between two builds of the library.

    python tools/mlp_bwd_ab.py LIB_A LIB_B            both libraries on the GPU, seeded inputs, outputs compared byte for byte
    python tools/mlp_bwd_ab.py --emu LIB_A LIB_B      the same with two HOST builds of xr_mlp.hip (tests/hip_emu/_build/libemu_xr_mlp.so
                                                      of two source trees), small sizes: the emulated MFMA adds in a fixed k order, so a
                                                      lost or swapped operand part shows without a GPU
    python tools/mlp_bwd_ab.py --record LIB --commit C   writes tests/golden/mlp_bwd_digests.json from LIB (the build of commit C)

One fresh child process per library (XRNERF_LIB is read when xrnerf_amd is imported).  Per case -- arithmetic (XR_MLP_BWD_DW) x rows
x {all rows, live list} -- the sha256 of the float32 bytes of dWd, dWc and dL/d(encoding).  No tolerance: the builds are expected
to form the same sums in the same order.  tests/test_gpu_mlp_bwd_bits.py compares the loaded library with the recorded digests."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mlp_bwd_digests.json')
MODES = ('b2', 'b2x', 'b2f', 'h2f')
GPU_SIZES = ((33, None), (1025, None), (40001, None), (1 << 18, 230000))       # (rows, device-side count of valid rows)
EMU_SIZES = ((33, None), (1025, None), (5000, None))
SENTINEL = 7.0


def case_name(mode, n, n_valid, live):
    return '%s n=%d valid=%s %s' % (mode, n, n_valid, 'live-list' if live else 'all-rows')


def inputs(n, n_valid):
    """seeded by the size alone; a third of the rows carry an exactly zero dL/d(raw) (what the live list leaves out); rows behind the
    device-side count hold NaN"""
    import numpy as np
    from xrnerf_amd import synthetic as S
    rng = np.random.default_rng(1000 + n)
    enc = rng.normal(0, 0.5, (n, 32)).astype(np.float32)
    dirs = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    draw = rng.normal(0, 1, (n, 4)).astype(np.float32)
    draw[rng.uniform(size=n) < 1.0 / 3.0] = 0.0
    if n_valid is not None:
        enc[n_valid:] = np.nan
        draw[n_valid:] = np.nan
    return enc, dirs, draw, S.mlp_weights(32, 64, 1, 16, 4), S.mlp_weights(32, 64, 2, 16, 5)


def digests(dev, sizes=GPU_SIZES, modes=MODES):
    """{case: {'dwd' | 'dwc' | 'denc': sha256}} of the library xrnerf_amd has loaded"""
    import numpy as np
    import torch
    from xrnerf_amd import ops
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sha = lambda t: hashlib.sha256(np.ascontiguousarray(t.cpu().numpy(), dtype=np.float32).tobytes()).hexdigest()
    out = {}
    saved = os.environ.get('XR_MLP_BWD_DW')
    try:
        for n, n_valid in sizes:
            enc, dirs, draw, wd, wc = inputs(n, n_valid)
            enc_t, td, tdirs, twd, twc = T(enc.T), T(draw), T(dirs), T(wd), T(wc)
            n_dev = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device=dev)
            for mode in modes:
                os.environ['XR_MLP_BWD_DW'] = mode          # read by the library at every call
                for live in (False, True):
                    g_wd = torch.zeros(wd.size, dtype=torch.float32, device=dev)
                    g_wc = torch.zeros(wc.size, dtype=torch.float32, device=dev)
                    denc_t = torch.full((32, n), SENTINEL, dtype=torch.float32, device=dev)
                    lst = ops.live_rows(td, n, n_dev=n_dev) if live else None
                    ops.nerf_mlp_bwd(enc_t, tdirs, n, twd, twc, 1, 2, td, g_wd, g_wc, denc_t=denc_t, n_dev=n_dev, live=lst)
                    if dev.type == 'cuda':
                        torch.cuda.synchronize()
                    out[case_name(mode, n, n_valid, live)] = {'dwd': sha(g_wd), 'dwc': sha(g_wc), 'denc': sha(denc_t)}
    finally:
        if saved is None:
            os.environ.pop('XR_MLP_BWD_DW', None)
        else:
            os.environ['XR_MLP_BWD_DW'] = saved
    return out


def child(emu_lib, out_path, modes):
    sys.path.insert(0, ROOT)
    import torch
    if emu_lib:
        sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))
        import emubuild
        import emulib
        build = emubuild.build
        emubuild.build = lambda name, extra=(): emu_lib if name == 'xr_mlp' else build(name, extra)
        with emulib.emulated_ops() as dev:
            d = digests(dev, EMU_SIZES, modes)
    else:
        from xrnerf_amd import _lib
        _lib.load()
        d = digests(torch.device('cuda:0'), GPU_SIZES, modes)
    with open(out_path, 'w') as f:
        json.dump(d, f)
    return 0


def run(lib, emu, modes=MODES):
    """digests of one library, computed in a fresh process"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'digests.json')
        env = dict(os.environ)
        env.pop('XR_MLP_BWD_DW', None)
        cmd = [sys.executable, os.path.abspath(__file__), '--child', out, '--modes', ','.join(modes)]
        if emu:
            cmd += ['--emu-lib', os.path.abspath(lib)]
        else:
            env['XRNERF_LIB'] = os.path.abspath(lib)
        subprocess.run(cmd, env=env, check=True, timeout=3000)
        with open(out) as f:
            return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('libs', nargs='*')
    ap.add_argument('--emu', action='store_true', help='the libraries are host builds of xr_mlp.hip')
    ap.add_argument('--record', metavar='LIB', help='write the golden digests from this library (GPU)')
    ap.add_argument('--commit', help='with --record: the commit LIB was built from')
    ap.add_argument('--out', default=GOLDEN)
    ap.add_argument('--modes', default=','.join(MODES), help='XR_MLP_BWD_DW values, comma separated (f32 may be added; the golden file holds the default four)')
    ap.add_argument('--child', metavar='OUT', help=argparse.SUPPRESS)
    ap.add_argument('--emu-lib', help=argparse.SUPPRESS)
    a = ap.parse_args()
    modes = tuple(a.modes.split(','))
    if a.child:
        return child(a.emu_lib, a.child, modes)
    if a.record:
        if not a.commit:
            ap.error('--record needs --commit')
        d = run(a.record, False)
        with open(a.out, 'w') as f:
            json.dump({'recorded_with': 'the library built from commit %s, on an MI355X' % a.commit, 'cases': d}, f, indent=1, sort_keys=True)
            f.write('\n')
        print('%d cases -> %s' % (len(d), a.out))
        return 0
    if len(a.libs) != 2:
        ap.error('two library paths')
    da, db = run(a.libs[0], a.emu, modes), run(a.libs[1], a.emu, modes)
    bad = 0
    print('A = %s\nB = %s' % tuple(a.libs))
    print('%-44s %-6s %-6s %-6s' % ('case', 'dWd', 'dWc', 'denc'))
    for k in sorted(set(da) | set(db)):
        cols = ['same' if k in da and k in db and da[k][x] == db[k][x] else 'DIFF' for x in ('dwd', 'dwc', 'denc')]
        bad += cols.count('DIFF')
        print('%-44s %-6s %-6s %-6s' % tuple([k] + cols))
    print('%d cases, %d arrays differ' % (len(da), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
