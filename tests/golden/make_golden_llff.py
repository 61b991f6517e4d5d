"""Generates tests/golden/ref_llff.npz from the REFERENCE ITSELF (needs the reference tree; the fixture, not the reference,
travels): the outputs of the reference's own load_llff_data (xrnerf/datasets/load_data/load_llff.py, imageio replaced by PIL)
on the tiny forward-facing rig tests/test_datasets.py::write_llff_scene writes, for the three pose-normalisation variants
of tests/test_datasets.py::LLFF_VARIANTS.

Run:  python tests/golden/make_golden_llff.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import test_datasets as T
    assert os.path.isdir(os.path.join(T.REF, 'xrnerf')), 'needs the reference tree'
    out = {}
    with tempfile.TemporaryDirectory() as d:
        T.write_llff_scene(d)
        for v, kw in enumerate(T.LLFF_VARIANTS):
            b = T.reference_load_llff(d, kw)
            for k in range(4):
                out['v%d_%d' % (v, k)] = np.asarray(b[k])
            out['v%d_4' % v] = np.array(int(b[4]))
    np.savez_compressed(os.path.join(HERE, 'ref_llff.npz'), **out)
    print(sorted((k, v.shape, v.dtype.str) for k, v in out.items()))


if __name__ == '__main__':
    main()
