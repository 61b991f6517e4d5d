"""Generates tests/golden/ref_pipeline.npz, the fixture of the scene-pipeline tests:  python tests/golden/make_golden_pipeline.py

Needs the reference tree (tests/golden/ref_import.py).  The reference's own datasets/pipelines/create.py, augment.py, transforms.py and
compose.py are imported unmodified (ref_import.load_mip() brings create.py in with its stubs; the remaining package shells are added
here, in this process) and run on the host in float32 on the config-shaped lists of tests/pipeline_cases.py.  The draws are pinned
inside this process, not by editing the reference: `time.time` is held constant in augment.py's namespace (SelectRays seeds numpy with
it) and torch is re-seeded before every call; select_inds and t_rand are re-derived from the same seeds and stored beside the outputs.

Stored per case and output: the float32 result, and dev = max|reference32 - restatement64| against tests/pipeline_restatement.py (the
specification).  The maker asserts that dev is within the few ulp fp32 rounding allows -- DEPTH roundings of 2^-24 relative to the
largest magnitude met on the way -- otherwise the restatement (or a stored draw) is wrong."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import pipeline_cases as K  # noqa: E402
import pipeline_restatement as RS  # noqa: E402
import ref_import  # noqa: E402

T0, SEED = 1234567.0, 20
DEPTH = 16          # no output is more than 16 roundings deep (pts under ndc: dirs 2, sum 3, t 2, shift 2, projection 3, z 3)


def reference():
    ref_import.load_mip()
    import mmcv
    mmcv.is_str = lambda x: isinstance(x, str)
    shell = types.ModuleType('xrnerf.datasets.utils')
    shell.get_rigid_transformation = None                      # transforms.py imports the name; only CalculateSkelTransf calls it
    sys.modules['xrnerf.datasets.utils'] = shell
    mods = {n: importlib.import_module('xrnerf.datasets.pipelines.' + n) for n in ('create', 'augment', 'transforms', 'compose')}
    mods['augment'].time = types.SimpleNamespace(time=lambda: T0)
    return mods


def main():
    mods = reference()
    Compose = mods['compose'].Compose
    out = {}
    for name, c in K.CASES.items():
        info = K.datainfo(c)
        comp = Compose([dict(step, **info) for step in K.pipeline_list(c)])
        torch.manual_seed(SEED)
        got = comp(K.first_dict(name))
        got = {k: v for k, v in got.items() if isinstance(v, torch.Tensor)}
        pose, image, table = K.inputs(name)
        kw = {}
        if c['chain'] == 'select':
            h0, w0, nh, nw = (c['H'] // 2 - 1, c['W'] // 2 - 1, 2, 2) if (c['precrop_iters'] and c['iter_n'] < c['precrop_iters']) else (0, 0, c['H'], c['W'])
            np.random.seed(int(T0 + 0))
            inds = np.random.choice(nh * nw, size=[c['sel_n']], replace=False)
            out[name + '.select_inds'] = inds.astype(np.int64)
            kw.update(c2w=pose[:3, :4], sel=(h0 + inds // nw) * c['W'] + w0 + inds % nw, image=image)
            R = c['sel_n']
        elif c['chain'] == 'flatten':
            kw.update(c2w=pose[:3, :4])
            R = c['H'] * c['W']
        else:
            kw.update(table=table[c['N_rand'] * c['idx']:c['N_rand'] * (c['idx'] + 1)])
            R = c['N_rand']
        if c['perturb'] or c['randomized']:
            torch.manual_seed(SEED)
            out[name + '.t_rand'] = kw['t_rand'] = torch.rand(R, c['S']).numpy()
        near, far = (c['near'], c['far']) if c['near_new'] is None else (c['near_new'], c['far_new'])
        spec = RS.ray_front(c['H'], c['W'], info['K'], with_viewdirs=c['viewdirs'], ndc=c['ndc'], with_radii=c['radius'], near=near, far=far, S=c['S'],
                            lindisp=c['lindisp'], with_pts=c['pts'], **kw)
        line = []
        for k, v in got.items():
            v = v.numpy()
            out['%s.out.%s' % (name, k)] = np.ascontiguousarray(v)
            if k == 'src_shape':
                assert v.tolist() == [c['H'], c['W'], 3]
                dev = 0.0
            else:
                assert v.dtype == np.float32 and v.shape == spec[k].shape, (name, k, v.dtype, v.shape, spec[k].shape)
                dev = float(np.abs(v.astype(np.float64) - spec[k]).max())
                scale = max(1.0, float(np.abs(spec[k]).max()), max(float(np.abs(spec[q]).max()) for q in ('rays_o', 'rays_d')))
                assert dev <= DEPTH * 2.0 ** -24 * scale, (name, k, dev, DEPTH * 2.0 ** -24 * scale)
            out['%s.dev.%s' % (name, k)] = np.float64(dev)
            line.append('%s %.2e' % (k, dev))
        assert sorted(k for k in spec if k in got or k == 'pts' and c['pts']) == sorted(k for k in got if k != 'src_shape'), (name, sorted(spec), sorted(got))
        print('%-16s R %2d S %2d  %s' % (name, R, c['S'], '  '.join(line)))
    path = os.path.join(HERE, 'ref_pipeline.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
