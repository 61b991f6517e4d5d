"""Generates tests/golden/ref_gnr_encoder.npz and gnr_encoder_cfg.json from the REFERENCE'S OWN HGFilter, in the build container only:
    python tests/golden/make_golden_gnr_encoder.py

embedders/gnr_embedder.py is imported unmodified (ref_import.load() + importlib).  HGFilter is built with the option dict of
configs/gnr/gnr_genebody.py, loaded with the generated weights (tests/gnr_encoder_restatement.make_state_dict) and run on [2, 3, 32, 16]
U(-1, 1) images in float32 and float64.  32 x 16 is deliberate: the maps are 8 x 4 -> 4 x 2 -> 2 x 1, so height and width differ and the
innermost bicubic upsampling goes from width 1 to 2.

Stored: `images`; for the outputs of conv4, of m0 and of the whole filter ([2, 256, 8, 4] each, taken with forward hooks) the float32
run (`conv4`, `m0`, `out`) and the float64 run's difference from it (`conv4.d`, ...); `keys` / `shapes`, the reference's state_dict
names and shapes; `crcs`, zlib.crc32 of every generated float32 tensor.  gnr_encoder_cfg.json holds the filter's option dict and
gnr_model_cfg.json the `model` dict of configs/gnr/gnr_genebody.py.  The maker asserts that every output is finite, that the output's
standard deviation lies in (0.5, 2), that the float32 run differs from the float64 run, and that the restatement reproduces the float64
run to 1e-12 of its magnitude."""
import importlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gnr_encoder_restatement as R  # noqa: E402
import ref_import  # noqa: E402


def run():
    ref_import.load()
    emb = importlib.import_module('xrnerf.models.embedders.gnr_embedder')
    opt = ref_import.Cfg(R.CONFIG_OPT)
    torch.manual_seed(0)
    model = emb.HGFilter(opt)
    ref_sd = model.state_dict()
    keys = list(ref_sd.keys())
    shapes = {k: tuple(ref_sd[k].shape) for k in keys}
    sd = R.make_state_dict(shapes)
    model.load_state_dict(sd, strict=True)
    model.eval()
    images = torch.from_numpy(np.random.default_rng(20).uniform(-1, 1, (2, 3, 32, 16)).astype(np.float32))

    def taps_of(m, x):
        got = {}
        hooks = [getattr(m, name).register_forward_hook(lambda mod, i, o, n=name: got.__setitem__(n, o.detach().clone())) for name in ('conv4', 'm0')]
        with torch.no_grad():
            got['out'] = m(x).detach().clone()
        for h in hooks:
            h.remove()
        return got
    g32 = taps_of(model, images)
    model64 = emb.HGFilter(opt).double()
    model64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    g64 = taps_of(model64.eval(), images.double())
    mine = {}
    with torch.no_grad():
        R.hg_filter({k: v.double() for k, v in sd.items()}, R.CONFIG_OPT, images.double(), mine)
    out = {'images': images.numpy(), 'keys': np.array(keys), 'shapes': np.array([json.dumps(list(shapes[k])) for k in keys]),
           'crcs': np.array([R.crc(sd[k].numpy()) for k in keys], dtype=np.uint32)}
    for name in ('conv4', 'm0', 'out'):
        a32, a64 = g32[name].numpy(), g64[name].numpy()
        assert a32.shape == (2, 256, 8, 4) and np.isfinite(a32).all() and np.isfinite(a64).all(), name
        assert np.abs(a32.astype(np.float64) - a64).max() > 0, name
        assert np.abs(mine[name].numpy() - a64).max() <= 1e-12 * np.abs(a64).max(), (name, np.abs(mine[name].numpy() - a64).max())
        out[name] = a32
        out[name + '.d'] = a64 - a32.astype(np.float64)
        print('%-6s std %.3f  max|y| %.3f  max|f32 - f64| %.3e' % (name, a64.std(), np.abs(a64).max(), np.abs(a32 - a64).max()))
    assert 0.5 < g64['out'].std() < 2
    np.savez_compressed(os.path.join(HERE, 'ref_gnr_encoder.npz'), **out)
    with open(os.path.join(HERE, 'gnr_encoder_cfg.json'), 'w') as f:
        json.dump({'image_filter': dict(type='HGFilter', opt=R.CONFIG_OPT)}, f, indent=1, sort_keys=True)
        f.write('\n')
    # the `model` dict of the reference's configuration, as settings: what build_network is handed
    spec = importlib.util.spec_from_file_location('gnr_genebody', os.path.join(ref_import.REF, 'configs', 'gnr', 'gnr_genebody.py'))
    cfg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cfg)
    assert cfg.model['cfg']['image_filter']['opt'] == R.CONFIG_OPT
    with open(os.path.join(HERE, 'gnr_model_cfg.json'), 'w') as f:
        json.dump(cfg.model, f, indent=1, sort_keys=True)
        f.write('\n')
    print('%d state_dict entries, %d bytes' % (len(keys), os.path.getsize(os.path.join(HERE, 'ref_gnr_encoder.npz'))))


if __name__ == '__main__':
    run()
