"""GNR's image encoder and network on the host (no GPU): the generated weights, the reference's state_dict names and shapes, the
tensor-op path of HGFilter against the reference's own run (tests/golden/ref_gnr_encoder.npz) and against the restatement, the refusals,
and GnrNetwork built from the `model` dict of configs/gnr/gnr_genebody.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import gnr_encoder_restatement as R  # noqa: E402
import test_gpu_gnr_encoder as T  # noqa: E402
from test_gpu_gnr_encoder import gold, held  # noqa: E402,F401

CPU = torch.device('cpu')


def f64(gold, name):
    return gold[name].astype(np.float64) + gold[name + '.d']


def shapes_of(gold):
    return {str(k): tuple(json.loads(str(s))) for k, s in zip(gold['keys'], gold['shapes'])}


def test_generated_weights_match_the_fixture(gold):
    sd = R.make_state_dict(shapes_of(gold))
    assert [R.crc(sd[str(k)].numpy()) for k in gold['keys']] == gold['crcs'].tolist()
    assert sum(v.numel() for k, v in sd.items() if 'downsample.0.' not in k) == 14420864


def test_key_set_is_the_references_and_loads_strictly(gold):
    from xrnerf_amd import builder
    with open(os.path.join(T.G, 'gnr_encoder_cfg.json')) as f:
        m = builder.build_embedder(json.load(f)['image_filter'])
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold['keys']]
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes_of(gold)
    # every ConvBlock owns a bn4, used or not; with a downsample the same parameters appear a second time
    assert 'conv3.bn4.weight' in sd and 'conv3.downsample.0.weight' not in sd
    assert sd['conv4.bn4.weight'].data_ptr() == sd['conv4.downsample.0.weight'].data_ptr()
    m.load_state_dict(R.make_state_dict(shapes_of(gold)), strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'm3.b3_1.bn4.bias'}, strict=True)


def test_host_path_holds_the_fixture_at_the_three_taps(gold):
    m = T.fixture_filter(gold, CPU)
    taps = {}
    with torch.no_grad():
        out = m(torch.from_numpy(gold['images']), taps)
    assert tuple(out.shape) == (2, 256, 8, 4)
    for name in ('conv4', 'm0', 'out'):
        held(taps[name].numpy(), gold[name], f64(gold, name), 'host path %s' % name)


def test_restatement_holds_the_fixture(gold):
    sd = R.make_state_dict(shapes_of(gold))
    taps32, taps64 = {}, {}
    with torch.no_grad():
        R.hg_filter(sd, R.CONFIG_OPT, torch.from_numpy(gold['images']), taps32)
        R.hg_filter({k: v.double() for k, v in sd.items()}, R.CONFIG_OPT, torch.from_numpy(gold['images']).double(), taps64)
    for name in ('conv4', 'm0', 'out'):
        held(taps32[name].numpy(), gold[name], f64(gold, name), 'restatement %s' % name)
        assert np.abs(taps64[name].numpy() - f64(gold, name)).max() <= 1e-12 * np.abs(f64(gold, name)).max()


@pytest.mark.parametrize('kw', (dict(hg_down='conv128'), dict(num_stack=1, num_hourglass=1), dict(num_stack=2, num_hourglass=1, hourglass_dim=64)))
def test_other_options_against_the_restatement(kw):
    from xrnerf_amd import gnr_encoder as E
    opt = T.opt_of(**kw)
    m, sd = T.generated(E.HGFilter(opt))
    x = T.u(np.random.default_rng(9), -1, 1, (1, 3, 16, 32))
    with torch.no_grad():
        got = m(x)
        r32 = R.hg_filter(sd, opt, x)
        r64 = R.hg_filter({k: v.double() for k, v in sd.items()}, opt, x.double())
    assert tuple(got.shape) == (1, opt.hourglass_dim, 4, 8)
    held(got.numpy(), r32.numpy(), r64.numpy(), 'host path %r' % (kw,))


def test_conv64_fails_at_construction_like_the_reference():
    """hg_down='conv64' asks for ConvBlock(64, 64), whose bn3 is GroupNorm(32, 16): torch refuses it, in the reference as well"""
    from xrnerf_amd import gnr_encoder as E
    with pytest.raises(ValueError):
        E.HGFilter(T.opt_of(hg_down='conv64'))


def test_batch_norm_and_bad_sizes_raise():
    from xrnerf_amd import gnr_encoder as E
    with pytest.raises(NotImplementedError):
        E.HGFilter(T.opt_of(norm='batch'))
    with pytest.raises(NotImplementedError):
        E.ConvBlock(64, 128, 'batch')
    with pytest.raises(NameError):
        E.HGFilter(T.opt_of(hg_down='nearest'))
    m = E.HGFilter(T.opt_of(num_stack=1))
    for shape in ((1, 3, 40, 20), (1, 3, 32, 20), (1, 4, 32, 16)):
        with pytest.raises(ValueError):
            m(torch.zeros(shape))


def test_sr_filters_shapes():
    from xrnerf_amd import builder
    sr = builder.build_embedder(dict(type='SRFilters', order=2, in_ch=8, out_ch=4))
    assert [tuple(c.weight.shape) for c in sr.convs] == [(4, 11, 3, 3), (4, 7, 3, 3), (4, 7, 3, 3)]
    with torch.no_grad():
        assert tuple(sr(torch.zeros((2, 8, 4, 6)), torch.zeros((2, 3, 16, 24))).shape) == (2, 4, 16, 24)


@pytest.fixture(scope='module')
def network():
    from xrnerf_amd import builder
    torch.manual_seed(3)
    return builder.build_network(T.network_cfg())


def test_config_model_builds_frozen_and_initialised():
    from xrnerf_amd import builder
    from xrnerf_amd.gnr_encoder import HGFilter
    from xrnerf_amd.gnr_network import GnrNetwork
    from xrnerf_amd.gnr_render import GNRMLP, GnrRenderer
    with open(os.path.join(T.G, 'gnr_model_cfg.json')) as f:
        model = json.load(f)
    torch.manual_seed(1)
    net = builder.build_network(model)                                              # the configuration's dict, unchanged
    assert isinstance(net, GnrNetwork) and isinstance(net.image_filter, HGFilter) and isinstance(net.nerf, GNRMLP)
    assert isinstance(net.nerf_renderer, GnrRenderer) and net.nerf_renderer.nerf is net.nerf and not hasattr(net, 'sr_filter')
    assert net.num_views == 4 and net.feat_dim == 256 and net.nerf_renderer.N_samples == 256
    assert all(not p.requires_grad for p in net.image_filter.parameters()) and all(p.requires_grad for p in net.nerf.parameters())
    for mod in net.modules():
        if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)):
            if mod.weight.numel() >= 4096:
                assert abs(float(mod.weight.std()) - 0.02) < 0.002 and abs(float(mod.weight.mean())) < 0.002
            assert mod.bias is None or not bool(mod.bias.any())
    with pytest.raises(NotImplementedError):
        net.reconstruct({})
    model['cfg']['train_encoder'] = True
    assert all(p.requires_grad for p in builder.build_network(model).image_filter.parameters())


def test_image_rescale_and_get_image_feature(network):
    net = network
    masks = torch.zeros((4, 1, 8, 8))
    masks[:, :, 2:6] = 1
    plus = torch.rand((4, 3, 8, 8))                                                 # already in [0, 1]: returned as it is
    assert net.image_rescale(plus, masks) is plus
    minus = plus * 2 - 1
    minus[0, 0, 0, 0] = -1
    want = (minus + 1) / 2 * (masks > 0).float()
    assert torch.equal(net.image_rescale(minus, masks), want)
    data = {'images': minus, 'masks': masks, 'feats': torch.zeros(1)}               # feats given: nothing is touched
    assert net.get_image_feature(data) is data and data['images'] is minus and data['feats'].numel() == 1
    assert net.to8b(torch.full((3, 2, 2), 0.5)).tolist() == [[[127] * 3] * 2] * 2 and net.to8b(np.full((2, 2, 3), -1.0)).max() == 0


def test_forward_is_the_renderer_on_the_encoders_maps(network):
    net = network
    data = T.scene_data(CPU)
    with T.host_draws(5):
        got = net(dict(data))
    with torch.no_grad():
        feats = net.image_filter(data['images'][:4])
    assert tuple(feats.shape) == (4, 256, 16, 16)
    with T.host_draws(5):
        want = net.nerf_renderer.render(**dict(data, feats=feats))
    assert torch.isfinite(got['loss']) and got['num_samples'] == 48
    assert float(got['loss']) == float(want['loss'])
    filled = net.get_image_feature(dict(data))
    assert torch.equal(filled['feats'], feats) and torch.equal(filled['images'], data['images'])
    assert got['loss'].requires_grad                                                # the network trains through the frozen encoder's maps
