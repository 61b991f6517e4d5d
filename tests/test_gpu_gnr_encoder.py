"""GNR's image encoder on the kernels of xrnerf_amd/csrc/xr_gnr_encoder.hip: every stage against float64 torch
ops, ConvBlock / HourGlass against the restatement, HGFilter against the reference's own run (tests/golden/ref_gnr_encoder.npz), and
GnrNetwork on the generated scene.

The bar of every comparison is sections 13-15's: max|got - ref64| <= max(4 max|ref32 - ref64|, 2^-22 max|ref64|) per tensor, where
ref32 is the reference's (or torch's) float32 CPU run of the same composition, never the code under test.  The check_* bodies take the
device, so tests/test_emu_gnr_encoder.py runs them on the kernels' host build."""
import contextlib
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')
import gnr_encoder_restatement as R  # noqa: E402

FLOOR = 2.0 ** -22
RATIOS = {}                                     # what -> worst figure / bar, for profiles/gnr_encoder_gpu_tests.txt


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_gnr_encoder.npz'))


def held(got, r32, r64, what, columns=False, floor_abs=0.0):
    got, r32, r64 = (np.asarray(a, np.float64) for a in (got, r32, r64))
    assert got.shape == r64.shape and np.isfinite(got).all(), what
    if got.size == 0:
        return
    ax = tuple(range(got.ndim - 1)) if columns else None
    scale = np.abs(r64).max(ax)
    bar = np.maximum(np.maximum(4.0 * np.abs(r32 - r64).max(ax), FLOOR * scale), floor_abs)
    worst = np.abs(got - r64).max(ax)
    ratio = float(np.max(worst / np.maximum(bar, 1e-300)))
    RATIOS[what] = max(RATIOS.get(what, 0.0), ratio)
    print('%s: worst %.3e, bar %.3e, ratio %.3f (max|ref| %.3e)' % (what, float(np.max(worst)), float(np.max(bar)), ratio, float(np.max(scale))))
    assert (worst <= bar).all(), (what, np.asarray(worst).tolist(), np.asarray(bar).tolist())


def write_ratios(tier):
    path = os.environ.get('XR_GNR_ENCODER_RATIOS')
    if path:
        with open(path, 'w') as f:
            f.write('# worst |got - ref64| / bar of every bar of tests/test_gpu_gnr_encoder.py on the %s (1.0 = at the bar)\n' % tier)
            for k in sorted(RATIOS):
                f.write('%-70s %.4f\n' % (k, RATIOS[k]))


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def last(x, dev):
    """[N,C,H,W] host tensor -> a channel-last float32 copy on the device (a copy on the host too, where a map with one pixel is
    already contiguous after the permute)"""
    return x.float().permute(0, 2, 3, 1).contiguous().clone().to(dev)


def first(y):
    """channel-last device map -> [N,C,H,W] float64 numpy"""
    return y.detach().cpu().permute(0, 3, 1, 2).double().numpy()


def group_norm(x, gamma, beta):
    """F.group_norm(x, 32, gamma, beta, 1e-5) without its refusal of a single value per channel (the 1 x 1 x 1 case)"""
    N, C, H, W = x.shape
    return torch.native_group_norm(x, gamma, beta, N, C, H * W, 32, 1e-5)[0]


def u(rng, lo, hi, shape):
    return torch.from_numpy(rng.uniform(lo, hi, shape).astype(np.float32))


# ------------------------------------------------------------------------------------------ convolution
# (N, H, W, Cin, Cout, k, stride): the 3x3 grid of the issue, the two 1x1 layers, the stem, the strided 3x3 -- all on the 64 x 64 tile
# (306 rows = five row tiles, the last one ragged) -- and one launch on each of the other two tiles: 128 x 128 takes Cout >= 128 and at
# least 256 workgroups, 128 x 64 takes Cout <= 64 and at least 256 row tiles; both with a ragged last row tile
CONV_CASES = [(n, h, w, ci, co, 3, 1) for (n, h, w) in ((1, 1, 1), (1, 3, 2), (2, 5, 7), (2, 17, 9)) for (ci, co) in ((32, 32), (64, 128), (256, 128))] + \
             [(2, 5, 7, 256, 256, 1, 1), (2, 5, 7, 64, 128, 1, 1), (2, 12, 10, 3, 64, 7, 2), (2, 6, 8, 128, 128, 3, 2)]
CONV_TILE_CASES = [(1, 130, 127, 32, 256, 1, 1), (1, 182, 181, 32, 64, 3, 1)]
CONV_VARIANTS = ((False, False, False), (True, True, True), (True, False, False), (False, True, True))      # (norm, bias, add)


def conv_inputs(case, seed=0):
    N, H, W, Cin, Cout, k, stride = case
    rng = np.random.default_rng([seed, N, H, W, Cin, Cout, k, stride])
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return {'x': u(rng, -1, 1, (N, Cin, H, W)) + u(rng, -0.5, 0.5, (1, Cin, 1, 1)),
            'w': u(rng, -1, 1, (Cout, Cin, k, k)) * float(1.4 * np.sqrt(3.0 / (Cin * k * k))),
            'gamma': u(rng, 0.5, 1.5, (Cin,)), 'beta': u(rng, -0.3, 0.3, (Cin,)), 'bias': u(rng, -0.3, 0.3, (Cout,)),
            'y0': u(rng, -1, 1, (N, Cout, Ho, Wo))}


def conv_reference(i, case, norm, bias, add, dtype):
    stride, k = case[6], case[5]
    t = {n: v.to(dtype) for n, v in i.items()}
    x = F.relu(group_norm(t['x'], t['gamma'], t['beta'])) if norm else t['x']
    y = F.conv2d(x, t['w'], t['bias'] if bias else None, stride=stride, padding=k // 2)
    return (t['y0'] + y if add else y).double().numpy()


def conv_run(dev, i, case, norm, bias, add, relu=False):
    from xrnerf_amd import ops
    k, stride = case[5], case[6]
    x = last(i['x'], dev)
    stats = ops.hg_gn_stats(x) + (i['gamma'].to(dev), i['beta'].to(dev)) if norm else None
    out = last(i['y0'], dev) if add else None
    y = ops.hg_conv2d(x, ops.hg_relay_weight(i['w'].to(dev)), k, stride, stats, i['bias'].to(dev) if bias else None, relu, out, add)
    sync()
    return y


def check_conv(dev, case):
    i = conv_inputs(case)
    for norm, bias, add in CONV_VARIANTS:
        if norm and case[3] % 32:
            continue
        y = conv_run(dev, i, case, norm, bias, add)
        held(first(y), conv_reference(i, case, norm, bias, add, torch.float32), conv_reference(i, case, norm, bias, add, torch.float64),
             'conv k%d s%d %d->%d norm %d bias %d add %d' % (case[5], case[6], case[3], case[4], norm, bias, add))
    # option (c), and the same bits twice
    y1 = conv_run(dev, i, case, False, True, False, relu=True)
    y2 = conv_run(dev, i, case, False, True, False, relu=True)
    assert torch.equal(y1, y2)
    held(first(y1), np.maximum(conv_reference(i, case, False, True, False, torch.float32), 0), np.maximum(conv_reference(i, case, False, True, False, torch.float64), 0),
         'conv k%d s%d %d->%d relu' % (case[5], case[6], case[3], case[4]))


def check_conv_slices(dev):
    """reads columns 32..96 of a 160-wide buffer and adds into columns 64..192 of a 200-wide one: everything else keeps its bits"""
    from xrnerf_amd import ops
    case = (2, 5, 7, 64, 128, 3, 1)
    i = conv_inputs(case, 1)
    xin = torch.full((2, 5, 7, 160), 9.0, device=dev)
    xin[..., 32:96] = last(i['x'], dev)
    out = torch.full((2, 5, 7, 200), 7.0, device=dev)
    out[..., 64:192] = last(i['y0'], dev)
    stats = ops.hg_gn_stats(xin[..., 32:96]) + (i['gamma'].to(dev), i['beta'].to(dev))
    ops.hg_conv2d(xin[..., 32:96], ops.hg_relay_weight(i['w'].to(dev)), 3, 1, stats, i['bias'].to(dev), False, out[..., 64:192], True)
    sync()
    held(first(out[..., 64:192]), conv_reference(i, case, True, True, True, torch.float32), conv_reference(i, case, True, True, True, torch.float64), 'conv on slices')
    assert bool((out[..., :64] == 7).all()) and bool((out[..., 192:] == 7).all())
    assert bool((xin[..., :32] == 9).all()) and bool((xin[..., 96:] == 9).all())


def check_conv_padding_after_norm(dev):
    """beta = 5: a normalised padding tap would contribute relu(beta - mean rstd gamma) ~ 5 per weight to every border output"""
    case = (2, 5, 7, 32, 32, 3, 1)
    i = conv_inputs(case, 2)
    i['beta'] = i['beta'] + 5.0
    y = conv_run(dev, i, case, True, False, False)
    held(first(y), conv_reference(i, case, True, False, False, torch.float32), conv_reference(i, case, True, False, False, torch.float64), 'conv padding after the norm')


def check_conv_refusals(dev):
    from xrnerf_amd import _lib, ops
    x = torch.zeros((1, 3, 2, 32), device=dev)
    w = torch.zeros((9 * 32, 32), device=dev)
    out = torch.full((1, 3, 2, 32), 7.0, device=dev)
    for k, stride in ((5, 1), (3, 3)):
        with pytest.raises(_lib.XrError):
            ops.hg_conv2d(x, torch.zeros((k * k * 32, 32), device=dev), k, stride)
    with pytest.raises((_lib.XrError, ValueError)):
        ops.hg_conv2d(x, w[:, :30].contiguous(), 3, 1, None, None, False, out[..., :30])                   # Cout not a multiple of 4
    with pytest.raises(ValueError):
        ops.hg_conv2d(x.permute(0, 3, 1, 2), w, 3, 1)                                          # not channel-last
    assert bool((out == 7).all())


# ------------------------------------------------------------------------------------------ statistics, pool, bicubic
STATS_CASES = [(2, 1, 1, 32), (1, 17, 18, 32), (2, 17, 18, 64), (2, 17, 18, 256), (2, 40, 30, 64)]     # 1 and 306 pixels (three chunks); 1200 = ten chunks, more than the second pass has phases


def stats_reference(x, dtype):
    N, C, H, W = x.shape
    _, mean, rstd = torch.native_group_norm(x.to(dtype), None, None, N, C, H * W, 32, 1e-5)
    return mean.double().numpy(), rstd.double().numpy()


def check_stats(dev, case):
    from xrnerf_amd import ops
    N, H, W, C = case
    rng = np.random.default_rng([3, N, H, W, C])
    x = u(rng, -1, 1, (N, C, H, W)) * u(rng, 0.2, 3, (1, C, 1, 1)) + u(rng, -2, 2, (1, C, 1, 1))
    x[:, :C // 32] = 3.7                                                                       # a constant group: variance 0
    xl = last(x, dev)
    mean, rstd = ops.hg_gn_stats(xl)
    mean2, rstd2 = ops.hg_gn_stats(xl)
    sync()
    assert torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    (m32, r32), (m64, r64) = stats_reference(x, torch.float32), stats_reference(x, torch.float64)
    held(mean.cpu().numpy(), m32, m64, 'stats mean, groups of %d' % (C // 32))
    held(rstd.cpu().numpy(), r32, r64, 'stats rstd, groups of %d' % (C // 32))
    assert np.isfinite(rstd.cpu().numpy()).all()
    # a slice of a wider buffer, and the stand-alone apply
    wide = torch.full((N, H, W, C + 40), 5.0, device=dev)
    wide[..., 8:8 + C] = xl
    m3, r3 = ops.hg_gn_stats(wide[..., 8:8 + C])
    assert torch.equal(m3, mean) and torch.equal(r3, rstd)
    gamma, beta = u(rng, 0.5, 1.5, (C,)), u(rng, -0.3, 0.3, (C,))
    y = ops.hg_gn_relu(wide[..., 8:8 + C], mean, rstd, gamma.to(dev), beta.to(dev), out=wide[..., 8:8 + C])
    sync()
    ref = lambda dt: F.relu(group_norm(x.to(dt), gamma.to(dt), beta.to(dt))).double().numpy()
    held(first(y), ref(torch.float32), ref(torch.float64), 'norm + relu apply, groups of %d' % (C // 32))
    assert bool((wide[..., :8] == 5).all()) and bool((wide[..., 8 + C:] == 5).all())


POOL_CASES = [(2, 4, 6, 32), (2, 5, 7, 64)]
BICUBIC_CASES = [(2, 1, 1, 32), (2, 1, 2, 32), (2, 2, 1, 32), (2, 3, 5, 64), (2, 8, 4, 256)]


def check_pool(dev, case):
    from xrnerf_amd import ops
    N, H, W, C = case
    x = u(np.random.default_rng([4, H, W]), -1, 1, (N, C, H, W))
    y = ops.hg_avgpool2(last(x, dev))
    sync()
    assert tuple(y.shape) == (N, H // 2, W // 2, C)
    held(first(y), F.avg_pool2d(x, 2, stride=2).double().numpy(), F.avg_pool2d(x.double(), 2, stride=2).numpy(), 'avg_pool %dx%d' % (H, W))


def check_bicubic(dev, case):
    from xrnerf_amd import ops
    N, H, W, C = case
    rng = np.random.default_rng([5, H, W])
    x, add = u(rng, -1, 1, (N, C, H, W)), u(rng, -1, 1, (N, C, 2 * H, 2 * W))
    up = lambda t: F.interpolate(t, scale_factor=2, mode='bicubic', align_corners=True)
    y = ops.hg_bicubic_up2(last(x, dev))
    addl = last(add, dev)
    z = ops.hg_bicubic_up2(last(x, dev), addend=addl, out=addl)
    sync()
    assert z.data_ptr() == addl.data_ptr()
    held(first(y), up(x).double().numpy(), up(x.double()).numpy(), 'bicubic %dx%d' % (H, W))
    held(first(z), (add + up(x)).double().numpy(), (add.double() + up(x.double())).numpy(), 'bicubic %dx%d with addend' % (H, W))


# ------------------------------------------------------------------------------------------ modules
def opt_of(**kw):
    from xrnerf_amd.builder import ConfigDict
    return ConfigDict(dict(R.CONFIG_OPT, **kw))


def generated(module):
    """the module with the generated weights of its own state_dict names loaded strictly -> (module, state_dict)"""
    sd = R.make_state_dict({k: tuple(v.shape) for k, v in module.state_dict().items()})
    module.load_state_dict(sd, strict=True)
    return module.eval(), sd


def check_module(dev, kind):
    from xrnerf_amd import gnr_encoder as E
    if kind == 'block 64->128':
        m, sd = generated(E.ConvBlock(64, 128, 'group'))
        fn, C = (lambda s, x: R.conv_block(s, x)), 64
    elif kind == 'block 256->256':
        m, sd = generated(E.ConvBlock(256, 256, 'group'))
        fn, C = (lambda s, x: R.conv_block(s, x)), 256
    else:
        m, sd = generated(E.HourGlass(1, 2, 256, 'group'))
        fn, C = (lambda s, x: R.hourglass(s, 2, x)), 256
    x = u(np.random.default_rng([6, C]), -1, 1, (2, C, 8, 4))
    with torch.no_grad():
        got = m.to(dev)(x.to(dev))
        sync()
        held(got.cpu().numpy(), fn(sd, x).double().numpy(), fn({k: v.double() for k, v in sd.items()}, x.double()).numpy(), kind)


_filters = {}


def fixture_filter(gold, dev):
    """HGFilter with the config's options and the fixture's generated weights (checked against its CRCs), on the device"""
    if str(dev) not in _filters:
        from xrnerf_amd import builder
        with open(os.path.join(G, 'gnr_encoder_cfg.json')) as f:
            cfg = json.load(f)
        shapes = {str(k): tuple(json.loads(str(s))) for k, s in zip(gold['keys'], gold['shapes'])}
        sd = R.make_state_dict(shapes)
        assert [R.crc(sd[str(k)].numpy()) for k in gold['keys']] == gold['crcs'].tolist()
        m = builder.build_embedder(cfg['image_filter'])
        m.load_state_dict(sd, strict=True)
        _filters[str(dev)] = m.eval().to(dev)
    return _filters[str(dev)]


def check_filter(dev, gold):
    from xrnerf_amd import gnr_render
    m = fixture_filter(gold, dev)
    images = torch.from_numpy(gold['images'])
    taps, taps2 = {}, {}
    with torch.no_grad():
        out = m(images.to(dev), taps)
        out2 = m(images.to(dev), taps2)
        sync()
        for name in ('conv4', 'm0', 'out'):
            held(taps[name].cpu().numpy(), gold[name], gold[name].astype(np.float64) + gold[name + '.d'], 'HGFilter %s' % name)
            assert torch.equal(taps[name], taps2[name]), name
        # the view handed to the renderer IS the channel-last buffer the last layer wrote
        assert tuple(out.shape) == (2, 256, 8, 4) and out.data_ptr() == gnr_render.channel_last(out).data_ptr()
        assert out.permute(0, 2, 3, 1).is_contiguous()
        # the host path inside the same bar, and a non-contiguous input
        host = fixture_filter(gold, torch.device('cpu'))(images)
        held(host.numpy(), gold['out'], gold['out'].astype(np.float64) + gold['out.d'], 'HGFilter host path')
        wide = torch.zeros((2, 3, 32, 40))
        wide[..., 5:21] = images
        strided = wide.to(dev)[..., 5:21]
        assert not strided.is_contiguous()
        assert torch.equal(m(strided), out)


def check_filter_small(dev):
    """num_stack = 1, num_hourglass = 1 on [1, 3, 16, 16] against the restatement"""
    from xrnerf_amd import gnr_encoder as E
    opt = opt_of(num_stack=1, num_hourglass=1)
    m, sd = generated(E.HGFilter(opt))
    x = u(np.random.default_rng(8), -1, 1, (1, 3, 16, 16))
    with torch.no_grad():
        got = m.to(dev)(x.to(dev))
        sync()
    held(got.cpu().numpy(), R.hg_filter(sd, opt, x).double().numpy(), R.hg_filter({k: v.double() for k, v in sd.items()}, opt, x.double()).numpy(),
         'HGFilter one stack, depth 1')


# ------------------------------------------------------------------------------------------ the network
def network_cfg():
    """the `model` dict of configs/gnr/gnr_genebody.py with the renderer at the generated scene's size (64 x 64 images, 16 samples, 48 rays)"""
    with open(os.path.join(G, 'gnr_model_cfg.json')) as f:
        model = json.load(f)
    model['cfg']['nerf_renderer']['opt'].update(loadSize=64, N_samples=16, N_rand=48, N_rand_infer=512)
    return model


def scene_data(dev, bbox=(16, 48, 16, 48)):
    """GnrNetwork's data dict from the generated scene: four source views and the query view behind them"""
    from xrnerf_amd.gnr_render import synthetic_scene
    sc = synthetic_scene()
    rng = np.random.default_rng(11)
    d = lambda t: t.to(dev)
    q_img = torch.from_numpy(rng.uniform(0, 1, (1, 3, 64, 64)).astype(np.float32))
    return {'images': d(torch.cat([sc['images'], q_img], 0)), 'masks': d(torch.cat([sc['masks'], sc['masks'][:1]], 0)),
            'calibs': d(torch.cat([sc['calibs'], sc['q_calib'][None]], 0)), 'persps': d(torch.cat([sc['persps'], sc['q_persps'][None]], 0)),
            'bbox': list(bbox), 'mesh_param': {'center': d(sc['mesh_param']['center']), 'spatial_freq': sc['mesh_param']['spatial_freq']},
            'smpl': {k: d(v) for k, v in sc['smpl'].items()}, 'scan': None}


@contextlib.contextmanager
def host_draws(seed):
    """torch.rand / torch.randn drawn from one host generator whatever the device, numpy's choice seeded: the same draws on both paths"""
    g = torch.Generator().manual_seed(seed)
    np.random.seed(seed)
    rand, randn = torch.rand, torch.randn
    torch.rand = lambda *s, device=None, **k: rand(*s, generator=g, **k).to(device or 'cpu')
    torch.randn = lambda *s, device=None, **k: randn(*s, generator=g, **k).to(device or 'cpu')
    try:
        yield
    finally:
        torch.rand, torch.randn = rand, randn


def check_network(dev):
    """forward on the device (encoder on the kernels) against the same renderer fed the host path's float32 and float64 feature maps
    with the same draws: the three losses differ through the feature maps only.  render_path repeats its bits and is the renderer's
    own on the network's maps."""
    from xrnerf_amd import builder
    torch.manual_seed(3)
    net = builder.build_network(network_cfg()).to(dev)
    data = scene_data(dev)
    with host_draws(5):
        got = net(dict(data))
    sync()
    assert torch.isfinite(got['loss']) and got['num_samples'] == 48
    host = builder.build_embedder(network_cfg()['cfg']['image_filter'])
    host.load_state_dict({k: v.cpu() for k, v in net.image_filter.state_dict().items()}, strict=True)
    images = data['images'][:4].cpu()
    with torch.no_grad():
        f32 = host(images)
        f64 = host.double()(images.double()).float()
    losses = []
    for feats in (f32, f64):
        with host_draws(5):
            losses.append(float(net.nerf_renderer.render(**dict(data, feats=feats.to(dev)))['loss']))
    held(float(got['loss']), losses[0], losses[1], 'GnrNetwork.forward loss')
    rgbs, depths = net.render_path(dict(data))
    rgbs2, _ = net.render_path(dict(data))
    sync()
    assert tuple(rgbs.shape) == (1, 64, 64, 6) and tuple(depths.shape) == (1, 64, 64) and bool(torch.isfinite(rgbs).all())
    assert torch.equal(rgbs, rgbs2)
    with torch.no_grad():
        feats = net.image_filter(data['images'][:4])
        again, _ = net.nerf_renderer.render_path(**dict(data, feats=feats))
    assert torch.equal(rgbs, again)


def check_symbols():
    """the header, the ctypes table and the library's exported symbols name the same encoder entry points"""
    import re
    from xrnerf_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_gnr_encoder.h')).read()
    declared = set(re.findall(r'^(?:int|size_t) (xr_hg_\w+)\(', header, re.M))
    assert declared == set(_lib.GNR_ENCODER_SIGNATURES) and len(declared) == 9
    for name, (res, args) in _lib.GNR_ENCODER_SIGNATURES.items():
        text = header[header.index(' %s(' % name):]
        text = text[:text.index(');')]
        assert text.count(',') + 1 == len(args), name
        assert hasattr(_lib.load(), name), name


# ------------------------------------------------------------------------------------------ the MI355X
@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from xrnerf_amd import ops
    assert ops.gnr_encoder_kernels_available(), 'the library has no xr_gnr_encoder entry points'
    check_symbols()
    yield torch.device('cuda')
    write_ratios('MI355X')


@pytest.mark.gpu
@pytest.mark.parametrize('case', CONV_CASES + CONV_TILE_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_conv_against_float64_conv2d(dev, case):
    check_conv(dev, case)


@pytest.mark.gpu
def test_conv_reads_and_writes_slices_of_wider_buffers(dev):
    check_conv_slices(dev)


@pytest.mark.gpu
def test_conv_pads_with_zeros_after_the_norm(dev):
    check_conv_padding_after_norm(dev)


@pytest.mark.gpu
def test_conv_refuses_unsupported_shapes(dev):
    check_conv_refusals(dev)


@pytest.mark.gpu
@pytest.mark.parametrize('case', STATS_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_group_statistics_and_apply(dev, case):
    check_stats(dev, case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', POOL_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_avg_pool(dev, case):
    check_pool(dev, case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', BICUBIC_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_bicubic_upsampling_with_and_without_addend(dev, case):
    check_bicubic(dev, case)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ('block 64->128', 'block 256->256', 'hourglass'))
def test_modules_against_the_restatement(dev, kind):
    check_module(dev, kind)


@pytest.mark.gpu
def test_filter_on_the_fixture(dev, gold):
    check_filter(dev, gold)


@pytest.mark.gpu
def test_filter_with_one_stack(dev):
    check_filter_small(dev)


@pytest.mark.gpu
def test_network_forward_and_render_path(dev):
    check_network(dev)
