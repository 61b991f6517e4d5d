"""GNR's image encoder (the reference's embedders/gnr_embedder.py: ConvBlock, HourGlass, HGFilter with norm='group') restated as plain
torch functions over a state_dict, dtype-generic: the float64 (and float32 CPU) references of the encoder tests at shapes outside the
fixture tests/golden/ref_gnr_encoder.npz.  tests/golden/make_golden_gnr_encoder.py holds it to the reference's own modules.

make_state_dict(shapes) is the rule that generates the weights (the full model has 14.4 M parameters: too many to commit): per key,
np.random.default_rng(zlib.crc32(key)); convolution weights U(-1, 1) 1.4 sqrt(3 / fan_in), norm weights U(0.5, 1.5), every bias
U(-0.3, 0.3).  `downsample.0.*` is ConvBlock's bn4 under a second name and gets bn4's values."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

CONFIG_OPT = dict(norm='group', num_stack=4, num_hourglass=2, skip_hourglass=True, hg_down='ave_pool', hourglass_dim=256)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def make_state_dict(shapes, dtype=torch.float32):
    """shapes: {key: shape} (the reference's state_dict names) -> {key: tensor}; generated in float32, then cast"""
    sd = {}
    for key, shape in shapes.items():
        shape = tuple(int(v) for v in shape)
        rng = np.random.default_rng(zlib.crc32(key.replace('downsample.0.', 'bn4.').encode()))
        if key.endswith('.bias'):
            a = rng.uniform(-0.3, 0.3, shape)
        elif len(shape) == 4:
            a = rng.uniform(-1.0, 1.0, shape) * (1.4 * np.sqrt(3.0 / (shape[1] * shape[2] * shape[3])))
        else:
            a = rng.uniform(0.5, 1.5, shape)
        sd[key] = torch.from_numpy(a.astype(np.float32)).to(dtype)
    return sd


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def norm_relu(sd, name, x):
    return F.relu(F.group_norm(x, 32, sd[name + '.weight'], sd[name + '.bias'], 1e-5))


def conv(sd, name, x, stride=1):
    w = sd[name + '.weight']
    return F.conv2d(x, w, sd.get(name + '.bias'), stride=stride, padding=w.shape[-1] // 2)


def conv_block(sd, x):
    out1 = conv(sd, 'conv1', norm_relu(sd, 'bn1', x))
    out2 = conv(sd, 'conv2', norm_relu(sd, 'bn2', out1))
    out3 = conv(sd, 'conv3', norm_relu(sd, 'bn3', out2))
    residual = conv(sd, 'downsample.2', norm_relu(sd, 'bn4', x)) if 'downsample.2.weight' in sd else x
    return torch.cat((out1, out2, out3), 1) + residual


def hourglass(sd, depth, x):
    def level(n, inp):
        up1 = conv_block(_sub(sd, 'b1_%d.' % n), inp)
        low1 = conv_block(_sub(sd, 'b2_%d.' % n), F.avg_pool2d(inp, 2, stride=2))
        low2 = level(n - 1, low1) if n > 1 else conv_block(_sub(sd, 'b2_plus_%d.' % n), low1)
        low3 = conv_block(_sub(sd, 'b3_%d.' % n), low2)
        return up1 + F.interpolate(low3, scale_factor=2, mode='bicubic', align_corners=True)
    return level(depth, x)


def hg_filter(sd, opt, x, taps=None):
    """HGFilter.forward; taps (a dict) receives the outputs of conv4, m0 and the whole filter"""
    x = norm_relu(sd, 'bn1', conv(sd, 'conv1', x, stride=2))
    x = conv_block(_sub(sd, 'conv2.'), x)
    x = F.avg_pool2d(x, 2, stride=2) if opt['hg_down'] == 'ave_pool' else conv(sd, 'down_conv2', x, stride=2)
    previous = conv_block(_sub(sd, 'conv4.'), conv_block(_sub(sd, 'conv3.'), x))
    if taps is not None:
        taps['conv4'] = previous
    for i in range(opt['num_stack']):
        hg = hourglass(_sub(sd, 'm%d.' % i), opt['num_hourglass'], previous)
        if taps is not None and i == 0:
            taps['m0'] = hg
        ll = norm_relu(sd, 'bn_end%d' % i, conv(sd, 'conv_last%d' % i, conv_block(_sub(sd, 'top_m_%d.' % i), hg)))
        tmp_out = conv(sd, 'l%d' % i, ll)
        if i < opt['num_stack'] - 1:
            previous = previous + conv(sd, 'bl%d' % i, ll) + conv(sd, 'al%d' % i, tmp_out)
    if taps is not None:
        taps['out'] = tmp_out
    return tmp_out
