"""GNR's image encoder (configs/gnr/gnr_genebody.py: image_filter = HGFilter; the reference's embedders/gnr_embedder.py:16-80 and
180-387) on the kernels of csrc/xr_gnr_encoder.hip:

    ConvBlock, HourGlass, HGFilter, SRFilters   the reference's modules: same constructor arguments, parameter names and shapes (a
                                                reference checkpoint loads with strict=True), registered with the builder

Device tensors that need no gradient run the kernels on channel-last maps: GroupNorm + ReLU ride on the next convolution's loads,
ConvBlock's three convolutions write the column ranges of one buffer (no cat), its residual is the 1x1 downsample convolution adding
to that buffer (or one add), the hourglass's `up1 + up2` rides on the bicubic upsampling, and `previous + ll + tmp_out_` is two 1x1
convolutions adding to `previous`.  HGFilter returns a [V, C, h, w] VIEW of the channel-last buffer its last layer wrote, so
gnr_render.channel_last() of it is that buffer.  Host tensors, and any call that needs a gradient (train_encoder), take the tensor-op
path: the reference's graph in torch ops."""
import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .builder import EMBEDDERS

TENSOR_OPS = False               # measurements only: device tensors take the tensor-op path too


def _use_kernels(x, module):
    """device tensors without a gradient to carry run the kernels; a library handle without the entry points is an error"""
    if TENSOR_OPS or not ops._on_device(x):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters())):
        return False
    if not ops.gnr_encoder_kernels_available():
        from . import _lib
        raise _lib.XrError('the loaded library has no xr_gnr_encoder entry points (stale build?)')
    return True


def _norm(norm, channels):
    if norm == 'group':
        return nn.GroupNorm(32, channels)
    if norm == 'batch':
        raise NotImplementedError("norm='batch' is not built: the GNR configuration uses norm='group'")
    raise ValueError('unknown norm %r' % (norm,))


def _w(conv):
    """the convolution's weight in the kernels' [k k Cin, Cout] layout: re-laid when the parameter changes (load_state_dict, an optimizer
    step, .to(device): its version counter or address moves), not per call.  A write through `.data` moves neither."""
    w = conv.weight
    c = conv.__dict__.get('_xr_relaid')
    if c is None or c[0] != w._version or c[1] != w.data_ptr() or c[2].device != w.device:
        c = (w._version, w.data_ptr(), ops.hg_relay_weight(w))
        conv.__dict__['_xr_relaid'] = c
    return c[2]


def _p(t):
    return t.detach().contiguous()


def _gn(stats, gn):
    return (stats[0], stats[1], _p(gn.weight), _p(gn.bias))


def _conv_k(conv, x, norm=None, out=None, accumulate=False):
    return ops.hg_conv2d(x, _w(conv), conv.kernel_size[0], conv.stride[0], norm, _p(conv.bias) if conv.bias is not None else None, False, out,
                         accumulate)


def _last(x):
    """[N, C, H, W] -> a fresh contiguous channel-last [N, H, W, C]"""
    return x.detach().float().permute(0, 2, 3, 1).contiguous()


@EMBEDDERS.register_module()
class ConvBlock(nn.Module):
    """gnr_embedder.py:26-79.  `bn4` exists whether used or not; with a downsample its parameters appear a second time in the
    state_dict as downsample.0.*, as in the reference."""

    def __init__(self, in_planes, out_planes, norm='batch'):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, int(out_planes / 2), kernel_size=3, stride=1, padding=1, bias=False)
        self.conv2 = nn.Conv2d(int(out_planes / 2), int(out_planes / 4), kernel_size=3, stride=1, padding=1, bias=False)
        self.conv3 = nn.Conv2d(int(out_planes / 4), int(out_planes / 4), kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = _norm(norm, in_planes)
        self.bn2 = _norm(norm, int(out_planes / 2))
        self.bn3 = _norm(norm, int(out_planes / 4))
        self.bn4 = _norm(norm, in_planes)
        if in_planes != out_planes:
            self.downsample = nn.Sequential(self.bn4, nn.ReLU(True), nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=1, bias=False))
        else:
            self.downsample = None

    def forward(self, x):
        if _use_kernels(x, self):
            return self.forward_last(_last(x)).permute(0, 3, 1, 2)
        out1 = self.conv1(F.relu(self.bn1(x)))
        out2 = self.conv2(F.relu(self.bn2(out1)))
        out3 = self.conv3(F.relu(self.bn3(out2)))
        residual = self.downsample(x) if self.downsample is not None else x
        return torch.cat((out1, out2, out3), 1) + residual

    def forward_last(self, x):
        """kernel path: x [N, H, W, Cin] channel-last (left unchanged) -> a fresh [N, H, W, Cout].  One call (xr_hg_conv_block): the
        three convolutions write the column ranges of the output, bn1 and bn4 share the statistics of x, and the residual comes last,
        after conv2 and conv3 have read out1 and out2 as they were"""
        ds = self.downsample[2] if self.downsample is not None else None
        return ops.hg_conv_block(x, (_w(self.conv1), _w(self.conv2), _w(self.conv3), _w(ds) if ds is not None else None),
                                 [_p(t) for bn in (self.bn1, self.bn2, self.bn3, self.bn4) for t in (bn.weight, bn.bias)])


@EMBEDDERS.register_module()
class HourGlass(nn.Module):
    """gnr_embedder.py:209-270"""

    def __init__(self, num_modules, depth, num_features, norm='batch'):
        super().__init__()
        self.num_modules, self.depth, self.features, self.norm = num_modules, depth, num_features, norm
        self._generate_network(self.depth)

    def _generate_network(self, level):
        self.add_module('b1_' + str(level), ConvBlock(self.features, self.features, norm=self.norm))
        self.add_module('b2_' + str(level), ConvBlock(self.features, self.features, norm=self.norm))
        if level > 1:
            self._generate_network(level - 1)
        else:
            self.add_module('b2_plus_' + str(level), ConvBlock(self.features, self.features, norm=self.norm))
        self.add_module('b3_' + str(level), ConvBlock(self.features, self.features, norm=self.norm))

    def _check(self, h, w):
        if h % (1 << self.depth) or w % (1 << self.depth):
            raise ValueError('an hourglass of depth %d needs a map whose sides are multiples of %d, got %d x %d' % (self.depth, 1 << self.depth, h, w))

    def _forward(self, level, inp):
        up1 = self._modules['b1_' + str(level)](inp)
        low1 = self._modules['b2_' + str(level)](F.avg_pool2d(inp, 2, stride=2))
        low2 = self._forward(level - 1, low1) if level > 1 else self._modules['b2_plus_' + str(level)](low1)
        low3 = self._modules['b3_' + str(level)](low2)
        return up1 + F.interpolate(low3, scale_factor=2, mode='bicubic', align_corners=True)

    def _forward_last(self, level, inp):
        up1 = self._modules['b1_' + str(level)].forward_last(inp)
        low1 = self._modules['b2_' + str(level)].forward_last(ops.hg_avgpool2(inp))
        low2 = self._forward_last(level - 1, low1) if level > 1 else self._modules['b2_plus_' + str(level)].forward_last(low1)
        low3 = self._modules['b3_' + str(level)].forward_last(low2)
        return ops.hg_bicubic_up2(low3, addend=up1, out=up1)

    def forward_last(self, x):
        self._check(x.shape[1], x.shape[2])
        return self._forward_last(self.depth, x)

    def forward(self, x):
        self._check(x.shape[2], x.shape[3])
        if _use_kernels(x, self):
            return self.forward_last(_last(x)).permute(0, 3, 1, 2)
        return self._forward(self.depth, x)


@EMBEDDERS.register_module()
class HGFilter(nn.Module):
    """gnr_embedder.py:273-387: images [V, 3, H, W] -> [V, hourglass_dim, H / 4, W / 4]; H and W multiples of 4 * 2^num_hourglass"""

    def __init__(self, opt):
        super().__init__()
        self.num_modules = opt.num_stack
        self.opt = opt
        if opt.norm == 'batch':
            raise NotImplementedError("norm='batch' is not built: the GNR configuration uses norm='group'")
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3)
        self.bn1 = _norm(opt.norm, 64)
        if opt.hg_down == 'conv64':
            self.conv2 = ConvBlock(64, 64, opt.norm)
            self.down_conv2 = nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1)
        elif opt.hg_down == 'conv128':
            self.conv2 = ConvBlock(64, 128, opt.norm)
            self.down_conv2 = nn.Conv2d(128, 128, kernel_size=3, stride=2, padding=1)
        elif opt.hg_down == 'ave_pool':
            self.conv2 = ConvBlock(64, 128, opt.norm)
        else:
            raise NameError('Unknown Fan Filter setting!')
        self.conv3 = ConvBlock(128, 128, opt.norm)
        self.conv4 = ConvBlock(128, 256, opt.norm)
        for i in range(self.num_modules):
            self.add_module('m' + str(i), HourGlass(1, opt.num_hourglass, 256, opt.norm))
            self.add_module('top_m_' + str(i), ConvBlock(256, 256, opt.norm))
            self.add_module('conv_last' + str(i), nn.Conv2d(256, 256, kernel_size=1, stride=1, padding=0))
            self.add_module('bn_end' + str(i), _norm(opt.norm, 256))
            self.add_module('l' + str(i), nn.Conv2d(256, opt.hourglass_dim, kernel_size=1, stride=1, padding=0))
            if i < self.num_modules - 1:
                self.add_module('bl' + str(i), nn.Conv2d(256, 256, kernel_size=1, stride=1, padding=0))
                self.add_module('al' + str(i), nn.Conv2d(opt.hourglass_dim, 256, kernel_size=1, stride=1, padding=0))

    def _check(self, x):
        m = 4 << self.opt.num_hourglass
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % m or x.shape[3] % m:
            raise ValueError('HGFilter takes [V, 3, H, W] images with H and W multiples of %d, got %r' % (m, tuple(x.shape)))

    def forward(self, x, taps=None):
        """taps: a dict that receives the outputs of conv4, m0 and the filter as [V, C, h, w] (the fixture's three tensors)"""
        self._check(x)
        if _use_kernels(x, self):
            return self._forward_kernels(x, taps)
        m = self._modules
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.avg_pool2d(self.conv2(x), 2, stride=2) if self.opt.hg_down == 'ave_pool' else self.down_conv2(self.conv2(x))
        previous = self.conv4(self.conv3(x))
        if taps is not None:
            taps['conv4'] = previous
        for i in range(self.num_modules):
            hg = m['m' + str(i)](previous)
            if taps is not None and i == 0:
                taps['m0'] = hg
            ll = F.relu(m['bn_end' + str(i)](m['conv_last' + str(i)](m['top_m_' + str(i)](hg))))
            tmp_out = m['l' + str(i)](ll)
            if i < self.num_modules - 1:
                previous = previous + m['bl' + str(i)](ll) + m['al' + str(i)](tmp_out)
        if taps is not None:
            taps['out'] = tmp_out
        return tmp_out

    def _forward_kernels(self, images, taps=None):
        m = self._modules
        nchw = lambda t: t.clone().permute(0, 3, 1, 2)
        x = _conv_k(self.conv1, _last(images))                                     # the 3-channel stem reads element by element
        ops.hg_gn_relu(x, *_gn(ops.hg_gn_stats(x), self.bn1), out=x)
        x = self.conv2.forward_last(x)
        x = ops.hg_avgpool2(x) if self.opt.hg_down == 'ave_pool' else _conv_k(self.down_conv2, x)
        previous = self.conv4.forward_last(self.conv3.forward_last(x))
        if taps is not None:
            taps['conv4'] = nchw(previous)
        for i in range(self.num_modules):
            hg = m['m' + str(i)].forward_last(previous)
            if taps is not None and i == 0:
                taps['m0'] = nchw(hg)
            ll = _conv_k(m['conv_last' + str(i)], m['top_m_' + str(i)].forward_last(hg))
            end = _gn(ops.hg_gn_stats(ll), m['bn_end' + str(i)])                   # relu(bn_end(.)) rides on the loads of `l` and `bl`
            tmp_out = _conv_k(m['l' + str(i)], ll, end)
            if i < self.num_modules - 1:                                           # previous + bl(ll) + al(tmp_out), in that order
                _conv_k(m['bl' + str(i)], ll, end, out=previous, accumulate=True)
                _conv_k(m['al' + str(i)], tmp_out, out=previous, accumulate=True)
        out = tmp_out.permute(0, 3, 1, 2)
        if taps is not None:
            taps['out'] = out
        return out


@EMBEDDERS.register_module()
class SRFilters(nn.Module):
    """gnr_embedder.py:180-206 (use_feat_sr; off in the GNR configuration): tensor ops only"""

    def __init__(self, order=2, in_ch=256, out_ch=128):
        super().__init__()
        self.in_ch, self.out_ch = in_ch, out_ch
        self.image_factor = [0.5 ** (order - i) for i in range(0, order + 1)]
        self.convs = nn.ModuleList([nn.Conv2d(in_ch + 3, out_ch, kernel_size=3, padding=1)] +
                                   [nn.Conv2d(out_ch + 3, out_ch, kernel_size=3, padding=1) for i in range(order)])

    def forward(self, feat, images):
        for i, conv in enumerate(self.convs):
            # the reference tests `factor is not 1` and `i is not 0`: a float factor is never the int 1, so the images pass through
            # interpolate at factor 1.0 as well (the identity up to rounding)
            im = F.interpolate(images, scale_factor=self.image_factor[i], mode='bicubic', align_corners=True)
            if i != 0:
                feat = F.interpolate(feat, scale_factor=2, mode='bicubic', align_corners=True)
            feat = conv(torch.cat([feat, im], dim=1))
        return feat
