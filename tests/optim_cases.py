"""The bodies of the xr_adam_step_list / xr_log_window_add checks, shared by the GPU tier (tests/test_gpu_optim.py) and the host emulation of
the same source (tests/test_optim_host.py).

The reference of the list kernel is xr_adam_step_multi, the kernel every optimiser step went through before: both apply adam1 / ema1 of
csrc/xr_adam.h and both sources are compiled without fused multiply-adds, so p, m, v and ema must agree in every bit -- no tolerance.
The reference of the log window is numpy float64 sum(v n) / sum(n) in update order: an fp32 value times an integer below 2^29 is exact
in double and the order is fixed, so equality is exact as well."""
import numpy as np
import torch

LENGTHS = (70001, 5, 1025, 1, 255, 4, 1024, 3)        # the issue's set, in the order the tensors of a case take them
STEPS = 3


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def counts():
    from xrnerf_amd import ops
    cap = ops.adam_list_capacity()
    return (1, 4, 5, cap, cap + 1, 2 * cap + 3)


def _values(n, seed, dev, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(dev)


def check_fused_adam(dev, n_tensors, with_ema, grad_scale):
    """FusedAdam.step (the list kernel) against xr_adam_step_multi called tensor by tensor on aligned copies, STEPS steps.
    Tensor 0 is a view at a 4-byte offset into a larger buffer whose guard elements must stay as they are (its gradient is such a view
    too); with four tensors or more, tensor 1 never has a gradient (skipped, no state, step not advanced) and tensor 2 has none in the
    first step, so its step count differs from the others' afterwards: two groups."""
    from xrnerf_amd import ops
    from xrnerf_amd.train import FusedAdam
    assert ops.optim_kernels_available()
    lengths = [LENGTHS[i % len(LENGTHS)] for i in range(n_tensors)]
    GUARD = 5
    buf = _values(lengths[0] + 1 + GUARD, 1000, dev)
    buf0 = buf.clone()
    params = [torch.nn.Parameter(buf[1:1 + lengths[0]])] + [torch.nn.Parameter(_values(n, 1000 + i, dev)) for i, n in enumerate(lengths) if i > 0]
    assert params[0].data_ptr() % 16 == 4 and params[0].data_ptr() == buf.data_ptr() + 4
    kw = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-4)
    opt = FusedAdam(params, ema_momentum=0.05 if with_ema else None, ema_warm_up=10, **kw)
    # the reference's own copies: p, m, v, ema, step per tensor
    ref = [dict(p=p.detach().clone(), m=torch.zeros(p.numel(), device=dev), v=torch.zeros(p.numel(), device=dev), ema=p.detach().clone(), step=0)
           for p in params]
    never, late = (1, 2) if n_tensors >= 4 else (None, None)
    for it in range(STEPS):
        for i, p in enumerate(params):
            if i == never or (i == late and it == 0):
                p.grad = None
                continue
            g = _values(p.numel() + 1, 5000 + 97 * it + i, dev, scale=0.3)
            p.grad = g[1:] if i == 0 else g[1:].clone()              # tensor 0: the gradient at a 4-byte offset as well
            r = ref[i]
            r['step'] += 1
            mom = FusedAdam._ema_momentum(opt.param_groups[0], r['step']) if with_ema else 0.0
            ops.adam_step_multi([r['p']], [g[1:].clone()], [r['m']], [r['v']], r['step'], kw['lr'], kw['betas'][0], kw['betas'][1], kw['eps'],
                                kw['weight_decay'], [r['ema']] if with_ema else None, mom, grad_scale=grad_scale)
        opt.step(grad_scale=grad_scale)
    for i, (p, r) in enumerate(zip(params, ref)):
        if i == never:
            assert p not in opt.state or not opt.state[p], 'a tensor without a gradient got optimiser state'
            assert same_bits(p, r['p'])
            continue
        st = opt.state[p]
        assert st['step'] == r['step'] == (STEPS - 1 if i == late else STEPS), (i, st['step'], r['step'])
        for name, a, b in (('p', p, r['p']), ('m', st['m'], r['m']), ('v', st['v'], r['v'])) + ((('ema', st['ema'], r['ema']),) if with_ema else ()):
            assert same_bits(a, b), 'tensor %d (%d floats): %s differs from xr_adam_step_multi, max |d| = %g' % (
                i, p.numel(), name, float((a.detach().reshape(-1) - b.reshape(-1)).abs().max()))
        assert not same_bits(p, _values(p.numel(), 1000 + i, dev)) or i == 0, 'tensor %d was not updated' % i
    assert same_bits(buf[:1], buf0[:1]) and same_bits(buf[1 + lengths[0]:], buf0[1 + lengths[0]:]), 'guard elements around the view were written'
    assert not same_bits(buf[1:1 + lengths[0]], buf0[1:1 + lengths[0]])


def check_unaligned_each(dev, which):
    """ops.adam_step_list with ONE of p / g / m / v / ema at a 4-byte offset: same bits as the aligned call of xr_adam_step_multi, and
    the float on either side of the view untouched"""
    from xrnerf_amd import ops
    n = 1025
    names = ('p', 'g', 'm', 'v', 'ema')
    src = {k: _values(n, 40 + i, dev).abs() if k == 'v' else _values(n, 40 + i, dev) for i, k in enumerate(names)}
    ref = {k: t.clone() for k, t in src.items()}
    ops.adam_step_multi([ref['p']], [ref['g']], [ref['m']], [ref['v']], 2, 1e-2, 0.9, 0.99, 1e-8, 1e-3, [ref['ema']], 0.1, grad_scale=0.5)
    hold = {}
    for k in names:
        if k == which:
            hold[k] = torch.full((n + 2,), 7.0, device=dev)
            hold[k][1:n + 1] = src[k]
            src[k] = hold[k][1:n + 1]
            assert src[k].data_ptr() % 16 == 4
    ops.adam_step_list([src['p']], [src['g']], [src['m']], [src['v']], 2, 1e-2, 0.9, 0.99, 1e-8, 1e-3, [src['ema']], 0.1, grad_scale=0.5)
    for k in ('p', 'm', 'v', 'ema'):
        assert same_bits(src[k], ref[k]), k
    assert float(hold[which][0]) == 7.0 and float(hold[which][n + 1]) == 7.0


def check_single_lengths(dev):
    """every length of the issue's set on its own, one launch each"""
    from xrnerf_amd import ops
    for n in LENGTHS:
        a = [_values(n, 60 + i, dev) for i in range(3)] + [_values(n, 63, dev).abs()]
        b = [t.clone() for t in a]
        ops.adam_step_multi([a[0]], [a[1]], [a[2]], [a[3]], 1, 1e-2, 0.9, 0.99, 1e-15, 1e-6)
        ops.adam_step_list([b[0]], [b[1]], [b[2]], [b[3]], 1, 1e-2, 0.9, 0.99, 1e-15, 1e-6)
        for x, y in zip(a, b):
            assert same_bits(x, y), n


def check_refusals(dev):
    from xrnerf_amd import _lib, ops
    import pytest
    t = [_values(8, i, dev) for i in range(4)]
    with pytest.raises(_lib.XrError):
        ops.adam_step_list(t[:1], t[1:2], t[2:3], t[3:4], 0)                                   # step < 1
    with pytest.raises(_lib.XrError):
        ops.adam_step_list([t[0][:0]], [t[1][:0]], [t[2][:0]], [t[3][:0]], 1)                # an empty tensor
    with pytest.raises(_lib.XrError):
        ops.log_window_add([torch.zeros(1, device=dev)], 1 << 29, torch.zeros(32, dtype=torch.float64, device=dev))
    with pytest.raises(_lib.XrError):
        ops.log_window_add([torch.zeros(1, device=dev)] * 17, 1, torch.zeros(32, dtype=torch.float64, device=dev))


# ------------------------------------------------------------------------------------------ the log window
LOG_NUM_SAMPLES = (1, 4096, 3, 4096, 1)
LOG_NAMES = ('loss', 'psnr', 'L2 reg')


def _log_values(window):
    rng = np.random.RandomState(7 + window)
    return (rng.standard_normal((len(LOG_NUM_SAMPLES), len(LOG_NAMES))) * [1.0, 30.0, 1e-4]).astype(np.float32)


def _expected(v):
    out = {}
    for j, name in enumerate(LOG_NAMES):
        sv, sn = np.float64(0), np.float64(0)
        for i, n in enumerate(LOG_NUM_SAMPLES):
            sv = sv + np.float64(v[i, j]) * np.float64(n)
            sn = sn + np.float64(n)
        out[name] = float(sv / sn)
    return out


def check_log_window(dev):
    """5 iterations of 3 scalars with num_samples in {1, 4096, 3}, read(); a second window starts from zero; the host-float path gives
    the same value"""
    from xrnerf_amd import ops
    from xrnerf_amd.runner import LogWindow
    assert ops.optim_kernels_available()
    on_device, on_host = LogWindow(), LogWindow()
    for window in range(2):
        v = _log_values(window)
        for i, n in enumerate(LOG_NUM_SAMPLES):
            on_device.update({name: torch.tensor(v[i, j], device=dev) for j, name in enumerate(LOG_NAMES)}, n)
            on_host.update({name: float(v[i, j]) for j, name in enumerate(LOG_NAMES)}, n)
        assert on_device.window is not None and not on_device.host, 'the device scalars did not go through the device window'
        want = _expected(v)
        got_d, got_h = on_device.read(), on_host.read()
        assert list(got_d) == list(LOG_NAMES) and got_d == want, (window, got_d, want)
        assert got_h == want, (window, got_h, want)
        assert float(on_device.window.abs().sum()) == 0.0
    assert on_device.read() == {} and on_host.read() == {}
