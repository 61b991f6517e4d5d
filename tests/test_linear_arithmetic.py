"""xr_linear_arithmetic / ops.linear_arithmetic / linear_act(..., exact=True): the calling thread's choice of arithmetic for the linear
kernels in front of XR_GEMM_F32.  The same body on the kernels' host build (tests/hip_emu) and on the MI355X:
  * mode 4 ('mfma') gives, bit for bit, what XR_GEMM_F32=mfma gives for the forward, the input gradient and the weight gradient -- and
    that is not what the default split arithmetic gives, so the override does select another kernel;
  * the context manager hands the previous mode back (nested, and when its body raises), after which the default's bits return;
  * a mode outside 0..4 is XR_EINVAL and leaves the mode as it was;
  * linear_act(exact=True) runs its forward and backward in that mode whatever the environment says."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'hip_emu'))


def _products(ops, x, w, b, dy):
    y = ops.linear_forward(x, w, b, True)
    return y, ops.linear_backward_input(dy, y, w), ops.linear_backward_weight(dy, y, x)


def check_arithmetic(dev, monkeypatch):
    from xrnerf_amd import _lib, linear, ops
    lib = _lib.load()
    monkeypatch.delenv('XR_GEMM_F32', raising=False)
    g = torch.Generator(device='cpu').manual_seed(5)
    M, N, K = 300, 64, 96
    x, w = torch.randn(M, K, generator=g).to(dev), (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b, dy = torch.randn(N, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
    default = _products(ops, x, w, b, dy)
    monkeypatch.setenv('XR_GEMM_F32', 'mfma')
    by_env = _products(ops, x, w, b, dy)
    monkeypatch.delenv('XR_GEMM_F32')
    assert lib.xr_linear_arithmetic(0) == 0                                   # the environment decides: the state every test starts from
    with ops.linear_arithmetic('mfma'):
        chosen = _products(ops, x, w, b, dy)
        with ops.linear_arithmetic('split2'):                                 # nested: the inner choice, then the outer one again
            inner = _products(ops, x, w, b, dy)
        again = _products(ops, x, w, b, dy)
    after = _products(ops, x, w, b, dy)
    for a, e, i, d, r, f in zip(chosen, by_env, inner, default, again, after):
        assert torch.equal(a, e), 'mode 4 is not the fp32-MFMA kernel of XR_GEMM_F32=mfma'
        assert torch.equal(i, d) and torch.equal(f, d), 'the previous mode did not come back'
        assert torch.equal(r, a)
    assert any(not torch.equal(a, d) for a, d in zip(chosen, default)), 'the override selected the same arithmetic as the default'
    # against float64: the chosen kernel is the exact-product one
    ref = torch.relu(x.double().cpu() @ w.double().cpu().t() + b.double().cpu())
    assert float((chosen[0].cpu().double() - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
    # a body that raises still restores the mode
    with pytest.raises(RuntimeError):
        with ops.linear_arithmetic('mfma'):
            raise RuntimeError('body')
    assert lib.xr_linear_arithmetic(0) == 0
    # bad modes: XR_EINVAL, the mode unchanged
    assert lib.xr_linear_arithmetic(3) == 0
    for bad in (-1, 5, 99):
        assert lib.xr_linear_arithmetic(bad) == -22
    assert lib.xr_linear_arithmetic(0) == 3
    with pytest.raises(KeyError):
        ops.linear_arithmetic('f64')
    # the autograd node: exact=True is the mfma mode forward and backward, under any environment
    monkeypatch.setenv('XR_GEMM_F32', 'split2')
    xs, ws = x.clone().requires_grad_(True), w.clone().requires_grad_(True)        # (no bias gradient: the weight gradient alone, as above)
    y = linear.linear_act(xs, ws, b, True, exact=True)
    (y * dy).sum().backward()
    assert torch.equal(y.detach(), by_env[0]) and torch.equal(xs.grad, by_env[1]) and torch.equal(ws.grad, by_env[2])
    assert lib.xr_linear_arithmetic(0) == 0


def test_arithmetic_override_on_the_host_build(monkeypatch):
    import emulib as E
    with E.emulated_ops() as edev:
        check_arithmetic(edev, monkeypatch)


@pytest.mark.gpu
def test_arithmetic_override_on_the_device(dev, monkeypatch):
    check_arithmetic(dev, monkeypatch)
