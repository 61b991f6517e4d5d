"""Host-side checks of the vanilla-NeRF binding (no GPU): the ctypes table mirrors include/xrnerf_mi355_vanilla.h, the built library
exports its entry points, the ops wrappers refuse host tensors, and host tensors keep the tensor-op path of xrnerf_amd/vanilla.py."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signature_table_mirrors_the_header():
    from xrnerf_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_vanilla.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r'\bint\s+(xr_\w+)\s*\((.*?)\)\s*;', src, flags=re.S)}
    assert sorted(decls) == sorted(_lib.VANILLA_SIGNATURES)
    assert not set(_lib.VANILLA_SIGNATURES) & set(_lib.SIGNATURES)
    ctype = {'uint64_t': _lib._u64, 'uint32_t': _lib._u32, 'int': _lib._i32}
    for name, params in decls.items():
        want = []
        for p in params.split(','):
            p = p.strip()
            want.append(_lib._vp if '*' in p else ctype[p.split()[0]])
        res, args = _lib.VANILLA_SIGNATURES[name]
        assert res is _lib._i32 and args == want, name


def test_library_exports_the_entry_points():
    from xrnerf_amd import _lib
    lib = _lib.load()
    for name in _lib.VANILLA_SIGNATURES:
        assert getattr(lib, name).argtypes == _lib.VANILLA_SIGNATURES[name][1]
    from xrnerf_amd import ops
    assert ops.vanilla_kernels_available()


def test_ops_refuse_host_tensors():
    from xrnerf_amd import _lib, ops
    z = torch.linspace(2., 6., 8).expand(4, 8).contiguous()
    o = torch.zeros(4, 3)
    for call in (lambda: ops.nerf_encode(torch.zeros(4, 8, 3), torch.ones(4, 3), 10, 4),
                 lambda: ops.nerf_render_train_forward(torch.zeros(4, 8, 4), z, o + 1, True),
                 lambda: ops.nerf_render_backward(torch.zeros(4, 8, 4), z, o + 1, torch.zeros(4, 3), True),
                 lambda: ops.nerf_sample_pdf(z, torch.ones(4, 8), o, o + 1, 16)):
        with pytest.raises(_lib.XrError):
            call()


def test_host_tensors_keep_the_tensor_op_path():
    from xrnerf_amd import vanilla
    emb = vanilla.BaseEmbedder(multires=10, multires_dirs=4)
    pts, dirs = torch.randn(4, 8, 3), torch.nn.functional.normalize(torch.randn(4, 3), dim=-1)
    assert not emb._kernel_ok(pts, dirs)
    e = emb({'pts': pts, 'viewdirs': dirs})['embedded']
    assert tuple(e.shape) == (32, 90) and e.is_contiguous()
    mlp = vanilla.NerfMLP(skips=[2], netdepth=4, netwidth=32, embedder=dict(type='BaseEmbedder', multires=10, multires_dirs=4))
    assert not mlp._device_graph_ok(e)
