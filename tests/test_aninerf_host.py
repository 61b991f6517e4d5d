"""Host-side checks of the Animatable-NeRF binding (no GPU): the ctypes table mirrors include/xrnerf_mi355_aninerf.h one to one and is
disjoint from the other tables, the built library exports its entry points, the ops wrappers refuse host tensors, and host tensors keep
the tensor-op path of xrnerf_amd/aninerf.py."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signature_table_mirrors_the_header():
    from xrnerf_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'xrnerf_mi355_aninerf.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    decls = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r'\b(int|size_t)\s+(xr_\w+)\s*\((.*?)\)\s*;', src, flags=re.S)}
    assert sorted(decls) == sorted(_lib.ANINERF_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.BUNGEE_SIGNATURES, _lib.VANILLA_SIGNATURES):
        assert not set(_lib.ANINERF_SIGNATURES) & set(other)
    ctype = {'uint64_t': _lib._u64, 'uint32_t': _lib._u32, 'int': _lib._i32, 'size_t': _lib._sz, 'float': _lib._f}
    for name, (ret, params) in decls.items():
        want = []
        for p in params.split(','):
            p = p.strip()
            want.append(_lib._vp if '*' in p else ctype[p.split()[0]])
        res, args = _lib.ANINERF_SIGNATURES[name]
        assert res is ctype[ret] and args == want, name


def test_library_exports_the_entry_points():
    from xrnerf_amd import _lib
    lib = _lib.load()
    for name in _lib.ANINERF_SIGNATURES:
        assert getattr(lib, name).argtypes == _lib.ANINERF_SIGNATURES[name][1]
    from xrnerf_amd import ops
    assert ops.aninerf_kernels_available()
    assert lib.xr_ani_select_workspace_bytes(1000) == (4 * 4 + 1) * 4


def test_ops_refuse_host_tensors():
    from xrnerf_amd import _lib, ops
    p, bw = torch.zeros(4, 3), torch.full((4, 24), 1 / 24.)
    A = torch.eye(4).expand(24, 4, 4).contiguous()
    i = torch.zeros(4, dtype=torch.int32)
    for call in (lambda: ops.ani_closest(p, torch.ones(5, 3), 0.05),
                 lambda: ops.ani_select(i, torch.zeros(4)),
                 lambda: ops.ani_blend_forward(bw, i, bw),
                 lambda: ops.ani_blend_backward(bw, bw),
                 lambda: ops.ani_skin_forward(p, p, bw, A, A),
                 lambda: ops.ani_skin_backward(p, p, bw, A, A, p, p),
                 lambda: ops.ani_encode_backward(p, torch.zeros(4, 39), 6)):
        with pytest.raises(_lib.XrError):
            call()


def test_host_tensors_keep_the_tensor_op_path():
    from xrnerf_amd import aninerf
    d = aninerf.synthetic_body(64, 1, n_rays=6, n_samples=8)
    assert not aninerf._kernels(d['pts'])
    q, idx, dist, flag = aninerf.closest(d['pts'].reshape(-1, 3), d['smpl_verts'], 0.05, d['smpl_R'], d['smpl_T'])
    sel = aninerf.select(flag, dist)
    assert idx.dtype == torch.int32 and sel.numel() >= 1 and bool((sel[1:] > sel[:-1]).all())
    bw = aninerf.blend_head(torch.zeros(sel.numel(), 24, requires_grad=True), d['smpl_bw'], idx[sel])
    p, dd = aninerf.skin(q[sel], q[sel], bw, d['A'], d['big_A'])
    assert p.requires_grad and tuple(dd.shape) == (sel.numel(), 3)
    assert tuple(aninerf.embed(p, 6).shape) == (sel.numel(), 39)


def test_synthetic_body_has_sparse_weights_and_well_conditioned_blends():
    from xrnerf_amd import aninerf
    d = aninerf.synthetic_body(257, 3)
    bw = d['smpl_bw'].double()
    assert bool((d['smpl_bw'] == 0).any()) and float((bw.sum(1) - 1).abs().max()) < 1e-6
    for k in ('A', 'big_A'):
        R = (bw @ d[k].double().reshape(24, 16)).view(-1, 4, 4)[:, :3, :3]
        assert float(torch.linalg.det(R).min()) > 0.2 and float(torch.linalg.cond(R).max()) < 3.0
