"""TEST INFRASTRUCTURE: restatements of the Animatable-NeRF stages of xrnerf_amd/csrc/xr_aninerf.hip in torch on the host.
float64 versions of stages 1-5 (autograd through them gives the backward references), and the float32 restatement of the
nearest-vertex query, whose every operation is one un-fused fp32 tensor op in the kernel's order: the kernel must match it bit for bit."""
import math

import numpy as np
import torch

J = 24


def t64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def t32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------ 1. closest vertex
def to_pose(p, R, T):
    """q_j = sum_k (p_k - T_k) R_kj, k ascending (any dtype; one rounding per operation)"""
    d = p - T.reshape(1, 3)
    return (d[:, 0:1] * R[0] + d[:, 1:2] * R[1]) + d[:, 2:3] * R[2]


def d2_matrix(q, v):
    """[N, V] of (dx dx + dy dy) + dz dz"""
    d = q[:, None, :] - v[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def closest32(pts, verts, th, R=None, T=None):
    """float32: -> q [N,3], idx [N] (lowest index on a tie), d2 [N], dist [N], flag [N] bool"""
    q, v = t32(pts), t32(verts)
    if R is not None:
        q, v = to_pose(q, t32(R), t32(T)), to_pose(v, t32(R), t32(T))
    dd = d2_matrix(q, v)
    m = dd.min(1)[0]
    idx = (dd == m[:, None]).to(torch.uint8).argmax(1)               # the FIRST entry that equals the minimum
    # numpy's sqrt is the hardware's correctly rounded one, as sqrtf is required to be; torch's vectorised host sqrt is not always
    dist = torch.from_numpy(np.sqrt(m.numpy()))
    return q, idx, m, dist, dist < torch.tensor(th, dtype=torch.float32)


def closest64(pts, verts, R=None, T=None):
    """float64 on the float32 inputs: -> idx [N], gap [N] = second smallest d2 - smallest (inf with one vertex), dist [N]"""
    q, v = t64(pts), t64(verts)
    if R is not None:
        q, v = to_pose(q, t64(R), t64(T)), to_pose(v, t64(R), t64(T))
    dd = d2_matrix(q, v)
    s, order = torch.sort(dd, dim=1)
    gap = s[:, 1] - s[:, 0] if dd.shape[1] > 1 else torch.full((dd.shape[0],), float('inf'), dtype=torch.float64)
    return order[:, 0], gap, torch.sqrt(s[:, 0])


# ------------------------------------------------------------------------------------------ 2. selection
def select(flag, dist):
    """pind = flag; pind[argmin(dist)] = True (the first minimum) -> nonzero(pind)"""
    pind = torch.as_tensor(flag).bool().clone()
    dist = torch.as_tensor(dist)
    if pind.numel():
        first = int((dist == dist.min()).to(torch.uint8).argmax())
        pind[first] = True
    return pind.nonzero()[:, 0]


# ------------------------------------------------------------------------------------------ 3. blend head
def blend(smpl_bw, idx, logits):
    """softmax_j(log(smpl_bw[idx] + 1e-9) + logits); smpl_bw / logits float64 tensors"""
    return torch.softmax(torch.log(smpl_bw[torch.as_tensor(idx).long()] + 1e-9) + logits, dim=1)


# ------------------------------------------------------------------------------------------ 4. skinning
def skin(pts, dirs, bw, a_from, a_to):
    """the reference's composition (utils/aninerf.py:41-100) in the [N,24] layout, any dtype"""
    A = (bw @ a_from.reshape(J, 16)).view(-1, 4, 4)
    B = (bw @ a_to.reshape(J, 16)).view(-1, 4, 4)
    r_inv = torch.inverse(A[:, :3, :3])
    p = torch.sum(r_inv * (pts - A[:, :3, 3])[:, None], dim=2)
    p = torch.sum(B[:, :3, :3] * p[:, None], dim=2) + B[:, :3, 3]
    if dirs is None:
        return p, None
    d = torch.sum(r_inv * dirs[:, None], dim=2)
    return p, torch.sum(B[:, :3, :3] * d[:, None], dim=2)


# ------------------------------------------------------------------------------------------ 5. positional encoding
def embed(p, L):
    """BaseEmbedder.run_embed: [p, sin(2^0 p), cos(2^0 p), ..]"""
    parts = [p]
    for k in range(L):
        parts += [torch.sin(p * 2.0 ** k), torch.cos(p * 2.0 ** k)]
    return torch.cat(parts, -1)


# ------------------------------------------------------------------------------------------ fixture parameters
def formula_tensor(key, shape, seed):
    """the value of state-dict entry `key` in tests/golden/ref_aninerf.npz's networks: a function of (key, shape, seed), so that the
    fixture stores no weights (the AN_* widths are hard-wired to 256: 2 M parameters).  Weights ~ N(0, 2 / fan_in), weight-norm gains
    around the rows' norm, small biases (the density head's, `lin8.bias`, centred at 0.4 so that about half of the alphas are positive),
    latent codes ~ N(0, 0.3^2)."""
    import zlib
    rng = np.random.default_rng([zlib.crc32(key.encode()), int(seed)])
    shape = tuple(int(s) for s in shape)
    if key.endswith('latent.weight'):
        a = rng.normal(0, 0.3, shape)
    elif key.endswith('weight_g'):
        a = math.sqrt(2.0) * rng.uniform(0.8, 1.2, shape)
    elif key.endswith('bias'):
        a = rng.normal(0.4 if key.endswith('lin8.bias') else 0.0, 0.05, shape)
    else:
        a = rng.normal(0, math.sqrt(2.0 / shape[1]), shape)
    return torch.as_tensor(a.astype(np.float32))


def formula_state_dict(keys, shapes, seed):
    return {k: formula_tensor(k, s, seed) for k, s in zip(keys, shapes)}


def sample_positions(key, numel, n=256):
    """the flat positions at which the fixture stores a gradient tensor's entries: all of them up to n, else n seeded draws"""
    import zlib
    if numel <= n:
        return np.arange(numel)
    return np.sort(np.random.default_rng([zlib.crc32(key.encode()), 77]).choice(numel, n, replace=False))
