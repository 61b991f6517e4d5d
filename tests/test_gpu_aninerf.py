"""Animatable NeRF on the device: the kernels of xrnerf_amd/csrc/xr_aninerf.hip (xr_ani_closest, xr_ani_select, xr_ani_blend_forward /
_backward, xr_ani_skin_forward / _backward, xr_ani_encode_backward) against the restatements of tests/aninerf_restatement.py, and the
registry modules of xrnerf_amd/aninerf.py over them against one `train_pose` and one `novel_pose` step of the reference's own modules
(tests/golden/ref_aninerf.npz, made by tests/golden/make_golden_aninerf.py).

The bodies are `check_*(dev, ...)` functions: tests/test_emu_aninerf.py runs the same bodies on the CPU through the HIP-on-CPU shim.

Bars.  Closest vertex: bit for bit against the fp32 restatement (index, d2, dist, flag, transformed point); against float64 the index
wherever the d2 gap is >= 1e-6, and at most 1 % of a case below that gap.  Selection: bit for bit.  Blend head: 2e-6 forward (outputs
<= 1: logf / expf at ~2 ulp and a 24-term sum), rows sum to 1 within 1e-6, backward 1e-5 max|ref|.  Skinning: 1e-5 max(1, |ref|)
forward, 1e-5 max|ref| backward; a one-hot rotation is inverted to 2e-6.  Encode backward: 1e-5 max|ref|.  (The fp32-stage bars of
test_gpu_vanilla.py / test_gpu_mip.py.)  Fixture steps: pind and the chosen rows identical, tpose / pbw / tbw 1e-5, raw
grad_bars.RAW_BAR of max|raw|, losses 1e-5 relative, sampled gradients and norms conftest.grad_close."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')
pytestmark = pytest.mark.gpu

TILE = 1024                                   # XR_ANI_CLOSEST_TILE
N_SHAPES = [1, 63, 65, 130]
V_SHAPES = [1, 24, TILE + 1, 6890]
TH = 0.05


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'ref_aninerf.npz'))


def _dt(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


_BODIES = {}


def body(V):
    """xrnerf_amd.aninerf.synthetic_body(V, seed V) as numpy arrays, computed once per V and shared"""
    if V not in _BODIES:
        from xrnerf_amd.aninerf import synthetic_body
        _BODIES[V] = {k: v.numpy() for k, v in synthetic_body(V, V).items()}
    return _BODIES[V]


def queries(N, V, seed=0):
    """N world-space points: a quarter within 0.02 of a vertex, the rest uniform in the body's bounds + 0.05"""
    b = body(V)
    rng = np.random.default_rng(100000 * seed + 1000 * N + V)
    w = b['smpl_verts']
    lo, hi = w.min(0) - 0.05, w.max(0) + 0.05
    p = rng.uniform(lo, hi, (N, 3))
    near = rng.uniform(0, 1, N) < 0.25
    off = rng.normal(0, 1, (N, 3))
    off = off / np.linalg.norm(off, axis=-1, keepdims=True) * rng.uniform(0, 0.02, (N, 1))
    p[near] = (w[rng.integers(0, V, N)] + off)[near]
    return p.astype(np.float32)


# ------------------------------------------------------------------------------------------ 1. closest vertex
def _closest_case(dev, pts, verts, R, T, what, tied=()):
    """tied: points placed on a duplicated vertex (a float64 gap of 0 by construction), left out of the 1 % count"""
    import aninerf_restatement as RS
    from xrnerf_amd import ops
    q, idx, dist, flag, d2 = ops.ani_closest(_dt(pts, dev), _dt(verts, dev), TH, None if R is None else _dt(R, dev),
                                             None if T is None else _dt(T, dev), want_d2=True)
    rq, ridx, rd2, rdist, rflag = RS.closest32(pts, verts, TH, R, T)
    assert np.array_equal(_np(q).view(np.uint32), rq.numpy().view(np.uint32)), what
    assert np.array_equal(_np(idx).astype(np.int64), ridx.numpy()), what
    assert np.array_equal(_np(d2).view(np.uint32), rd2.numpy().view(np.uint32)), what
    assert np.array_equal(_np(dist).view(np.uint32), rdist.numpy().view(np.uint32)), what
    assert np.array_equal(_np(flag) != 0, rflag.numpy()), what
    i64, gap, _ = RS.closest64(pts, verts, R, T)
    clear = gap.numpy() >= 1e-6
    print('%s: %d of %d points under the 1e-6 gap, %d near' % (what, int((~clear).sum()), len(clear), int(rflag.sum())))
    assert np.delete(~clear, list(tied)).mean() <= 0.01, what
    assert np.array_equal(_np(idx).astype(np.int64)[clear], i64.numpy()[clear]), what
    return idx, dist, flag


def check_closest(dev, N, V):
    b = body(V)
    pts = queries(N, V)
    _closest_case(dev, pts, b['smpl_verts'], b['smpl_R'], b['smpl_T'].reshape(3), 'N=%d V=%d with (R, T)' % (N, V))
    _closest_case(dev, pts, b['smpl_verts'], None, None, 'N=%d V=%d' % (N, V))


def check_closest_edges(dev):
    from xrnerf_amd import ops
    b = body(257)
    verts = b['canonical_smpl_verts'].copy()
    verts[200] = verts[31]                       # a duplicated vertex: the lowest index wins
    pts = queries(65, 257)
    pts[0] = verts[200] + np.float32(1e-3)
    pts[1] = verts[77]                           # a point exactly on a vertex
    idx, dist, flag = _closest_case(dev, pts, verts, None, None, 'duplicate / on-vertex', tied=(0,))
    assert int(idx[0]) == 31
    assert int(idx[1]) == 77 and float(dist[1]) == 0.0 and int(flag[1]) == 1
    # no points: a no-op
    q, idx, dist, flag = ops.ani_closest(_dt(pts[:0], dev), _dt(verts, dev), TH)
    assert idx.numel() == 0 and dist.numel() == 0 and tuple(q.shape) == (0, 3)


# ------------------------------------------------------------------------------------------ 2. selection
def check_select(dev):
    import aninerf_restatement as RS
    from xrnerf_amd import ops
    rng = np.random.default_rng(5)

    def run(flag, dist, what):
        f, d = torch.as_tensor(flag.astype(np.int32)).to(dev), _dt(dist, dev)
        lst, count = ops.ani_select(f, d)
        n = int(count.item())
        want = RS.select(flag, dist.astype(np.float32)).numpy()
        assert n == len(want), what
        assert np.array_equal(_np(lst[:n]).astype(np.int64), want), what
        lst2, count2 = ops.ani_select(f, d)                           # the same list on a second run
        assert torch.equal(count2, count) and torch.equal(lst2[:n], lst[:n]), what
        return want

    for N in (1, 63, 130, 1000, 70000):                               # 70000: 274 workgroups, two sweeps of the count scan
        dist = rng.uniform(0.0, 0.3, N)
        run(dist < TH, dist, 'random N=%d' % N)
    dist = rng.uniform(0.1, 0.3, 1000)
    dist[[700, 300]] = 0.07                                           # no point near: the list is the argmin alone, the lower of a tie
    assert run(np.zeros(1000, bool), dist, 'none near').tolist() == [300]
    assert len(run(np.ones(1000, bool), dist, 'all near')) == 1000
    assert run(np.zeros(1, bool), dist[:1], 'N=1').tolist() == [0]
    flag = dist < 0.2
    flag[300] = False                                                 # the argmin is forced in between flagged points
    got = run(flag, dist, 'forced in the middle')
    assert 300 in got.tolist()
    lst, count = ops.ani_select(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, device=dev))
    assert int(count.item()) == 0


# ------------------------------------------------------------------------------------------ 3. blend head
def check_blend(dev, N):
    import aninerf_restatement as RS
    from xrnerf_amd import ops
    b = body(257)
    bw = b['smpl_bw']
    assert (bw == 0).any()                                             # exact zeros, as real SMPL weights have
    rng = np.random.default_rng(N)
    idx = rng.integers(0, 257, N)
    idx[0] = int(np.argmax((bw == 0).sum(1)))
    logits = rng.normal(0, 2, (N, 24)).astype(np.float32)
    g = rng.normal(0, 1, (N, 24)).astype(np.float32)
    out = ops.ani_blend_forward(_dt(bw, dev), torch.as_tensor(idx.astype(np.int32)).to(dev), _dt(logits, dev))
    l64 = RS.t64(logits).requires_grad_(True)
    want = RS.blend(RS.t64(bw), idx, l64)
    (want * RS.t64(g)).sum().backward()
    got = _np(out).astype(np.float64)
    e_f, e_s = np.abs(got - want.detach().numpy()).max(), np.abs(got.sum(1) - 1).max()
    dl = ops.ani_blend_backward(out, _dt(g, dev))
    ref = l64.grad.numpy()
    e_b = np.abs(_np(dl) - ref).max()
    print('blend N=%d: forward %.3g, row sums %.3g, backward %.3g of max %.3g' % (N, e_f, e_s, e_b, np.abs(ref).max()))
    assert np.isfinite(got).all() and e_f <= 2e-6 and e_s <= 1e-6
    assert np.isfinite(_np(dl)).all() and e_b <= 1e-5 * np.abs(ref).max()
    assert torch.equal(ops.ani_blend_forward(_dt(bw, dev), torch.as_tensor(idx.astype(np.int32)).to(dev), _dt(logits, dev)), out)


# ------------------------------------------------------------------------------------------ 4. skinning
def skin_inputs(M):
    import aninerf_restatement as RS
    b = body(257)
    rng = np.random.default_rng(31 * M)
    idx = rng.integers(0, 257, M)
    posed = RS.to_pose(RS.t64(b['smpl_verts']), RS.t64(b['smpl_R']), RS.t64(b['smpl_T'].reshape(3))).numpy()
    pts = (posed[idx] + rng.normal(0, 0.03, (M, 3))).astype(np.float32)
    dirs = rng.normal(0, 1, (M, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)
    bw = RS.blend(RS.t64(b['smpl_bw']), idx, RS.t64(rng.normal(0, 1, (M, 24)))).numpy().astype(np.float32)
    return pts, dirs, bw, b['A'], b['big_A'], rng.normal(0, 1, (M, 3)).astype(np.float32), rng.normal(0, 1, (M, 3)).astype(np.float32)


def check_skin(dev, M):
    import aninerf_restatement as RS
    from xrnerf_amd import ops
    pts, dirs, bw, A, B, gp, gd = skin_inputs(M)
    worst = {}
    for what, a_from, a_to, with_dirs in (('A -> big_A', A, B, True), ('no dirs', A, B, False), ('big_A -> A', B, A, True)):
        d_in = _dt(dirs, dev) if with_dirs else None
        po, do = ops.ani_skin_forward(_dt(pts, dev), d_in, _dt(bw, dev), _dt(a_from, dev), _dt(a_to, dev))
        w64 = RS.t64(bw).requires_grad_(True)
        rp, rd = RS.skin(RS.t64(pts), RS.t64(dirs) if with_dirs else None, w64, RS.t64(a_from), RS.t64(a_to))
        loss = (rp * RS.t64(gp)).sum() + ((rd * RS.t64(gd)).sum() if with_dirs else 0.0)
        loss.backward()
        rp = rp.detach().numpy()
        e_p = (np.abs(_np(po) - rp) / np.maximum(1, np.abs(rp))).max()
        e_d = 0.0
        if with_dirs:
            rd = rd.detach().numpy()
            e_d = (np.abs(_np(do) - rd) / np.maximum(1, np.abs(rd))).max()
        else:
            assert do is None
        dbw = ops.ani_skin_backward(_dt(pts, dev), d_in, _dt(bw, dev), _dt(a_from, dev), _dt(a_to, dev), _dt(gp, dev),
                                    _dt(gd, dev) if with_dirs else None)
        ref = w64.grad.numpy()
        e_b = np.abs(_np(dbw) - ref).max() / np.abs(ref).max()
        print('skin M=%d %s: points %.3g dirs %.3g  dL/dbw %.3g of max|ref| (%.3g)' % (M, what, e_p, e_d, e_b, np.abs(ref).max()))
        assert e_p <= 1e-5 and e_d <= 1e-5 and np.isfinite(_np(dbw)).all() and e_b <= 1e-5, what
        worst[what] = (e_p, e_d, e_b)
        if with_dirs:
            # the direction gradient alone (grad_pts = NULL), and the same bits on a second launch
            w64.grad = None
            (RS.skin(RS.t64(pts), RS.t64(dirs), w64, RS.t64(a_from), RS.t64(a_to))[1] * RS.t64(gd)).sum().backward()
            only_d = ops.ani_skin_backward(_dt(pts, dev), d_in, _dt(bw, dev), _dt(a_from, dev), _dt(a_to, dev), None, _dt(gd, dev))
            assert np.abs(_np(only_d) - w64.grad.numpy()).max() <= 1e-5 * np.abs(w64.grad.numpy()).max()
            again = ops.ani_skin_forward(_dt(pts, dev), d_in, _dt(bw, dev), _dt(a_from, dev), _dt(a_to, dev))
            assert torch.equal(again[0], po) and torch.equal(again[1], do)
    return worst


def check_skin_one_hot(dev):
    """bw one-hot, a_from a pure rotation, a_to the identity: the rotation is inverted to 2e-6"""
    from xrnerf_amd import ops
    from xrnerf_amd.aninerf import _rot
    rng = np.random.default_rng(9)
    M = 65
    A = np.tile(np.eye(4), (24, 1, 1))
    for j in range(24):
        A[j, :3, :3] = _rot(rng.normal(0, 1, 3), rng.uniform(0, 3.0))
    I = np.tile(np.eye(4), (24, 1, 1))
    x = rng.uniform(-1, 1, (M, 3))
    j = rng.integers(0, 24, M)
    p = np.einsum('mij,mj->mi', A[j, :3, :3], x)
    bw = np.zeros((M, 24), np.float32)
    bw[np.arange(M), j] = 1
    po, do = ops.ani_skin_forward(_dt(p, dev), _dt(p, dev), _dt(bw, dev), _dt(A, dev), _dt(I, dev))
    err = max(np.abs(_np(po) - x).max(), np.abs(_np(do) - x).max())
    print('one-hot rotation inverted to %.3g' % err)
    assert err <= 2e-6


# ------------------------------------------------------------------------------------------ 5. encode backward
def check_encode_backward(dev, L, padded):
    import aninerf_restatement as RS
    from xrnerf_amd import ops
    N = 130
    rng = np.random.default_rng(17 * L + padded)
    p = rng.uniform(-1.5, 1.5, (N, 3)).astype(np.float32)
    cp = 3 + 6 * L
    ld = cp + 5 if padded else cp
    g = rng.normal(0, 1, (N, ld)).astype(np.float32)
    p64 = RS.t64(p).requires_grad_(True)
    (RS.embed(p64, L) * RS.t64(g[:, :cp])).sum().backward()
    ref = p64.grad.numpy()
    gt = _dt(g, dev)
    got = ops.ani_encode_backward(_dt(p, dev), gt[:, :cp] if padded else gt, L)
    err = np.abs(_np(got) - ref).max()
    print('encode backward L=%d padded=%d: %.3g of max %.3g' % (L, padded, err, np.abs(ref).max()))
    assert err <= 1e-5 * np.abs(ref).max()
    # a column range that starts inside a wider matrix
    if padded:
        wide = torch.cat([gt.new_zeros((N, 3)), gt], 1)
        assert torch.equal(ops.ani_encode_backward(_dt(p, dev), wide[:, 3:3 + cp], L), got)


@pytest.mark.parametrize('V', V_SHAPES)
@pytest.mark.parametrize('N', N_SHAPES)
def test_closest_vertex_matches_the_fp32_restatement_bit_for_bit(dev, N, V):
    check_closest(dev, N, V)


def test_closest_vertex_duplicate_and_on_vertex(dev):
    check_closest_edges(dev)


def test_selection_is_nonzero_of_the_restated_mask(dev):
    check_select(dev)


@pytest.mark.parametrize('N', [1, 63, 65, 130, 300])
def test_blend_head_forward_and_backward(dev, N):
    check_blend(dev, N)


@pytest.mark.parametrize('M', N_SHAPES)
def test_skinning_forward_and_backward_against_float64_autograd(dev, M):
    check_skin(dev, M)


def test_skinning_inverts_a_one_hot_rotation(dev):
    check_skin_one_hot(dev)


@pytest.mark.parametrize('padded', [0, 1])
@pytest.mark.parametrize('L', [0, 6, 10])
def test_encode_backward_against_float64_autograd(dev, L, padded):
    check_encode_backward(dev, L, padded)


# ------------------------------------------------------------------------------------------ the reference's steps
def model_cfg():
    return json.load(open(os.path.join(G, 'aninerf_model_cfg.json')))['model']


def network(dev, gold, phase):
    import aninerf_restatement as RS
    import xrnerf_amd
    cfg = copy.deepcopy(model_cfg())
    cfg['cfg']['phase'] = cfg['cfg']['deform_field']['phase'] = phase
    net = xrnerf_amd.build_network(cfg)
    sd = net.state_dict()
    net.load_state_dict(RS.formula_state_dict(list(sd.keys()), [tuple(v.shape) for v in sd.values()], int(gold['seed'])), strict=True)
    return net.to(dev)


def batch(dev, gold):
    """what the data loader hands train_step: the fixture's `datas` with a leading batch axis of 1"""
    out = {}
    for k in gold.files:
        if k.startswith('tp_in.'):
            v = gold[k]
            out[k[6:]] = (torch.as_tensor(v) if v.dtype.kind == 'i' else _dt(v, dev)).to(dev)[None]
    return out


def _grads_close(net, gold, prefix):
    import aninerf_restatement as RS
    from conftest import grad_close
    n = 0
    for k, p in net.named_parameters():
        if prefix + 'gnorm.' + k not in gold.files:
            assert p.grad is None or not p.requires_grad, k
            continue
        assert p.grad is not None, k
        g = _np(p.grad).reshape(-1)
        grad_close(g[RS.sample_positions(k, g.size)], gold[prefix + 'gsample.' + k], prefix + k, kinks=True)
        grad_close(np.array([np.linalg.norm(g.astype(np.float64))]), np.array([float(gold[prefix + 'gnorm.' + k])]), prefix + k + ' norm',
                   kinks=True)
        n += 1
    return n


def check_train_pose_step(dev, gold, repeat=False):
    import grad_bars
    net = network(dev, gold, 'train_pose')
    params = net.get_params()
    out = net.train_step(batch(dev, gold), None)
    out['loss'].backward()
    ret = out['ret']
    d = ret['deform']
    assert np.array_equal(_np(d['pind'][0]), gold['tp.pind'])
    assert np.array_equal(_np(ret['bw_mask']), gold['tp.chosen'])
    for k, got in (('tpose', d['tpose']), ('tpose_dirs', d['tpose_dirs']), ('pbw', d['pbw_rows']), ('tbw', d['tbw_rows'])):
        err = np.abs(_np(got) - gold['tp.' + k]).max()
        print('%s: %.3g' % (k, err))
        assert _np(got).shape == gold['tp.' + k].shape and err <= 1e-5, k
    assert tuple(d['pbw'].shape) == (1, 24, gold['tp.pbw'].shape[0])              # the reference's layout at the module boundary
    raw = _np(ret['raw'])
    print('raw: %.3g of max %.3g' % (np.abs(raw - gold['tp.raw']).max(), np.abs(gold['tp.raw']).max()))
    grad_bars.raw_close(raw, gold['tp.raw'], 'raw')
    assert np.abs(_np(ret['rgb']) - gold['tp.rgb']).max() <= 1e-5
    for k in ('img_loss', 'bw_loss'):
        got, ref = float(out[k].detach()), float(gold['tp.' + k])
        print('%s %.9g against %.9g: %.3g relative' % (k, got, ref, abs(got - ref) / abs(ref)))
        assert abs(got - ref) <= 1e-5 * abs(ref), k
    assert _grads_close(net, gold, 'tp.') == len(params)
    if repeat:
        first = [out['loss'].detach().clone()] + [p.grad.clone() for p in params]
        net.zero_grad()
        out = net.train_step(batch(dev, gold), None)
        out['loss'].backward()
        for a, b in zip(first, [out['loss'].detach()] + [p.grad for p in params]):
            assert torch.equal(a, b)


def check_novel_pose_step(dev, gold):
    net = network(dev, gold, 'novel_pose')
    params = net.get_params()
    assert sorted(k for k, p in net.named_parameters() if p.requires_grad) == sorted(gold['np.trainable'].tolist())
    draws = (_dt(gold['np.draws_world'], dev), _dt(gold['np.draws_canonical'], dev))
    out = net.train_step(batch(dev, gold), None, draws=draws)
    out['loss'].backward()
    for i, ((pbw, tbw), m) in enumerate(zip(out['bw_rows'], out['bw_masks'])):
        assert int(m.sum()) == gold['np.pbw%d' % i].shape[0], i                    # the same rows chosen
        for name, rows in (('pbw', pbw), ('tbw', tbw)):
            err = np.abs(_np(rows[m]) - gold['np.%s%d' % (name, i)]).max()
            print('novel %s%d: %.3g' % (name, i, err))
            assert err <= 1e-5
    got, ref = float(out['loss'].detach()), float(gold['np.loss0']) + float(gold['np.loss1'])
    print('novel loss %.9g against %.9g: %.3g relative' % (got, ref, abs(got - ref) / abs(ref)))
    assert abs(got - ref) <= 1e-5 * abs(ref)
    assert _grads_close(net, gold, 'np.') == len(params)


def check_path_taken(dev, gold):
    """a train_pose step issues the new entry points: two nearest-vertex queries, one selection, two blend heads, one skinning, and
    their backwards with the encodings' input gradients"""
    from xrnerf_amd import ops
    names = ('ani_closest', 'ani_select', 'ani_blend_forward', 'ani_blend_backward', 'ani_skin_forward', 'ani_skin_backward',
             'ani_encode_backward')
    saved = {n: getattr(ops, n) for n in names}
    calls = []

    def wrap(n):
        def f(*a, **k):
            calls.append(n)
            return saved[n](*a, **k)
        return f
    net = network(dev, gold, 'train_pose')
    net.get_params()
    try:
        for n in names:
            setattr(ops, n, wrap(n))
        out = net.train_step(batch(dev, gold), None)
        fwd = list(calls)
        out['loss'].backward()
    finally:
        for n in names:
            setattr(ops, n, saved[n])
    assert fwd == ['ani_closest', 'ani_select', 'ani_blend_forward', 'ani_skin_forward', 'ani_closest', 'ani_blend_forward'], fwd
    bwd = calls[len(fwd):]
    assert bwd.count('ani_skin_backward') == 1 and bwd.count('ani_blend_backward') == 2, bwd
    if ops.vanilla_kernels_available():
        # tpose feeds the blend-weight, density and colour MLPs; the skinned directions feed the colour MLP
        assert bwd.count('ani_encode_backward') == 3, bwd


def check_state_dict_and_registry(gold):
    import xrnerf_amd
    from xrnerf_amd import aninerf
    net = xrnerf_amd.build_network(copy.deepcopy(model_cfg()))
    assert isinstance(net, aninerf.AniNeRFNetwork) and isinstance(net.deform_field, aninerf.DeformField)
    assert isinstance(net.tpose_human, aninerf.TPoseHuman) and isinstance(net.tpose_human.density_network, aninerf.AN_DensityMLP)
    assert isinstance(net.tpose_human.color_network, aninerf.AN_ColorMLP) and isinstance(net.deform_field.bw_mlp, aninerf.AN_BlendWeightMLP)
    sd = net.state_dict()
    assert list(sd.keys()) == gold['sd_keys'].tolist()
    assert [list(v.shape) for v in sd.values()] == [json.loads(s) for s in gold['sd_shapes'].tolist()]
    assert tuple(sd['deform_field.bw_mlp.bw_linears.0.weight'].shape) == (256, 191, 1)
    assert 'tpose_human.density_network.lin0.weight_g' in sd and 'tpose_human.color_network.lin3.weight_v' in sd
    # get_params freezes what the reference freezes
    p = net.get_params()
    frozen = {k for k, v in net.named_parameters() if not v.requires_grad}
    assert frozen and all(k.startswith('deform_field.novel_pose_bw_mlp.') for k in frozen)
    assert len(p) == len(list(net.tpose_human.parameters())) + len(list(net.deform_field.bw_mlp.parameters()))
    cfg = copy.deepcopy(model_cfg())
    cfg['cfg']['phase'] = 'novel_pose'
    net = xrnerf_amd.build_network(cfg)
    p = net.get_params()
    live = {k for k, v in net.named_parameters() if v.requires_grad}
    assert live and all(k.startswith('deform_field.novel_pose_bw_mlp.') for k in live) and len(p) == len(live)


def check_val_step(dev, gold):
    """val_step through batchify_forward: the rays go through in `chunk`-sized pieces and come back as an image"""
    net = network(dev, gold, 'train_pose')
    net.chunk = 12
    b = batch(dev, gold)
    n = b['rays_o'].shape[1]
    H, W = 5, 8
    mask = torch.zeros(H * W, dtype=torch.bool, device=dev)
    mask[torch.arange(n, device=dev)] = True
    b['mask_at_box'] = mask[None]
    b['src_shape'] = torch.tensor([[H, W, 3]])
    out = net.val_step(b)
    assert out['rgb'].shape == (H, W, 3) and np.isfinite(out['rgb']).all() and out['gt_img'].shape == (H, W, 3)
    # one piece: the image holds forward()'s colours (smaller pieces each add their own nearest sample, as in the reference)
    net.chunk = n
    b = batch(dev, gold)
    b['mask_at_box'], b['src_shape'] = mask[None], torch.tensor([[H, W, 3]])
    one = net.val_step(b)
    with torch.no_grad():
        ret = net.forward({k: v[0] for k, v in batch(dev, gold).items()}, is_test=True)
    assert np.array_equal(one['rgb'].reshape(-1, 3)[:n], _np(ret['rgb'])) and one['idx'] == 1


def check_convergence(dev, steps=100):
    """100 Adam steps of train_pose on the synthetic body: the 20-step loss means fall"""
    import xrnerf_amd
    from xrnerf_amd.aninerf import synthetic_body
    torch.manual_seed(2)
    net = xrnerf_amd.build_network(copy.deepcopy(model_cfg())).to(dev)
    opt = torch.optim.Adam(net.get_params(), lr=5e-4)
    datas = synthetic_body(257, 5, 64, 16, device=dev)
    losses = []
    for _ in range(steps):
        out = net.train_step({k: v[None] for k, v in datas.items()}, opt)
        opt.zero_grad(set_to_none=True)
        out['loss'].backward()
        opt.step()
        losses.append(out['loss'].detach())
    means = torch.stack(losses).reshape(-1, 20).mean(1).cpu().numpy()
    print('20-step loss means:', ' '.join('%.4g' % v for v in means))
    assert np.isfinite(means).all() and (means[1:] < means[:-1]).all(), means


def test_train_pose_step_against_the_reference_fixture(dev, gold):
    check_train_pose_step(dev, gold)


def test_novel_pose_step_against_the_reference_fixture(dev, gold):
    check_novel_pose_step(dev, gold)


def test_two_identical_steps_give_the_same_bits(dev, gold):
    check_train_pose_step(dev, gold, repeat=True)


def test_training_step_issues_the_aninerf_kernels(dev, gold):
    check_path_taken(dev, gold)


def test_state_dict_registry_and_frozen_parameters(dev, gold):
    check_state_dict_and_registry(gold)


def test_val_step_renders_in_chunks(dev, gold):
    check_val_step(dev, gold)


def test_train_pose_converges_on_the_synthetic_body(dev):
    check_convergence(dev)
