"""TEST INFRASTRUCTURE ONLY (numpy): synthetic inputs of the compositor kernels, built directly (no marching) so that the paths marched
Lego rays never reach are reached: rays longer than 128 samples (k_composite_train_w's long chunks), 64-ray groups wider than
CT_CAP = 6144 rows (k_composite_train's direct path), lengths on both sides of every chunking threshold, empty rays at group starts.

Ray bases ascend as K1's prefix gives them (an empty ray has the base of the next one); only column 3 of `coords` (the warped dt)
matters.  Common to all cases: 30 % of the rays are clipped to half their samples (then no background term), 2 % of the rows are
opaque (raw_w = 12), warped dt = uniform(0, 1)^4, rgb raw ~ N(0, 1.5), density raw ~ N(2, 3) (|.| of it for the non-exponential
density activations).  Every case asserts from its own arrays that it still reaches what it is there for."""
import functools

import numpy as np

CT_CAP = 6144           # xr_raymarch.hip: rows a workgroup of k_composite_train stages through LDS
SEG = 1024              # XR_LIVE_SEG
EDGE_LENGTHS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 0, 0, 127, 128, 129, 255, 256, 257, 1, 0, 1023, 1024, 5, 0]
SEEDS = dict(A=101, B=102, C=103, D=104, E=100)     # (A, E: seeds at which no edge length is clipped in all three of its copies)


def group_spans(numsteps_c, group=64):
    """row span [min base, max base + n) of the rays WITH samples of every `group` consecutive rays (0: none has any)"""
    out = []
    for g0 in range(0, numsteps_c.shape[0], group):
        g = numsteps_c[g0:g0 + group]
        g = g[g[:, 0] > 0]
        out.append(int((g[:, 0] + g[:, 1]).max() - g[:, 1].min()) if len(g) else 0)
    return out


def wave_chunk_straddles(numsteps_c):
    """a ray of 961..1024 samples (16-row chunks per lane in the wave-per-ray kernel) with a chunk on both sides of a segment boundary"""
    for n, b in numsteps_c.tolist():
        if (n + 63) // 64 == 16:
            for l in range(64):
                k0, k1 = min(n, 16 * l), min(n, 16 * l + 16)
                if k1 > k0 and (b + k0) // SEG != (b + k1 - 1) // SEG:
                    return True
    return False


def _build(lengths, rng, extremes=False):
    lengths = np.asarray(lengths, np.int64)
    n_rays, S = len(lengths), int(lengths.sum())
    ns = np.zeros((n_rays, 2), np.int32)
    ns[:, 0] = lengths
    ns[:, 1] = np.cumsum(lengths) - lengths
    nsc = ns.copy()
    cut = rng.uniform(0, 1, n_rays) < 0.3
    nsc[cut, 0] //= 2
    raw = rng.normal(0, 1.5, (S, 4)).astype(np.float32)
    raw[:, 3] = rng.normal(2.0, 3.0, S)
    raw[rng.uniform(0, 1, S) < 0.02, 3] = 12.0
    coords = rng.uniform(0, 1, (S, 7)).astype(np.float32)
    coords[:, 3] = (rng.uniform(0, 1, S) ** 4).astype(np.float32)
    if extremes:
        k = np.nonzero(rng.uniform(0, 1, S) < 0.01)[0]
        raw[k, 3] = rng.choice(np.array([-200, -20, 20, 200], np.float32), k.size)
        k = np.nonzero(rng.uniform(0, 1, S) < 0.01)[0]
        raw[k, :3] = rng.choice(np.array([-20, 20], np.float32), (k.size, 3))
        k = np.nonzero(rng.uniform(0, 1, S) < 0.01)[0]
        coords[k, 3] = rng.choice(np.array([0, 1], np.float32), k.size)
    return dict(numsteps=ns, numsteps_c=nsc, raw=raw, coords=coords,
                bg=rng.uniform(0, 1, (n_rays, 3)).astype(np.float32), target=rng.uniform(0, 1, (n_rays, 3)).astype(np.float32),
                alpha=(rng.uniform(0, 1, (n_rays, 1)) > 0.3).astype(np.float32), grad=rng.normal(0, 1, (n_rays, 3)).astype(np.float32),
                n_rays=n_rays, S=S)


def _assert_edges(c):
    n = c['numsteps_c'][:, 0]
    assert c['n_rays'] == 81 and c['S'] == 10641
    assert n.max() > 128                                               # the long chunks of the wave-per-ray kernel
    assert set([128, 129, 255, 256, 257, 1023, 1024, 63, 64, 65]) <= set(n.tolist())    # every threshold survives the clipping
    assert any(n[i] == 0 for i in range(0, 81, 4)) and any(n[i] == 0 for i in range(0, 81, 64))   # empty rays that start a 4- / 64-ray group
    assert n[0] == 0 and (n[::4] == 0).sum() >= 2
    assert wave_chunk_straddles(c['numsteps_c'])
    assert (c['numsteps_c'][:, 0] < c['numsteps'][:, 0]).any()


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(SEEDS[name])
    if name in 'AE':
        c = _build(EDGE_LENGTHS * 3, rng, extremes=name == 'E')
        _assert_edges(c)
        if name == 'E':
            raw, dtw = c['raw'], c['coords'][:, 3]
            assert set(raw[:, 3].tolist()) >= {-200.0, -20.0, 20.0, 200.0} and (np.abs(raw[:, :3]) == 20).any()
            assert (dtw == 0).any() and (dtw == 1).any()
            import ref64_compositor as R          # (the constructor asserts that the float64 walk is finite on these)
            R.Walk(raw, c['coords'], c['numsteps'], 2, 3)
    elif name == 'B':
        c = _build(rng.integers(90, 200, 200), rng)
        spans = group_spans(c['numsteps_c'])
        # every COMPLETE 64-ray group is on the direct path of k_composite_train (200 rays: the 8 rays left over are staged).  The
        # counts before the clipping are all above 64 and mostly above 128; clipped to half, a ray of < 128 falls to <= 64, so on the
        # compacted counts the claim is: most above 64, many above 128
        assert len(spans) == 4 and all(s > CT_CAP for s in spans[:3])
        nf, n = c['numsteps'][:, 0], c['numsteps_c'][:, 0]
        assert nf.min() > 64 and (nf > 128).mean() > 0.5
        assert (n > 64).mean() > 0.5 and (n > 128).sum() >= 50
    elif name == 'C':
        c = _build(rng.integers(0, 40, 1001), rng)
        n = c['numsteps_c'][:, 0]
        assert c['n_rays'] % 64 and c['n_rays'] % 4 and (n == 0).sum() > 20 and max(group_spans(c['numsteps_c'])) <= CT_CAP
    elif name == 'D':
        c = _build(np.concatenate([rng.integers(0, 40, 64), rng.integers(90, 200, 64), rng.integers(0, 40, 64)]), rng)
        spans = group_spans(c['numsteps_c'])
        assert 0 < spans[0] <= CT_CAP < spans[1] and 0 < spans[2] <= CT_CAP    # staged, direct, staged workgroups in one launch
    else:
        raise KeyError(name)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def raw_for(c, density_act):
    raw = c['raw'].copy()
    if density_act != 3:
        raw[:, 3] = np.abs(raw[:, 3])
    return raw
