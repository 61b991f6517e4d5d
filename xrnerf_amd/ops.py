"""Tensor-level front-end of the C-ABI: torch is used only for device memory and streams.

Every function takes contiguous CUDA(ROCm) tensors, enqueues on torch's current stream and does
NOT synchronise.  There is no CPU path: a non-CUDA tensor is an error.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

G3 = 128 ** 3
N_GRID = 8 * G3

_workspaces = {}


class KernelTimer:
    """Optional per-entry-point device timing with events recorded on the launch stream (torch's
    current stream IS the stream every kernel of this library is enqueued on).  bench.py uses it to
    get the dominant kernel's average duration live inside the timed region."""

    def __init__(self, only=None, train_only=False):
        self.events = {}
        self.only = only            # record only these entry points (None = all)
        self.train_only = train_only   # record only the training step's launches (row count on the device), not the
                                       # occupancy-grid density queries / render launches of the same entry points

    def span(self, name, units=0, train=True):
        if self.only is not None and name not in self.only:
            return _NOSPAN
        if self.train_only and not train:
            return _NOSPAN
        return _Span(self, name, units)

    # the entry points xr_ngp_train_step runs (it can bracket ONE of them with a pair of events): a timer that asks for
    # nothing else inside the step leaves the native path usable
    STEP_STAGES = ('xr_hashgrid_fwd', 'xr_nerf_mlp_fwd', 'xr_composite_train', 'xr_live_rows', 'xr_nerf_mlp_bwd', 'xr_hashgrid_bwd')

    def native_stage(self):
        """-> (ok, stage): ok if the native step can serve this timer; stage = the one step stage to bracket (or None)"""
        if self.only is None:
            return False, None
        inside = [k for k in self.only if k in self.STEP_STAGES]
        return len(inside) <= 1, (inside[0] if inside else None)

    def summary(self):
        """name -> (launches, total_ms, total_units); call after torch.cuda.synchronize()"""
        return {k: (len(v), sum(a.elapsed_time(b) for a, b, _ in v), sum(u for _, _, u in v))
                for k, v in self.events.items()}


class _Span:
    def __init__(self, timer, name, units):
        self.timer, self.name, self.units = timer, name, units

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.b = torch.cuda.Event(enable_timing=True)
        self.a.record()

    def __exit__(self, *exc):
        self.b.record()
        self.timer.events.setdefault(self.name, []).append((self.a, self.b, self.units))


class _CEvent:
    """a timing event of the library (xr_timing_event_*): what xr_ngp_train_step / xr_ngp_loop_run record around a stage or in front of an
    iteration"""

    def __init__(self):
        self.h = _lib.load().xr_timing_event_create()
        if not self.h:
            raise _lib.XrError('cannot create a timing event')

    def elapsed_time(self, other):
        ms = C.c_float()
        _lib.check(_lib.load().xr_timing_event_elapsed_ms(self.h, other.h, C.byref(ms)), 'xr_timing_event_elapsed_ms')
        return float(ms.value)

    def __del__(self):
        try:
            _lib.load().xr_timing_event_destroy(self.h)
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class _NoSpan:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


TIMER = None
_NOSPAN = _NoSpan()


def _span(name, units=0, train=True):
    return TIMER.span(name, units, train) if TIMER is not None else _NOSPAN


_PRECISION = os.environ.get('XRNERF_MLP_PRECISION', 'f32')
if _PRECISION not in ('f32', 'f16'):
    raise ValueError("XRNERF_MLP_PRECISION must be 'f32' or 'f16' (got %r)" % _PRECISION)


# forward of the 'f32' mode (the `arithmetic` argument of xr_nerf_mlp_fwd): 'f16x2' = XR_MLP_F16X2 (the default: fp32 operands as two fp16 parts, three fp16 MFMAs per product
# block, fp32 accumulate: within a few ulps of fp32 at half the matrix instructions of the 3-way split), 'bf16x3' =
# XR_MLP_BF16X3 (three bf16 parts, six MFMAs: fp32-rounding accuracy), 'mfma' = XR_MLP_F32 (v_mfma_f32_32x32x2_f32).
# Depths other than (1, 2) run the streamed kernel (f16x2 arithmetic) whatever this says, except (1,1), (2,2), (2,3) under 'mfma'.
_F32_FORWARD = os.environ.get('XRNERF_F32_FORWARD', 'f16x2')          # (set_f32_forward; switches.py)
if _F32_FORWARD not in ('f16x2', 'bf16x3', 'mfma'):
    raise ValueError("XRNERF_F32_FORWARD must be 'f16x2', 'bf16x3' or 'mfma' (got %r)" % _F32_FORWARD)


def f32_forward():
    return _F32_FORWARD


def set_f32_forward(kind):
    global _F32_FORWARD
    if kind not in ('f16x2', 'bf16x3', 'mfma'):
        raise ValueError("the fp32 forward is 'f16x2', 'bf16x3' or 'mfma'")
    _F32_FORWARD = kind


def _mlp_mode(nhd=1, nhc=2):
    """xr_ngp_train_step's mlp_mode for the current settings"""
    if nhd == 1 and nhc == 2:
        if _PRECISION == 'f16':
            return 1
        if _F32_FORWARD == 'bf16x3':
            return 2
    return 3 if _F32_FORWARD == 'f16x2' else 0


def precision():
    """arithmetic mode of the fused MLP: 'f32' (parity mode, default: v_mfma_f32_32x32x2_f32, exact fp32) or 'f16'
    (the reference's own precision -- tiny-cuda-nn computes FullyFusedMLP in fp16 with fp32 accumulation:
    v_mfma_f32_32x32x16_f16, fp32 parameters / gradients in memory, fp32 outputs)"""
    return _PRECISION


def set_precision(p):
    global _PRECISION
    if p not in ('f32', 'f16'):
        raise ValueError("precision must be 'f32' or 'f16'")
    _PRECISION = p


def _stream():
    # raw hipStream_t of torch's current stream; torch.cuda.current_stream() costs ~7 us of Python per call and
    # a training step makes ~20 of them
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def _on_device(t):
    """the one place that decides whether a tensor may be handed to the library (tests/hip_emu swaps it to run the
    kernels' host build on CPU tensors)"""
    return t.is_cuda


def _ptr(t):
    if t is None:
        return None
    if not _on_device(t):
        raise _lib.XrError('xrnerf_amd ops need ROCm device tensors (got a %s tensor): there is no CPU fallback' % t.device)
    if not t.is_contiguous():
        raise _lib.XrError('tensor must be contiguous')
    return C.c_void_p(t.data_ptr())


def _ws(device, nbytes, tag):
    key = (str(device), tag)
    w = _workspaces.get(key)
    if w is None or w.numel() < nbytes:
        w = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        if tag == 'mlpbwd':
            # holds the live-row count block, whose words 1-2 are RUNNING totals (k_live_fill adds to them): they start at zero.
            # (uint32: a reader -- bench.py prices the backward kernels from them -- clears them per measurement window)
            w.zero_()
        _workspaces[key] = w
    return w


def _buf(device, shape, tag):
    """grow-only fp32 scratch of the given shape (a view of a persistent buffer per tag): frame-sized intermediates whose size
    changes from frame to frame (13-15 M samples: 1.7 GB of encoded features) would otherwise send the caching allocator to
    hipMalloc / hipFree -- device-synchronising calls of ~10 ms -- on most frames"""
    n = 1
    for v in shape:
        n *= int(v)
    key = (str(device), tag)
    have = _workspaces.get(key)
    need = 4 * max(n, 1) + 256
    # grow with 25 % headroom: frames of one sequence differ by a few per cent in their sample counts
    w = _ws(device, need if (have is not None and have.numel() >= need) else need + need // 4, tag)
    off = (-w.data_ptr()) % 16
    return w[off:off + 4 * n].view(torch.float32).view(*shape)


_helpers = {}
_helper_current = {}            # host thread -> the device whose helper the library's (per-thread) slot holds right now


def _ensure_helper(device):
    """hand the library this thread's helper stream (xr_set_helper_stream): one stream + fork / join events per device and host thread,
    created HERE -- the library itself creates nothing.  Without it the scatter's side work runs in order on the compute stream.
    The library's slot is one per host thread: a thread that moves to another device hands over that device's stream again."""
    import threading
    if device.type != 'cuda':
        return
    tid = threading.get_ident()
    key = (str(device), tid)
    if _helper_current.get(tid) == key:
        return
    h = _helpers.get(key)
    if h is None:
        with torch.cuda.device(device):
            st = torch.cuda.Stream(device=device)
            evs = (torch.cuda.Event(), torch.cuda.Event())
            for e in evs:
                e.record(st)                           # (torch creates the underlying event at its first record, on the current device)
        h = _helpers[key] = (st, evs)
    st, evs = h
    _lib.check(_lib.load().xr_set_helper_stream(C.c_void_p(st.cuda_stream), C.c_void_p(evs[0].cuda_event), C.c_void_p(evs[1].cuda_event)),
               'xr_set_helper_stream')
    _helper_current[tid] = key


# ---- range of the default MLP arithmetic (XR_MLP_F16X2 saturates its operands at +-65504 and counts the waves that saw one out of
# range in the caller's word: include/xrnerf_mi355.h).  One uint32 word per device; the library's slot is per host thread.
_range_words = {}
_range_current = {}
_range_off = set()              # host threads whose launches run untracked right now (mlp_range_tracking)


def mlp_range_word(device):
    """this device's range word (a [1] int32 tensor, allocated once), handed to the library for the calling thread -- unless the thread
    has tracking switched off (mlp_range_tracking), in which case the library is told `none`: the forwards then run without the max
    chain behind the count (4 us of a 32-us launch), the saturation itself stays"""
    import threading
    if device.type != 'cuda':
        return None
    w = _range_words.get(str(device))
    if w is None:
        w = _range_words[str(device)] = torch.zeros((1,), dtype=torch.int32, device=device)
    tid = threading.get_ident()
    want = None if tid in _range_off else str(device)
    if _range_current.get(tid, 0) != want:
        _lib.check(_lib.load().xr_set_mlp_range_word(C.c_void_p(w.data_ptr()) if want is not None else None), 'xr_set_mlp_range_word')
        _range_current[tid] = want
    return w


def mlp_range_tracking(device, on):
    """Switch the range count of the calling thread's XR_MLP_F16X2 forwards on (default) or off.  The trainer runs the iterations
    between two grid refreshes untracked (train._NativeLoop) and everything else -- the refresh iterations with their 2^20-point
    density queries, frames, direct calls -- tracked: one iteration in 16 looks, which is where growing weights or features show up"""
    import threading
    tid = threading.get_ident()
    if on:
        _range_off.discard(tid)
    else:
        _range_off.add(tid)
    mlp_range_word(device)


def mlp_range_events(device, reset=False):
    """waves of the default forward that met an operand above fp16's range since the last reset (a host read-back: synchronises)"""
    w = mlp_range_word(device)
    if w is None:
        return 0
    v = int(w.item())
    if reset and v:
        w.zero_()
    return v


def pcg32_host_state(ncalls, seed=9121):
    s, i = C.c_uint64(), C.c_uint64()
    _lib.load().xr_pcg32_host_state(seed, ncalls, C.byref(s), C.byref(i))
    return s.value, i.value


# ---------------------------------------------------------------- K1 / K2
def rays_sampler(rays_o, rays_d, bitfield, aabb, near_distance, cone_angle, max_samples, rng_calls,
                 coords_out=None, ws_tag='k1', small_out=None, xyz_out=None, rng_chunk=0, rng_ray0=0, wide=False):
    """returns coords_out [max_samples,7], rays_index [n,1], rays_numsteps [n,2], counter [2] (device).
    `small_out` = (rays_index, numsteps, counter) caller-owned buffers (persistent double buffers of the trainer).
    `xyz_out` = [3, >= max_samples] float32: the sample positions once more as three planes (hashgrid_fwd's fast input).
    `rng_chunk` > 0: the jitter of ceil(n / rng_chunk) consecutive launches over rng_chunk rays each (call indices rng_calls,
    rng_calls + 1, ...) in this one launch; `rng_ray0`: the launch's rays are rays rng_ray0.. of that series' frame.
    `wide`: nothing else runs on the device (XR_K1_WIDE): up to 32 768 rays march with 8 lanes per ray, same samples."""
    L = _lib.load()
    n = rays_o.shape[0]
    dev = rays_o.device
    if coords_out is None:
        coords_out = torch.empty((max_samples, 7), dtype=torch.float32, device=dev)
    if small_out is not None:
        rays_index, numsteps, counter = small_out
    else:
        rays_index = torch.empty((n, 1), dtype=torch.int32, device=dev)
        numsteps = torch.empty((n, 2), dtype=torch.int32, device=dev)
        counter = torch.empty((2,), dtype=torch.int32, device=dev)
    nb = L.xr_rays_sampler_workspace_bytes(n, 1)
    ws = _ws(dev, nb, ws_tag)
    st, inc = pcg32_host_state(rng_calls)
    with _span('xr_rays_sampler', n):
        _lib.check(L.xr_rays_sampler(_ptr(rays_o), _ptr(rays_d), _ptr(bitfield), n, aabb[0], aabb[1], near_distance,
                                      cone_angle, max_samples, st, inc, _ptr(coords_out), _ptr(rays_index),
                                      _ptr(numsteps), _ptr(counter), _ptr(xyz_out), xyz_out.shape[1] if xyz_out is not None else 0,
                                      int(rng_chunk), int(rng_ray0), 1 if wide else 0, _ptr(ws), ws.numel(), _stream()), 'xr_rays_sampler')
    return coords_out, rays_index, numsteps, counter


def compacted_coord(coords_in, numsteps, max_compacted, coords_out=None):
    L = _lib.load()
    n = numsteps.shape[0]
    dev = coords_in.device
    if coords_out is None:
        coords_out = torch.zeros((max_compacted, 7), dtype=torch.float32, device=dev)
    nc = torch.empty((n, 2), dtype=torch.int32, device=dev)
    rc = torch.empty((1,), dtype=torch.int32, device=dev)
    sc = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = _ws(dev, L.xr_rays_sampler_workspace_bytes(n, 1), 'k1')
    _lib.check(L.xr_compacted_coord(_ptr(coords_in), _ptr(numsteps), n, max_compacted, _ptr(coords_out), _ptr(nc),
                                    _ptr(rc), _ptr(sc), _ptr(ws), ws.numel(), _stream()), 'xr_compacted_coord')
    return coords_out, nc, rc, sc


# ---------------------------------------------------------------- K3 / K4 / K5
def calc_rgb_forward(raw, coords, numsteps, numsteps_c, bg, rgb_act, density_act, out=None):
    L = _lib.load()
    n = numsteps.shape[0]
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=raw.device)
    with _span('xr_calc_rgb_forward', 0):
        _lib.check(L.xr_calc_rgb_forward(_ptr(raw), _ptr(coords), _ptr(numsteps), _ptr(numsteps_c), _ptr(bg), n,
                                         int(rgb_act), int(density_act), _ptr(out), _stream()), 'xr_calc_rgb_forward')
    return out


def calc_rgb_backward(raw, numsteps_c, coords, grad_rgb, rgb_out, density_grid_mean, rgb_act, density_act, out=None):
    L = _lib.load()
    n = numsteps_c.shape[0]
    if out is None:
        out = torch.zeros_like(raw)
    with _span('xr_calc_rgb_backward', 0):
        _lib.check(L.xr_calc_rgb_backward(_ptr(raw), _ptr(numsteps_c), _ptr(coords), _ptr(grad_rgb), _ptr(rgb_out),
                                          _ptr(density_grid_mean), n, int(rgb_act), int(density_act), _ptr(out),
                                          _stream()), 'xr_calc_rgb_backward')
    return out


def composite_train(raw, coords, numsteps, numsteps_c, bg, target, alpha, density_grid_mean, rgb_act, density_act, loss_mse, draw,
                    delta=0.1, scale=5.0, rgb=None, live_seg=None):
    """K3 + scale * Huber (+ masked MSE) + K4 in one launch -> rgb [n,3]; `loss_mse` [2] and `draw` [S,4] must be zero-filled
    (loss terms are added, rows behind the last sample are not written).
    live_seg (int32 [live_segments(S)], zero-filled by the caller): the launch also counts the non-zero rows of `draw` per
    1024-row segment into it; follow with live_rows(..., seg_counts=live_seg).
    loss_mse=None: the wave-per-ray kernel (rgb / draw differ from the 16-lane kernels' like two fp32 summation orders); the loss
    scalars then come from train_loss_scalars(rgb, ...)."""
    n = numsteps.shape[0]
    if rgb is None:
        rgb = torch.empty((n, 3), dtype=torch.float32, device=raw.device)
    p_seg = _ptr(live_seg)
    with _span('xr_composite_train', 0):
        _lib.check(_lib.load().xr_composite_train(_ptr(raw), _ptr(coords), _ptr(numsteps), _ptr(numsteps_c), _ptr(bg), _ptr(target),
                                                   _ptr(alpha), _ptr(density_grid_mean), n, int(rgb_act), int(density_act),
                                                   float(delta), float(scale), _ptr(rgb), _ptr(loss_mse), _ptr(draw), p_seg, _stream()),
                   'xr_composite_train')
    return rgb


class MarchWindow:
    """Caller-owned buffers of a marched refresh window (xr_ngp_window, include/xrnerf_mi355.h): XR_NGP_WINDOW chunks at fixed strides.
    Iteration `it` lives in chunk it % WINDOW.  One allocation per array; `chunk(c)` hands out the views a single march / step takes."""

    N = _lib.WINDOW

    def __init__(self, device, ray_stride, coords_stride, planes=True):
        W = self.N
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        i = lambda *shape: torch.empty(shape, dtype=torch.int32, device=device)
        self.device, self.ray_stride, self.coords_stride = device, int(ray_stride), int(coords_stride)
        self.rays_o, self.rays_d, self.target, self.bg = f(W, ray_stride, 3), f(W, ray_stride, 3), f(W, ray_stride, 3), f(W, ray_stride, 3)
        self.alpha, self.img_ids = f(W, ray_stride, 1), i(W, ray_stride, 1)
        self.rays_index, self.numsteps, self.clipped = i(W, ray_stride, 1), i(W, ray_stride, 2), i(W, ray_stride, 2)
        self.coords = f(W, coords_stride, 7)
        self.xyz = f(W, 3, coords_stride) if planes else None
        self.counter2, self.n_valid = i(W, 2), i(W, 2)
        self.pinned = torch.zeros((W, 2), dtype=torch.int32).pin_memory() if device.type == 'cuda' else None
        c = _lib.Window()
        vp = lambda t: t.data_ptr() if t is not None else None
        c.rays_o, c.rays_d, c.target, c.alpha, c.bg, c.img_ids = vp(self.rays_o), vp(self.rays_d), vp(self.target), vp(self.alpha), vp(self.bg), vp(self.img_ids)
        c.rays_index, c.rays_numsteps, c.numsteps_clipped = vp(self.rays_index), vp(self.numsteps), vp(self.clipped)
        c.ray_stride, c.coords, c.coords_stride = self.ray_stride, vp(self.coords), self.coords_stride
        c.xyz_planes, c.plane_stride = vp(self.xyz), (self.coords_stride if planes else 0)
        c.counter2, c.n_valid = vp(self.counter2), vp(self.n_valid)
        self.c = c

    def batch(self, c, n):
        """the batch dict of chunk c (views; what HashBatchSample + RandomBGColor hand to train_step)"""
        return {'rays_o': self.rays_o[c, :n], 'rays_d': self.rays_d[c, :n], 'target_s': self.target[c, :n], 'alpha': self.alpha[c, :n],
                'img_ids': self.img_ids[c, :n], 'bg_color': self.bg[c, :n]}

    def batch_out(self, c):
        """chunk c's buffers in the form make_batch(out=...) takes"""
        return {'rays_o': self.rays_o[c], 'rays_d': self.rays_d[c], 'target_s': self.target[c], 'alpha': self.alpha[c],
                'img_ids': self.img_ids[c], 'bg_color': self.bg[c]}


def ngp_window_march(win, first_chunk, n_chunks, batches_ready, n, rows_table, cur_ray, batch_call_index, bitfield, aabb, near_distance,
                     cone_angle, max_samples, k1_call_index, max_compacted, batch_seed=20220901, ws_tag='k1_window'):
    """the batches and marches of window chunks [first_chunk, first_chunk + n_chunks) as one series of launches on the current stream
    (xr_ngp_window_march): batch assembly for all but the first `batches_ready` chunks, K1, K2's clip, counters to win.pinned.
    -> the table cursor behind the last batch drawn"""
    L = _lib.load()
    ws = _ws(win.device, L.xr_rays_sampler_workspace_bytes(n, n_chunks), ws_tag)
    try:
        native = L.xr_ngp_window_march
    except AttributeError:
        native = None            # the kernels' host build (tests/hip_emu) has no native executors: the same series calls from here
    if native is not None:
        cur = C.c_uint64(int(cur_ray))
        with _span('xr_rays_sampler', n * n_chunks):
            _lib.check(native(C.byref(win.c), first_chunk, n_chunks, batches_ready, n, _ptr(rows_table),
                              rows_table.shape[0] if rows_table is not None else 0, C.byref(cur), batch_seed, batch_call_index,
                              _ptr(bitfield), aabb[0], aabb[1], near_distance, cone_angle, max_samples, k1_call_index, max_compacted,
                              _ptr(ws), ws.numel(), C.c_void_p(win.pinned.data_ptr()) if win.pinned is not None else None, _stream()),
                       'xr_ngp_window_march')
        return int(cur.value)
    c0, c1, cur = first_chunk, first_chunk + n_chunks, int(cur_ray)
    if batches_ready < n_chunks:
        row0 = []
        for _ in range(batches_ready, n_chunks):
            if cur + n > rows_table.shape[0]:
                cur = 0
            row0.append(cur)
            cur += n
        b0 = c0 + batches_ready
        st, inc = pcg32_host_state(batch_call_index, batch_seed)
        _lib.check(L.xr_make_batch_series(_ptr(rows_table), (C.c_uint64 * len(row0))(*row0), n, len(row0), win.ray_stride, st, inc, _ptr(win.rays_o[b0:c1]),
                                          _ptr(win.rays_d[b0:c1]), _ptr(win.target[b0:c1]), _ptr(win.alpha[b0:c1]), _ptr(win.bg[b0:c1]),
                                          _ptr(win.img_ids[b0:c1]), _stream()), 'xr_make_batch_series')
    st, inc = pcg32_host_state(k1_call_index)
    _lib.check(L.xr_rays_sampler_series(_ptr(win.rays_o[c0:c1]), _ptr(win.rays_d[c0:c1]), win.ray_stride, _ptr(bitfield), n, n_chunks, aabb[0], aabb[1],
                                        near_distance, cone_angle, max_samples, st, inc, _ptr(win.coords[c0:c1]), win.coords_stride,
                                        _ptr(win.rays_index[c0:c1]), _ptr(win.numsteps[c0:c1]), _ptr(win.counter2[c0:c1]),
                                        _ptr(win.xyz[c0:c1]) if win.xyz is not None else None, win.coords_stride if win.xyz is not None else 0,
                                        _ptr(ws), ws.numel(), _stream()), 'xr_rays_sampler_series')
    _lib.check(L.xr_clip_numsteps(_ptr(win.numsteps[c0:c1]), _ptr(win.counter2[c0:c1]), n, n_chunks, win.ray_stride, max_compacted,
                                         _ptr(win.clipped[c0:c1]), _ptr(win.n_valid[c0:c1]), _stream()), 'xr_clip_numsteps')
    return cur


class TrainStepBuffers:
    """caller-owned buffers of xr_ngp_train_step for `n_rows` sample rows and up to `ray_cap` rays"""

    def __init__(self, device, n_rows, ray_cap, table_floats, wd_floats, wc_floats, meta, table_grad_storage=None):
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        self.n_rows, self.ray_cap, self.ld = n_rows, ray_cap, (n_rows + 63) // 64 * 64
        self.enc_t, self.denc_t = f(meta.n_output_dims, self.ld), f(meta.n_output_dims, self.ld)
        self.raw, self.draw, self.rgb = f(n_rows, 4), f(n_rows, 4), f(ray_cap, 3)
        # MLP gradients, the (loss, mse) scalars and the compositor's live-row counts in one block; the step writes the first two and
        # hands the counts back zeroed (no fill on the step's stream)
        n_seg = live_segments(n_rows)
        self.zero_block = torch.zeros((wd_floats + wc_floats + 4 + n_seg,), dtype=torch.float32, device=device)     # (the counts start at zero)
        self.live_seg = self.zero_block[wd_floats + wc_floats + 4:]
        self.g_wd, self.g_wc = self.zero_block[:wd_floats], self.zero_block[wd_floats:wd_floats + wc_floats]
        self.g_mlp = self.zero_block[:wd_floats + wc_floats]
        self.loss_mse = self.zero_block[wd_floats + wc_floats:wd_floats + wc_floats + 2]
        # `table_grad_storage`: -> (padded buffer, leading [table_floats] view) when the gradient collective wants padded storage
        # (dist.Zero1GradSync.pad_grad); the step writes the view
        self.g_table = table_grad_storage(device)[1] if table_grad_storage is not None else f(table_floats)


def ngp_train_step(table, wd, wc, nhd, nhc, pad_value, meta, coords, n_dev, numsteps, numsteps_c, bg, target, alpha,
                   density_grid_mean, rgb_act, density_act, bufs, huber_delta=0.1, loss_scale=5.0, scatter_level0=0, xyz=None,
                   adam=None, mlp_adam=None):
    """the device work of one HashNerfNetwork training step as one native call (xr_ngp_train_step): encode -> MLP -> K3 +
    Huber + K4 -> MLP backward -> table scatter into `bufs` (TrainStepBuffers).  Returns rgb [n_rays,3] (a view of bufs.rgb).
    scatter_level0 > 0 (data parallel): only hash levels [scatter_level0, n_levels) are scattered; the caller finishes with
    hashgrid_bwd(..., live=bufs.live, levels=(0, scatter_level0)) after handing the finer slice to its collective.
    adam (ops.adam_fuse of the table, single GPU): the scatter applies the optimiser's update to the table itself; bufs.g_table
    is not written.  mlp_adam = (adam_fuse of wd, adam_fuse of wc): their update runs behind the reduction of their gradients.

    The ~45 pointer / size arguments are validated and converted once per set of buffers (keyed by the data pointers of the
    tensors that alternate between iterations): at 0.45 ms per iteration the interpreter time of this call -- 30 pointer checks,
    four workspace queries -- was what the GPU waited for (tools/hosttime2.py)."""
    global LIVE_STATS
    L = _lib.load()
    n_rays = numsteps.shape[0]
    mode = _mlp_mode(nhd, nhc)
    mlp_range_word(coords.device)
    key = (table.data_ptr(), wd.data_ptr(), wc.data_ptr(), coords.data_ptr(), coords.shape[0], n_dev.data_ptr() if n_dev is not None else 0,
           numsteps.data_ptr(), numsteps_c.data_ptr(), bg.data_ptr(), target.data_ptr(), alpha.data_ptr(), density_grid_mean.data_ptr(),
           xyz.data_ptr() if xyz is not None else 0, xyz.shape[1] if xyz is not None else 0, nhd, nhc, pad_value, mode, id(meta),
           int(rgb_act), int(density_act), huber_delta, loss_scale, int(scatter_level0))
    cache = bufs.__dict__.setdefault('_step_args', {})
    ent = cache.get(key)
    if ent is None:
        n_rows = bufs.n_rows
        if coords.shape[0] < n_rows or coords.shape[1] != 7 or not coords.is_contiguous():
            raise _lib.XrError('coords must be contiguous [>= n_rows, 7] rows')
        s, r, o = meta._args()
        _ensure_helper(coords.device)
        _ws(coords.device, L.xr_nerf_mlp_bwd_workspace_bytes(n_rows, nhd, nhc), 'mlpbwd')
        ws_sc = _ws(coords.device, L.xr_hashgrid_bwd_workspace_bytes(n_rows, meta.n_levels, r, o), 'hgb')
        # the backward's (count, running live total, running valid total) block sits in the MLP workspace on this path
        ws_mlp, live_list, _, live_stats = _list_slots(coords.device, n_rows, nhd, nhc)
        live = (live_list, live_stats) if os.environ.get('XR_MLP_LIVE') != '0' else None     # (the native step reads the same switch)
        head = (_ptr(table), _ptr(wd), _ptr(wc), nhd, nhc, pad_value, mode, meta.n_levels, s, r, o,
                _ptr(coords), n_rows, _ptr(n_dev), _ptr(numsteps), _ptr(numsteps_c))
        mid = (_ptr(bg), _ptr(target), _ptr(alpha),
               _ptr(density_grid_mean), int(rgb_act), int(density_act), float(huber_delta), float(loss_scale),
               _ptr(bufs.enc_t), bufs.ld, _ptr(bufs.raw), _ptr(bufs.draw), _ptr(bufs.denc_t), _ptr(bufs.rgb),
               _ptr(bufs.zero_block), bufs.zero_block.numel(), _ptr(bufs.g_wd), _ptr(bufs.g_wc), _ptr(bufs.loss_mse), _ptr(bufs.live_seg),
               _ptr(bufs.g_table), bufs.g_table.numel(), 0 if n_dev is not None else 1,
               _ptr(ws_mlp), ws_mlp.numel(), _ptr(ws_sc), ws_sc.numel(), int(scatter_level0),
               _ptr(xyz), xyz.shape[1] if xyz is not None else 0)
        if len(cache) > 16:
            cache.clear()
        ent = cache[key] = (head, mid, live, live_stats, (ws_mlp, ws_sc, meta, table, wd, wc))     # (keeps what the pointers name alive)
    head, mid, live, LIVE_STATS = ent[0], ent[1], ent[2], ent[3]
    bufs.live = live
    stage, ev = None, (None, None)
    if TIMER is not None:
        ok, stage = TIMER.native_stage()
        if not ok:
            raise _lib.XrError('this KernelTimer needs the per-entry-point launch sequence (XRNERF_STEP=py)')
        if stage is not None:
            ev = (_CEvent(), _CEvent())
            TIMER.events.setdefault(stage, []).append((ev[0], ev[1], 0))
    rc = L.xr_ngp_train_step(*head, n_rays, *mid, C.byref(adam) if adam is not None else None,
                             C.byref(mlp_adam[0]) if mlp_adam else None, C.byref(mlp_adam[1]) if mlp_adam else None,
                             stage.encode() if stage else None, ev[0].h if stage else None, ev[1].h if stage else None, _stream())
    if rc != 0:
        _lib.check(rc, 'xr_ngp_train_step')
    return bufs.rgb[:n_rays]


def record_event(cevent):
    """record a timing event (_CEvent) on the current stream"""
    _lib.check(_lib.load().xr_event_record(cevent.h, _stream()), 'xr_event_record')


def calc_rgb_inference(raw, coords, numsteps, bg3, rgb_act, density_act):
    L = _lib.load()
    n = numsteps.shape[0]
    rgb = torch.empty((n, 3), dtype=torch.float32, device=raw.device)
    alpha = torch.empty((n, 1), dtype=torch.float32, device=raw.device)
    if raw.shape[0] == 0 or coords.shape[0] == 0:
        # a chunk of rays that all miss the occupied cells (the sky rows of a frame marched in chunk = 4096 pieces): every
        # per-ray count is 0 and nothing is read, but the entry point wants non-null buffers
        raw = torch.zeros((1, 4), dtype=torch.float32, device=numsteps.device)
        coords = torch.zeros((1, 7), dtype=torch.float32, device=numsteps.device)
    _lib.check(L.xr_calc_rgb_inference(_ptr(raw), _ptr(coords), _ptr(numsteps), float(bg3[0]), float(bg3[1]),
                                       float(bg3[2]), n, int(rgb_act), int(density_act), _ptr(rgb), _ptr(alpha),
                                       _stream()), 'xr_calc_rgb_inference')
    return rgb, alpha


def render_slice_select(numsteps, T, s0, s1, eps, rows, ray_off, count):
    _lib.check(_lib.load().xr_render_slice_select(_ptr(numsteps), _ptr(T), numsteps.shape[0], s0, s1, eps, _ptr(rows),
                                                  _ptr(ray_off), _ptr(count), _stream()), 'xr_render_slice_select')


def render_slice_composite(raw_s, coords, numsteps, ray_off, s0, s1, rgb_act, density_act, T, rgb_acc):
    _lib.check(_lib.load().xr_render_slice_composite(_ptr(raw_s), _ptr(coords), _ptr(numsteps), _ptr(ray_off),
                                                     numsteps.shape[0], s0, s1, int(rgb_act), int(density_act), _ptr(T),
                                                     _ptr(rgb_acc), _stream()), 'xr_render_slice_composite')


# ---------------------------------------------------------------- K6 .. K11
def generate_grid_samples(grid, ema_step, n_elements, n_cascades, thresh, aabb, rng_calls, planes_out=None, idx_out=None, offset=0):
    """K6.  Default: -> (positions [n,3], indices [n]).  `planes_out` [3, m] + `idx_out` [m]: the n points go to columns
    [offset, offset + n) of the planes (and of idx_out) instead -- both calls of a grid refresh fill one buffer, no concatenation,
    and the density query reads the planes with coalesced loads."""
    L = _lib.load()
    dev = grid.device
    st, inc = pcg32_host_state(rng_calls)
    if planes_out is not None:
        if n_elements:
            _ptr(planes_out); _ptr(idx_out)
            _lib.check(L.xr_generate_grid_samples(_ptr(grid), ema_step, n_elements, n_cascades, thresh, aabb[0], aabb[1], st, inc,
                                                   C.c_void_p(planes_out.data_ptr() + 4 * offset), 1, planes_out.stride(0),
                                                   C.c_void_p(idx_out.data_ptr() + 4 * offset), _stream()), 'xr_generate_grid_samples')
        return planes_out[:, offset:offset + n_elements], idx_out[offset:offset + n_elements]
    pos = torch.empty((n_elements, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((n_elements,), dtype=torch.int32, device=dev)
    _lib.check(L.xr_generate_grid_samples(_ptr(grid), ema_step, n_elements, n_cascades, thresh, aabb[0], aabb[1],
                                          st, inc, _ptr(pos), 3, 1, _ptr(idx), _stream()), 'xr_generate_grid_samples')
    return pos, idx


def mark_untrained_density_grid(focal, xforms, n_elements, resolutions, grid=None):
    L = _lib.load()
    if grid is None:
        grid = torch.empty((n_elements,), dtype=torch.float32, device=focal.device)
    _lib.check(L.xr_mark_untrained_density_grid(_ptr(focal), _ptr(xforms), n_elements, xforms.shape[0],
                                                int(resolutions[0]), int(resolutions[1]), _ptr(grid), _stream()),
               'xr_mark_untrained_density_grid')
    return grid


def splat_grid_samples(mlp_out, indices, padded_width, n_samples, grid_tmp):
    """mlp_out may be a strided [n,1] view: `padded_width` is its row stride in floats."""
    if not _on_device(mlp_out):
        raise _lib.XrError('xrnerf_amd ops need ROCm device tensors: there is no CPU fallback')
    _lib.check(_lib.load().xr_splat_grid_samples(C.c_void_p(mlp_out.data_ptr()), _ptr(indices), padded_width, n_samples,
                                                 _ptr(grid_tmp), _stream()), 'xr_splat_grid_samples')
    return grid_tmp


def ema_grid_samples(grid_tmp, n_elements, decay, grid):
    _lib.check(_lib.load().xr_ema_grid_samples(_ptr(grid_tmp), n_elements, decay, _ptr(grid), _stream()),
               'xr_ema_grid_samples')
    return grid


def update_bitfield(grid, mean, bitfield):
    L = _lib.load()
    ws = _ws(grid.device, L.xr_update_bitfield_workspace_bytes(), 'k10')
    _lib.check(L.xr_update_bitfield(_ptr(grid), _ptr(mean), _ptr(bitfield), _ptr(ws), ws.numel(), _stream()),
               'xr_update_bitfield')
    return bitfield, mean


def ema_update_bitfield(grid_tmp, n_elements, decay, grid, mean, bitfield):
    """K9 + K10 + K11 of one refresh in three launches (xr_ema_update_bitfield) == ema_grid_samples then update_bitfield, bit for bit"""
    L = _lib.load()
    ws = _ws(grid.device, L.xr_update_bitfield_workspace_bytes(), 'k10')
    _lib.check(L.xr_ema_update_bitfield(_ptr(grid_tmp), n_elements, decay, _ptr(grid), _ptr(mean), _ptr(bitfield), _ptr(ws), ws.numel(), _stream()),
               'xr_ema_update_bitfield')
    return grid


def bitfield_from_mean(grid, mean, bitfield):
    _lib.check(_lib.load().xr_bitfield_from_mean(_ptr(grid), _ptr(mean), _ptr(bitfield), _stream()),
               'xr_bitfield_from_mean')
    return bitfield


# ---------------------------------------------------------------- hash grid / SH / MLP
class GridMeta:
    """Host-side level geometry (shared verbatim with the oracle)."""

    def __init__(self, n_levels=16, log2_hashmap_size=19, base_resolution=16, per_level_scale=None):
        if per_level_scale is None:
            per_level_scale = float(np.exp2(np.log2(2048 * 1 / 16) / (16 - 1)))  # hashnerf_mlp.py:17-20
        self.n_levels = int(n_levels)
        self.log2_hashmap_size = int(log2_hashmap_size)
        self.n_features = 2
        self.scale = np.zeros(n_levels, np.float32)
        self.resolution = np.zeros(n_levels, np.uint32)
        self.offset = np.zeros(n_levels + 1, np.uint32)
        _lib.load().xr_hashgrid_meta(n_levels, log2_hashmap_size, base_resolution, per_level_scale,
                                     self.scale.ctypes.data, self.resolution.ctypes.data, self.offset.ctypes.data)
        self.n_params = int(self.offset[-1]) * 2
        self.n_output_dims = 2 * self.n_levels

    def _args(self):
        return self.scale.ctypes.data, self.resolution.ctypes.data, self.offset.ctypes.data


def _pos_view(x):
    """(tensor, element stride) for an [n,>=3] fp32 position source: a contiguous [n,3] tensor, or
    the leading 3 columns of contiguous [n,7] coordinate rows (consumed in place)."""
    if x.dim() != 2 or x.shape[1] < 3 or x.dtype != torch.float32:
        raise _lib.XrError('positions must be a 2-D float32 tensor with >= 3 columns')
    if x.stride(1) != 1:
        raise _lib.XrError('positions must have unit column stride')
    if not _on_device(x):
        raise _lib.XrError('xrnerf_amd ops need ROCm device tensors (got a %s tensor): there is no CPU fallback' % x.device)
    return x, int(x.stride(0))


def clip_numsteps(numsteps, counter, max_compacted, out=None):
    """K2 without the copy (K1's output kept in place): clipped per-ray counts + the device-side count of valid
    rows n_valid [2] = (total, total)  (the C entry point can also split the count over row chunks).
    `out` = caller-owned (clipped [n,2] int32, n_valid [2] int32) buffers."""
    n = numsteps.shape[0]
    if out is not None:
        out, n_valid = out
    else:
        out = torch.empty_like(numsteps)
        n_valid = torch.empty((2,), dtype=torch.int32, device=numsteps.device)
    _lib.check(_lib.load().xr_clip_numsteps(_ptr(numsteps), _ptr(counter), n, 1, n, max_compacted, _ptr(out), _ptr(n_valid),
                                            _stream()), 'xr_clip_numsteps')
    return out, n_valid


def hashgrid_fwd(table, x, meta, enc_t=None, ld=None, n_dev=None, rows=None, row0=0, count=None, levels=None):
    """x: [n,3] (or a column slice of [n,7] rows), or positions as three planes [3, m] (m >= n: structure of arrays, three
    coalesced loads per sample) -> enc_t [2L, ld] feature-major.
    n_dev: optional device int32[1]; only min(n, n_dev) rows are touched (no host read-back needed).
    levels=(l0, l1): only that level range is evaluated (rows 2*l0 .. 2*l1 of enc_t; measurement / partial updates)."""
    L = _lib.load()
    if x.dim() == 2 and x.shape[0] == 3 and x.shape[1] != 3 and x.stride(1) == 1:      # planes [3, m]
        if x.dtype != torch.float32 or not _on_device(x):
            raise _lib.XrError('positions must be float32 device tensors')
        xs, xcs, n_x = 1, int(x.stride(0)), x.shape[1]
    else:
        x, xs = _pos_view(x)
        xcs, n_x = 1, x.shape[0]
    n = n_x if rows is None else rows.shape[0]
    if ld is None:
        ld = (n + 63) // 64 * 64
    if enc_t is None:
        enc_t = torch.empty((meta.n_output_dims, ld), dtype=torch.float32, device=x.device)
    s, r, o = meta._args()
    l0, l1 = (0, meta.n_levels) if levels is None else levels
    if not 0 <= l0 < l1 <= meta.n_levels:
        raise _lib.XrError('bad level range %r' % (levels,))
    if count is not None:          # a row chunk [row0, row0+count) of the sample buffer, written to the same columns
        n = count
    xp = x.data_ptr() + 4 * xs * row0
    ep = enc_t.data_ptr() + 4 * (row0 + 2 * l0 * ld)
    with _span('xr_hashgrid_fwd', 0 if n_dev is not None else n, train=n_dev is not None):
        _ptr(enc_t)
        _lib.check(L.xr_hashgrid_fwd(_ptr(table), C.c_void_p(xp), xs, xcs, n, _ptr(n_dev), _ptr(rows), l1 - l0, s + 4 * l0, r + 4 * l0,
                                      o + 4 * l0, C.c_void_p(ep), ld, _stream()), 'xr_hashgrid_fwd')
    return enc_t


def hashgrid_bwd(x, denc_t, meta, grad_table, n_dev=None, row0=0, count=None, levels=None, use_workspace=True, live=None,
                 overwrite=False):
    """scatter dL/denc into dL/dtable.  `levels=(l0, l1)` restricts the launch to that level range (the level
    metadata arrays are passed from l0 on; table offsets are absolute, so `grad_table` stays the full table):
    the data-parallel trainer scatters the fine half first and reduces it across ranks under the coarse half.
    `live=(rows, n_live)` (ops.live_rows): only the listed rows are scattered.
    `overwrite=True` (XR_SCATTER_OVERWRITE): the levels' slices of grad_table are written instead of added to."""
    L = _lib.load()
    _ensure_helper(denc_t.device)
    x, xs = _pos_view(x)
    n = x.shape[0] if count is None else count
    s, r, o = meta._args()
    l0, l1 = (0, meta.n_levels) if levels is None else levels
    if not 0 <= l0 < l1 <= meta.n_levels:
        raise _lib.XrError('bad level range %r' % (levels,))
    ld = denc_t.shape[1]
    _ptr(denc_t)
    ws = _ws(x.device, L.xr_hashgrid_bwd_workspace_bytes(n, l1 - l0, r + 4 * l0, o + 4 * l0), 'hgb') if use_workspace else None
    rows = None
    if live is not None:
        if row0:
            raise _lib.XrError('a live-row list addresses rows from 0')
        rows, n_dev = live
    with _span('xr_hashgrid_bwd', 0 if n_dev is not None else n, train=n_dev is not None):
        _lib.check(L.xr_hashgrid_bwd(C.c_void_p(x.data_ptr() + 4 * xs * row0), xs,
                                      C.c_void_p(denc_t.data_ptr() + 4 * (row0 + 2 * l0 * ld)), ld, n, _ptr(n_dev), _ptr(rows),
                                      l1 - l0, s + 4 * l0, r + 4 * l0, o + 4 * l0, _ptr(grad_table),
                                      _ptr(ws), ws.numel() if ws is not None else 0, 1 if overwrite else 0, _stream()),
                   'xr_hashgrid_bwd')
    return grad_table


def adam_fuse(param, m, v, ema, step, lr, beta1, beta2, eps, weight_decay, ema_momentum=0.0, grad_scale=1.0):
    """-> xr_adam_fuse for hashgrid_bwd_adam / ngp_train_step(adam=): whole tensors + this update's constants (keeps the tensors alive)"""
    a = _lib.AdamFuse(param.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr() if ema is not None else None, int(step), float(lr),
                      float(beta1), float(beta2), float(eps), float(weight_decay), float(ema_momentum), float(grad_scale), param.numel())
    a._keep = (param, m, v, ema)
    for t in a._keep:
        if t is not None:
            _ptr(t)                       # device / contiguity check
    return a


def hashgrid_bwd_adam_supported(n, meta):
    """every level of `meta` has a non-atomic scatter path at a capacity of n rows (what the fused update needs)"""
    s, r, o = meta._args()
    return _lib.load().xr_hashgrid_bwd_adam(None, 0, None, 0, int(n), None, None, meta.n_levels, s, r, o, None, 0, None, None) == 0       # (adam = NULL: the dry run)


def hashgrid_bwd_adam(x, denc_t, meta, adam, n_dev=None, live=None, count=None):
    """the table scatter with the optimiser's update in place of the gradient write (xr_hashgrid_bwd_adam): the tensors named
    by `adam` (ops.adam_fuse) are updated exactly as hashgrid_bwd(overwrite=True) + adam_step_multi would; no gradient is produced"""
    L = _lib.load()
    _ensure_helper(denc_t.device)
    x, xs = _pos_view(x)
    n = x.shape[0] if count is None else count
    s, r, o = meta._args()
    ws = _ws(x.device, L.xr_hashgrid_bwd_workspace_bytes(n, meta.n_levels, r, o), 'hgb')
    rows = None
    if live is not None:
        rows, n_dev = live
    with _span('xr_hashgrid_bwd', 0 if n_dev is not None else n, train=n_dev is not None):
        _lib.check(L.xr_hashgrid_bwd_adam(C.c_void_p(x.data_ptr()), xs, _ptr(denc_t), denc_t.shape[1], n, _ptr(n_dev), _ptr(rows),
                                          meta.n_levels, s, r, o, _ptr(ws), ws.numel(), C.byref(adam), _stream()), 'xr_hashgrid_bwd_adam')


def sh4(dirs):
    dirs, ds = _pos_view(dirs)
    n = dirs.shape[0]
    out = torch.empty((n, 16), dtype=torch.float32, device=dirs.device)
    _lib.check(_lib.load().xr_sh4(C.c_void_p(dirs.data_ptr()), ds, n, _ptr(out), _stream()), 'xr_sh4')
    return out


# ---- deeper tiny MLPs than the fused kernels are built for --------------------------------------------------------
# tiny-cuda-nn's key for the depth is `n_hidden_layers` (default 5); the reference config writes `num_layers`
# (configs/instant_ngp/nerf_blender_local01.py:106-124, passed unchanged by xrnerf/models/mlps/hashnerf_mlp.py:39-45), so a
# checkpoint of the real reference may hold 5-hidden-layer nets (19 456 floats each; SURVEY.md section 2c, XRNERF_TCNN_STRICT_DEFAULTS).
# The (1, 2) kernels keep every activation of both nets in registers and both weight sets in LDS.  Any other depth up to 8 + 8
# hidden layers -- tcnn's default 5 + 5 first of all -- runs on the STREAMED fused kernels (k_nerf_mlp_fwd_deep / _bwd_deep: a
# workgroup takes its sample tiles through one layer at a time, the layers' weights pass through LDS), round 5.  The layer-by-layer
# path on the fp32 linear kernels of csrc/xr_gemm.hip (activations through HBM; rounds 3-4) stays as the independent statement the
# tests hold the fused kernels against (empty these two tuples to take it).
MAX_HIDDEN = 8          # XR_MLP_MAX_HIDDEN (csrc/xr_mlp.hip)
_FUSED_FWD = tuple((a, b) for a in range(1, MAX_HIDDEN + 1) for b in range(1, MAX_HIDDEN + 1))
_FUSED_BWD = _FUSED_FWD


def _net_layers(w_flat, n_hidden, n_in=32, width=64, n_out=16):
    """views [out, in] of a flat FullyFusedMLP parameter vector (row-major matrices in layer order)"""
    dims = [n_in] + [width] * n_hidden + [n_out]
    out, o = [], 0
    for a, b in zip(dims[:-1], dims[1:]):
        out.append(w_flat[o:o + a * b].view(b, a))
        o += a * b
    if o != w_flat.numel():
        raise _lib.XrError('parameter vector of %d floats does not hold %d hidden layers' % (w_flat.numel(), n_hidden))
    return out


def _layered_net(x, w_flat, n_hidden):
    from .linear import linear_act
    ws = _net_layers(w_flat, n_hidden)
    h = x
    for w in ws[:-1]:
        h = linear_act(h, w, None, True)
    return linear_act(h, ws[-1], None, False)


def _valid_rows(x, n_dev):
    """contiguous copy of the row-major [m, c] tensor `x` with the rows behind the device-side count n_dev[0] set to zero"""
    if n_dev is None:
        return x.contiguous()
    keep = torch.arange(x.shape[0], device=x.device)[:, None] < n_dev.reshape(-1)[:1].to(torch.int64)
    return torch.where(keep, x, torch.zeros((), dtype=x.dtype, device=x.device)).contiguous()


def _layered_nerf_mlp(enc, dirs, w_density, w_color, nhd, nhc, pad_value):
    """enc [n,32] (, dirs [n,3]) -> raw [n,4] = [rgb raw, sigma raw]; differentiable w.r.t. enc, w_density, w_color"""
    dout = _layered_net(enc, w_density, nhd)
    if dirs is None:
        z = torch.zeros((enc.shape[0], 3), dtype=torch.float32, device=enc.device)
        return torch.cat([z, dout[:, :1]], 1)
    cin = torch.cat([dout[:, 1:16], sh4(dirs), torch.full((enc.shape[0], 1), float(pad_value), dtype=torch.float32, device=enc.device)], 1)
    cout = _layered_net(cin, w_color, nhc)
    return torch.cat([cout[:, :3], dout[:, :1]], 1)


def nerf_mlp_fwd(enc_t, dirs, n, w_density, w_color, nhd, nhc, pad_value=1.0, raw=None, n_dev=None, rows=None, row0=0,
                 count=None):
    L = _lib.load()
    if (nhd, nhc) not in _FUSED_FWD:
        if rows is not None:
            raise _lib.XrError('row lists are served by the fused kernels only (hidden layers %d, %d)' % (nhd, nhc))
        m = n if count is None else count
        with torch.no_grad(), _span('xr_nerf_mlp_fwd', 0 if n_dev is not None else m, train=n_dev is not None):
            enc = _valid_rows(enc_t[:, row0:row0 + m].t(), n_dev)
            d = _pos_view(dirs)[0][row0:row0 + m] if dirs is not None else None
            out = _layered_nerf_mlp(enc, d.contiguous() if d is not None and d.stride(0) != 3 else d, w_density.detach(),
                                    w_color.detach() if w_color is not None else None, nhd, nhc, pad_value)
        if raw is None:
            raw = torch.empty((n, 4), dtype=torch.float32, device=enc_t.device)
        raw[row0:row0 + m] = out
        return raw
    if raw is None:
        raw = torch.empty((n, 4), dtype=torch.float32, device=enc_t.device)
    if dirs is not None:
        dirs, ds = _pos_view(dirs)
        dp = C.c_void_p(dirs.data_ptr() + 4 * ds * row0)
    else:
        ds, dp = 0, None
    _ptr(enc_t); _ptr(raw)
    if count is not None:
        n = count
    mlp_range_word(enc_t.device)
    with _span('xr_nerf_mlp_fwd', 0 if n_dev is not None else n, train=n_dev is not None):
        _lib.check(L.xr_nerf_mlp_fwd(_mlp_mode(nhd, nhc), C.c_void_p(enc_t.data_ptr() + 4 * row0), enc_t.shape[1], dp, ds, n, _ptr(n_dev),
                                     _ptr(rows), _ptr(w_density), _ptr(w_color) if w_color is not None else None, nhd,
                                     nhc, pad_value, C.c_void_p(raw.data_ptr() + 16 * row0), _stream()),
                   'xr_nerf_mlp_fwd')
    return raw


def nerf_density_splat(enc_t, n, w_density, nhd, nhc, indices, grid_tmp):
    """K9's density query + K8 in one launch: the density network over the n encoded points of enc_t, exp(density) * min_step merged into
    grid_tmp[indices[i]] by maximum from the forward kernel's epilogue (fused topologies only: see density_splat_supported)"""
    if indices.dtype != torch.int32 or grid_tmp.dtype != torch.float32:
        raise _lib.XrError('nerf_density_splat: int32 indices, float32 grid')
    mlp_range_word(enc_t.device)
    with _span('xr_nerf_mlp_fwd', n, train=False):
        _lib.check(_lib.load().xr_nerf_density_splat(_mlp_mode(nhd, nhc), _ptr(enc_t), enc_t.shape[1], n, _ptr(w_density), nhd, nhc, _ptr(indices),
                                                     _ptr(grid_tmp), _stream()), 'xr_nerf_density_splat')


def density_splat_supported(nhd, nhc):
    return (nhd, nhc) in _FUSED_FWD and (_PRECISION != 'f16' or (nhd, nhc) == (1, 2))


LIVE_STATS = None      # the backward's 4-word count block (words 1, 2: running live / valid row totals; clear to restart)


def _list_slots(dev, n, nhd=1, nhc=2):
    """the list area of the MLP backward's workspace for n rows (at its start, whatever the topology the workspace is sized for)
    -> (workspace, rows view, seg pointer, count-block view)"""
    L = _lib.load()
    ws = _ws(dev, L.xr_nerf_mlp_bwd_workspace_bytes(n, nhd, nhc), 'mlpbwd')
    p_rows, p_seg, p_cnt = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _lib.check(L.xr_nerf_mlp_bwd_list_slots(_ptr(ws), ws.numel(), n, C.byref(p_rows), C.byref(p_seg), C.byref(p_cnt)),
               'xr_nerf_mlp_bwd_list_slots')
    base = ws.data_ptr()
    rows = ws[p_rows.value - base:p_rows.value - base + 4 * n].view(torch.int32)
    cnt = ws[p_cnt.value - base:p_cnt.value - base + 16].view(torch.int32)   # [count, running live total, running valid total, spare]
    return ws, rows, p_seg, cnt


def train_loss_scalars(rgb, target, alpha, delta=0.1, scale=5.0, out=None):
    """-> out[2] = (scale * sum HuberLoss(rgb - target), sum ((rgb - target) * alpha)^2), written by one fixed-order sum"""
    if out is None:
        out = torch.empty((2,), dtype=torch.float32, device=rgb.device)
    _lib.check(_lib.load().xr_train_loss_scalars(_ptr(rgb), _ptr(target), _ptr(alpha), rgb.shape[0], float(delta), float(scale),
                                                 _ptr(out), _stream()), 'xr_train_loss_scalars')
    return out


def live_segments(n):
    """number of 1024-row segments of n rows (length of the compositor's live-row count array)"""
    return (int(n) + _lib.LIVE_SEGMENT_ROWS - 1) // _lib.LIVE_SEGMENT_ROWS


def live_rows(draw, n, n_dev=None, zero_denc_t=None, seg_counts=None):
    """-> (rows int32 [n], n_live int32 [4]) on the device: the rows of dL/d(raw) [n,4] that are not exactly zero, in
    order (xr_live_rows); n_live[0] is the count.  Handed to nerf_mlp_bwd and hashgrid_bwd as `live=`.  The list sits in
    the MLP backward's workspace (where xr_ngp_train_step keeps it too) and is overwritten by the next call.
    seg_counts: the per-segment counts composite_train(..., live_seg=) left (one launch less: the ranking pass only)."""
    global LIVE_STATS
    _, rows, p_seg, n_live = _list_slots(draw.device, n)
    LIVE_STATS = n_live
    with _span('xr_live_rows', 0 if n_dev is not None else n, train=n_dev is not None):
        _lib.check(_lib.load().xr_live_rows(_ptr(draw), n, _ptr(n_dev), p_seg if seg_counts is None else _ptr(seg_counts), _ptr(rows),
                                             _ptr(n_live), _ptr(zero_denc_t), zero_denc_t.shape[1] if zero_denc_t is not None else 0,
                                             0 if seg_counts is None else 1, _stream()), 'xr_live_rows')
    return rows, n_live


def nerf_mlp_bwd(enc_t, dirs, n, w_density, w_color, nhd, nhc, draw, grad_wd, grad_wc, pad_value=1.0, denc_t=None,
                 n_dev=None, row0=0, count=None, live=None):
    """`live=(rows, n_live)` (ops.live_rows(draw, ...)): the backward computes the listed rows only and leaves the other
    rows of denc_t untouched -- pass the same list to hashgrid_bwd.  Without it the call builds its own list and writes
    exact zeros to the dead rows (identical results to the backward over every row)."""
    L = _lib.load()
    if (nhd, nhc) not in _FUSED_BWD:
        # layer by layer: recompute the forward under autograd, back-propagate dL/d(raw); rows outside a live list have an
        # exactly-zero dL/d(raw) and get an exactly-zero dL/d(encoding) (a superset of the fused contract, which leaves them alone)
        m = n if count is None else count
        if denc_t is None:
            denc_t = torch.empty_like(enc_t)
        with _span('xr_nerf_mlp_bwd', 0 if n_dev is not None else m, train=n_dev is not None):
            d = _pos_view(dirs)[0][row0:row0 + m]
            d = d.contiguous() if d.stride(0) != 3 else d
            with torch.enable_grad():
                # rows behind the device-side count are padding of a fixed-size buffer that nothing wrote this step (the encode and the
                # compositor stop at the count): whatever they hold -- stale rows, NaN bit patterns of fresh memory -- is replaced by
                # zeros, not multiplied by zero (0 * NaN), in the features AND in the incoming gradient
                enc = _valid_rows(enc_t[:, row0:row0 + m].t(), n_dev).requires_grad_(True)
                wd, wc = w_density.detach().requires_grad_(True), w_color.detach().requires_grad_(True)
                out = _layered_nerf_mlp(enc, d, wd, wc, nhd, nhc, pad_value)
                g = _valid_rows(draw[row0:row0 + m], n_dev)
                ge, gwd, gwc = torch.autograd.grad(out, [enc, wd, wc], grad_outputs=g)
            denc_t[:, row0:row0 + m] = ge.t()
            grad_wd.add_(gwd)
            grad_wc.add_(gwc)
        return denc_t
    dirs, ds = _pos_view(dirs)
    if denc_t is None:
        denc_t = torch.empty_like(enc_t)
    ws = _ws(enc_t.device, L.xr_nerf_mlp_bwd_workspace_bytes(n, nhd, nhc), 'mlpbwd')
    _ptr(enc_t); _ptr(draw); _ptr(denc_t)
    if count is not None:
        n = count
    with _span('xr_nerf_mlp_bwd', 0 if n_dev is not None else n, train=n_dev is not None):
        _lib.check(L.xr_nerf_mlp_bwd(_mlp_mode(nhd, nhc), C.c_void_p(enc_t.data_ptr() + 4 * row0), enc_t.shape[1], C.c_void_p(dirs.data_ptr() + 4 * ds * row0), ds, n, _ptr(n_dev), _ptr(w_density),
                                     _ptr(w_color), nhd, nhc, pad_value, C.c_void_p(draw.data_ptr() + 16 * row0), C.c_void_p(denc_t.data_ptr() + 4 * row0), _ptr(grad_wd),
                                     _ptr(grad_wc), _ptr(ws), ws.numel(), _ptr(live[0]) if live is not None else None,
                                     _ptr(live[1]) if live is not None else None, _stream()), 'xr_nerf_mlp_bwd')
    return denc_t


# ---------------------------------------------------------------- callers either side
def gen_rays(pose43, H, W, fx, fy, cx, cy, row0=0, nrows=None, device='cuda'):
    pose = np.ascontiguousarray(np.asarray(pose43, dtype=np.float32).reshape(4, 3))
    nrows = H - row0 if nrows is None else nrows
    o = torch.empty((nrows * W, 3), dtype=torch.float32, device=device)
    d = torch.empty((nrows * W, 3), dtype=torch.float32, device=device)
    _lib.check(_lib.load().xr_gen_rays(pose.ctypes.data, H, W, fx, fy, cx, cy, row0, nrows, _ptr(o), _ptr(d),
                                       _stream()), 'xr_gen_rays')
    return o, d


def huber_loss_grad(rgb, target, delta=0.1, scale=5.0):
    grad = torch.empty_like(rgb)
    loss = torch.zeros((1,), dtype=torch.float32, device=rgb.device)
    _lib.check(_lib.load().xr_huber_loss_grad(_ptr(rgb), _ptr(target), None, rgb.numel(), delta, scale, _ptr(grad),
                                              _ptr(loss), _stream()), 'xr_huber_loss_grad')
    return loss, grad


def huber_loss_grad_mse(rgb, target, alpha, delta=0.1, scale=5.0, out=None):
    """-> out[2] = (scale * HuberLoss_sum, sum ((rgb-target)*alpha)^2), dL/drgb; `out` must be zero-filled"""
    grad = torch.empty_like(rgb)
    if out is None:
        out = torch.zeros((2,), dtype=torch.float32, device=rgb.device)
    _lib.check(_lib.load().xr_huber_loss_grad(_ptr(rgb), _ptr(target), _ptr(alpha), 3 * rgb.shape[0], delta, scale,
                                              _ptr(grad), _ptr(out), _stream()), 'xr_huber_loss_grad')
    return out, grad


def make_batch_buffers(capacity, device):
    """caller-owned output buffers for make_batch(out=...), `capacity` rays"""
    f = lambda c: torch.empty((capacity, c), dtype=torch.float32, device=device)
    return {'rays_o': f(3), 'rays_d': f(3), 'target_s': f(3), 'alpha': f(1), 'bg_color': f(3),
            'img_ids': torch.empty((capacity, 1), dtype=torch.int32, device=device)}


def make_batch(rows, n, call_index, seed=20220901, out=None):
    """rows: contiguous [>=n, 11] slice of the device-resident ray table -> dict of batch tensors
    (views of `out`'s buffers when given: no allocation, nothing for the caching allocator to track across streams)"""
    dev = rows.device
    if out is not None:
        o, d, tgt, alpha, bg, ids = (out[k][:n] for k in ('rays_o', 'rays_d', 'target_s', 'alpha', 'bg_color', 'img_ids'))
    else:
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        o, d, tgt, alpha, bg = f(n, 3), f(n, 3), f(n, 3), f(n, 1), f(n, 3)
        ids = torch.empty((n, 1), dtype=torch.int32, device=dev)
    st, inc = pcg32_host_state(call_index, seed)
    # (one batch = a series of one: rows from the slice's first row, the generator of call `call_index`)
    _lib.check(_lib.load().xr_make_batch_series(_ptr(rows), (C.c_uint64 * 1)(0), n, 1, n, st, inc, _ptr(o), _ptr(d), _ptr(tgt), _ptr(alpha),
                                                _ptr(bg), _ptr(ids), _stream()), 'xr_make_batch_series')
    return {'rays_o': o, 'rays_d': d, 'target_s': tgt, 'alpha': alpha, 'img_ids': ids, 'bg_color': bg}


def adam_step(p, g, m, v, step, lr=1e-2, beta1=0.9, beta2=0.99, eps=1e-15, weight_decay=1e-6, ema=None,
              ema_momentum=0.05):
    adam_step_multi([p], [g], [m], [v], step, lr, beta1, beta2, eps, weight_decay, [ema] if ema is not None else None, ema_momentum)


def scale_multi(ts, scale_dev=None, host_factor=1.0):
    """ts[k] *= scale_dev * host_factor in one launch (no memory traffic when the factor is exactly 1)"""
    k = len(ts)
    for t in ts:
        _ptr(t)
    arr = (C.c_void_p * k)(*[t.data_ptr() for t in ts])
    ns = (C.c_size_t * k)(*[t.numel() for t in ts])
    _lib.check(_lib.load().xr_scale_multi(k, arr, ns, _ptr(scale_dev), float(host_factor), _stream()), 'xr_scale_multi')


def adam_step_multi(ps, gs, ms, vs, step, lr=1e-2, beta1=0.9, beta2=0.99, eps=1e-15, weight_decay=1e-6, emas=None,
                    ema_momentum=0.05, grad_scale=1.0):
    """one launch for up to 4 tensors; `grad_scale` multiplies the gradients as they are read (the buffers stay as they are)"""
    k = len(ps)
    arr = lambda ts: (C.c_void_p * k)(*[t.data_ptr() if t is not None else None for t in ts])
    for t in list(ps) + list(gs) + list(ms) + list(vs):
        _ptr(t)     # validates device / contiguity
    ns = (C.c_size_t * k)(*[p.numel() for p in ps])
    with _span('xr_adam_step', sum(p.numel() for p in ps)):
        _lib.check(_lib.load().xr_adam_step_multi(k, arr(ps), arr(gs), arr(ms), arr(vs), arr(emas) if emas else None, ns,
                                                  step, lr, beta1, beta2, eps, weight_decay, ema_momentum, float(grad_scale),
                                                  _stream()),
                   'xr_adam_step_multi')


# ---------------------------------------------------------------- Mip-NeRF stages (BASELINE config #3)
def _f32c(t):
    if t.dtype != torch.float32:
        raise _lib.XrError('xrnerf_amd mip ops take float32 tensors (got %s)' % t.dtype)
    return t if t.is_contiguous() else t.contiguous()


def mip_zvals(near, far, n_z, lindisp=False, z_rand=None):
    """GetZvals (create.py:486-531): near/far [R] or [R,1]; z_rand [R,n_z] uniform draws or None -> [R,n_z]"""
    near, far = _f32c(near.reshape(-1)), _f32c(far.reshape(-1))
    R = near.shape[0]
    out = torch.empty((R, n_z), dtype=torch.float32, device=near.device)
    if z_rand is not None:
        z_rand = _f32c(z_rand)
        assert tuple(z_rand.shape) == (R, n_z)
    _lib.check(_lib.load().xr_mip_zvals(_ptr(near), _ptr(far), R, n_z, int(bool(lindisp)), _ptr(z_rand), _ptr(out),
                                        _stream()), 'xr_mip_zvals')
    return out


def mip_encode_channels(min_deg, max_deg, min_deg_view, max_deg_view, append_identity=True):
    return int(_lib.load().xr_mip_encode_channels(min_deg, max_deg, min_deg_view, max_deg_view, int(bool(append_identity))))


def mip_encode(rays_o, rays_d, viewdirs, radii, z_vals, min_deg, max_deg, min_deg_view, max_deg_view,
               append_identity=True, ray_shape='cone', out=None):
    """cast_rays + integrated_pos_enc + pos_enc + concat in one launch -> [R*(n_z-1), channels]"""
    L = _lib.load()
    R, n_z = z_vals.shape
    ch = mip_encode_channels(min_deg, max_deg, min_deg_view, max_deg_view, append_identity)
    if out is None:
        # rows padded to a multiple of 4 floats: the encoding (123 channels in the reference's config) is then a [M, ch] view whose rows start
        # on 16-byte boundaries, which the linear kernels read in place (ops._rows) -- no contiguous copy of the first layer's input
        out = torch.empty((R * (n_z - 1), (ch + 3) // 4 * 4), dtype=torch.float32, device=z_vals.device)[:, :ch]
    if not _on_device(out) or out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[1] < ch:
        raise _lib.XrError('mip_encode: out must be a float32 device matrix with contiguous rows of >= %d channels' % ch)
    shape = {'cone': 0, 'cylinder': 1}[ray_shape]
    with _span('xr_mip_encode', R * (n_z - 1)):
        _lib.check(L.xr_mip_encode(_ptr(_f32c(rays_o)), _ptr(_f32c(rays_d)), _ptr(_f32c(viewdirs)),
                                   _ptr(_f32c(radii.reshape(-1))), _ptr(_f32c(z_vals)), R, n_z, min_deg, max_deg,
                                   min_deg_view, max_deg_view, int(bool(append_identity)), shape, C.c_void_p(out.data_ptr()),
                                   out.stride(0), _stream()), 'xr_mip_encode')
    return out


def mip_encode_gaussians(means, covs, viewdirs, min_deg, max_deg, min_deg_view, max_deg_view, append_identity=True):
    L = _lib.load()
    R, S = means.shape[:2]
    ch = mip_encode_channels(min_deg, max_deg, min_deg_view, max_deg_view, append_identity)
    out = torch.empty((R * S, ch), dtype=torch.float32, device=means.device)
    _lib.check(L.xr_mip_encode_gaussians(_ptr(_f32c(means)), _ptr(_f32c(covs)), _ptr(_f32c(viewdirs)), R, S, min_deg,
                                         max_deg, min_deg_view, max_deg_view, int(bool(append_identity)), _ptr(out),
                                         ch, _stream()), 'xr_mip_encode_gaussians')
    return out


_MIP_ACT = {'softplus': 0, 'relu': 1}


def _render_outputs(R, S, dev):
    """what every dense renderer's forward writes: rgb [R,3], the ray's scalar (disparity or distance) [R], acc [R], weights [R,S]"""
    return (torch.empty((R, 3), dtype=torch.float32, device=dev), torch.empty((R,), dtype=torch.float32, device=dev),
            torch.empty((R,), dtype=torch.float32, device=dev), torch.empty((R, S), dtype=torch.float32, device=dev))


def _render_noise(noise, R, S):
    """the optional density noise of the vanilla and Bungee renderers: float32, contiguous, one value per sample"""
    if noise is None:
        return None
    noise = _f32c(noise)
    if tuple(noise.shape) != (R, S):
        raise _lib.XrError('noise must be [R, S]')
    return noise


def mip_render_forward(raw, z_vals, rays_d, density_bias, rgb_padding, white_bkgd, density_activation='softplus'):
    """-> rgb [R,3], distance [R], acc [R], weights [R,S]"""
    L = _lib.load()
    R, n_z = z_vals.shape
    raw = _f32c(raw)
    assert tuple(raw.shape) == (R, n_z - 1, 4), 'raw must be [R, n_z-1, 4] (rgb + density)'
    rgb, dist, acc, w = _render_outputs(R, n_z - 1, raw.device)
    with _span('xr_mip_render_forward', R * (n_z - 1)):
        _lib.check(L.xr_mip_render_forward(_ptr(raw), _ptr(_f32c(z_vals)), _ptr(_f32c(rays_d)), R, n_z,
                                           float(density_bias), float(rgb_padding), int(bool(white_bkgd)),
                                           _MIP_ACT[density_activation], _ptr(rgb), _ptr(dist), _ptr(acc), _ptr(w),
                                           _stream()), 'xr_mip_render_forward')
    return rgb, dist, acc, w


def mip_render_backward(raw, z_vals, rays_d, grad_rgb, density_bias, rgb_padding, white_bkgd,
                        density_activation='softplus'):
    L = _lib.load()
    R, n_z = z_vals.shape
    raw = _f32c(raw)
    out = torch.empty_like(raw)
    with _span('xr_mip_render_backward', R * (n_z - 1)):
        _lib.check(L.xr_mip_render_backward(_ptr(raw), _ptr(_f32c(z_vals)), _ptr(_f32c(rays_d)), _ptr(_f32c(grad_rgb)),
                                            R, n_z, float(density_bias), float(rgb_padding), int(bool(white_bkgd)),
                                            _MIP_ACT[density_activation], _ptr(out), _stream()),
                   'xr_mip_render_backward')
    return out


def mip_resample(z_vals, weights, resample_padding, rand=None):
    """resample_along_rays' new (detached) z_vals [R,n_z]; rand [R,n_z] uniform draws (randomized) or None"""
    L = _lib.load()
    R, n_z = z_vals.shape
    z_vals, weights = _f32c(z_vals), _f32c(weights.detach())
    assert tuple(weights.shape) == (R, n_z - 1)
    if rand is not None:
        rand = _f32c(rand)
        assert tuple(rand.shape) == (R, n_z)
    out = torch.empty_like(z_vals)
    with _span('xr_mip_resample', R):
        _lib.check(L.xr_mip_resample(_ptr(z_vals), _ptr(weights), _ptr(rand), float(resample_padding), R, n_z, _ptr(out),
                                     _stream()), 'xr_mip_resample')
    return out


# ---------------------------------------------------------------- KiloNeRF rendering (BASELINE config #5)
def kilo_param_floats(pos_freqs, dir_freqs, n_hidden):
    return int(_lib.load().xr_kilo_param_floats(pos_freqs, dir_freqs, n_hidden))


_KILO_WS_GEN = [0, 0]     # [count bumped by every call that rewrites the 'kilo' workspace's assignment arrays, that workspace's address]


def kilo_ws_generation():
    return _KILO_WS_GEN[0]


def kilo_pack_params(tensors, pos_freqs, dir_freqs, n_hidden, out=None):
    """MultiNetwork.ordered_parameters() -> the packed blocks [N, stride] the kernels take, in one launch (xr_kilo_pack_params)"""
    L = _lib.load()
    N = tensors[0].shape[0]
    stride = int(L.xr_kilo_param_floats(int(pos_freqs), int(dir_freqs), int(n_hidden)))
    ts = [_f32c(t.detach()) for t in tensors]
    if out is None:
        out = torch.empty((N, stride), dtype=torch.float32, device=ts[0].device)
    arr = (C.c_void_p * len(ts))(*[_ptr(t).value for t in ts])
    _lib.check(L.xr_kilo_pack_params(arr, N, int(pos_freqs), int(dir_freqs), int(n_hidden), _ptr(out), out.stride(0), _stream()), 'xr_kilo_pack_params')
    return out


def kilo_unpack_grads(blocks, like, pos_freqs, dir_freqs, n_hidden, clear=True):
    """the packed gradient blocks -> one contiguous tensor per parameter of `like` (views of ONE allocation), in one launch; clear: the
    blocks are left zero-filled for the next backward"""
    L = _lib.load()
    sizes = [t.numel() for t in like]
    flat = torch.empty((sum(sizes),), dtype=torch.float32, device=blocks.device)
    outs, o = [], 0
    for t, n in zip(like, sizes):
        outs.append(flat[o:o + n].view(t.shape))
        o += n
    arr = (C.c_void_p * len(outs))(*[t.data_ptr() for t in outs])
    _lib.check(L.xr_kilo_unpack_grads(_ptr(blocks), blocks.stride(0), blocks.shape[0], int(pos_freqs), int(dir_freqs), int(n_hidden), arr,
                                      1 if clear else 0, _stream()), 'xr_kilo_unpack_grads')
    return outs


def kilo_mlp_forward(viewdirs, gmin, gmax, fixed_res, occ_res, occupancy, domain_mins, domain_maxs, params, pos_freqs,
                     dir_freqs, n_hidden, pts=None, rays_o=None, rays_d=None, z_vals=None, want_counts=False):
    """KiloNerfMLP.forward: raw [R,S,4] (zeros where no network is evaluated) (+ batch_size_per_network [N] int32).
    Samples: pts [R,S,3], or rays_o/rays_d [R,3] + z_vals [R,S] (o + d*z, never materialised).
    gmin/gmax: 3 python floats; fixed_res/occ_res: 3 ints; occupancy: bool/uint8 device grid or None."""
    L = _lib.load()
    if pts is not None:
        pts = _f32c(pts)
        R, S = pts.shape[0], pts.shape[1]
        dev = pts.device
    else:
        rays_o, rays_d, z_vals = _f32c(rays_o), _f32c(rays_d), _f32c(z_vals)
        R, S = z_vals.shape
        dev = z_vals.device
    N = params.shape[0]
    raw = torch.empty((R, S, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((N,), dtype=torch.int32, device=dev) if want_counts else None
    ws = _ws(dev, L.xr_kilo_workspace_bytes(R * S, N), 'kilo')
    _KILO_WS_GEN[0] += 1              # the workspace now holds THIS call's assignment (kilo_mlp_backward(reuse=...) checks the count
    _KILO_WS_GEN[1] = ws.data_ptr()   # ... and that it is handed the same memory)
    if occupancy is not None:
        occupancy = occupancy.reshape(-1)
        if occupancy.dtype == torch.bool:
            occupancy = occupancy.view(torch.uint8)
        if occupancy.dtype != torch.uint8:
            raise _lib.XrError('occupancy grid must be bool or uint8')
    f3 = (C.c_float * 3)
    i3 = (C.c_int32 * 3)
    with _span('xr_kilo_mlp_forward', R * S):
        _lib.check(L.xr_kilo_mlp_forward(_ptr(pts), _ptr(rays_o), _ptr(rays_d), _ptr(z_vals), _ptr(_f32c(viewdirs)), R, S,
                                         f3(*[float(v) for v in gmin]), f3(*[float(v) for v in gmax]),
                                         i3(*[int(v) for v in fixed_res]), i3(*[int(v) for v in occ_res]) if occ_res is not None else None,
                                         _ptr(occupancy), _ptr(_f32c(domain_mins)), _ptr(_f32c(domain_maxs)), _ptr(params),
                                         params.stride(0), N, int(pos_freqs), int(dir_freqs), int(n_hidden), _ptr(raw),
                                         _ptr(counts), _ptr(ws), ws.numel(), _stream()), 'xr_kilo_mlp_forward')
    return (raw, counts) if want_counts else raw


def kilo_mlp_backward(draw, viewdirs, gmin, gmax, fixed_res, occ_res, occupancy, domain_mins, domain_maxs, params, pos_freqs,
                      dir_freqs, n_hidden, pts=None, rays_o=None, rays_d=None, z_vals=None, reuse_generation=None, grad=None):
    """gradient of the packed parameter blocks [N, stride] for dL/draw [R,S,4] (same sample arguments as the forward).
    reuse_generation: kilo_ws_generation() as it stood right after the forward call on these samples -- if nothing has touched the
    workspace since, the assignment / offsets / scatter launches are skipped.  grad: a zero-filled [N, stride] buffer to accumulate into."""
    L = _lib.load()
    draw = _f32c(draw)
    if pts is not None:
        pts = _f32c(pts)
        R, S = pts.shape[0], pts.shape[1]
    else:
        rays_o, rays_d, z_vals = _f32c(rays_o), _f32c(rays_d), _f32c(z_vals)
        R, S = z_vals.shape
    dev = draw.device
    N = params.shape[0]
    if grad is None:
        grad = torch.zeros_like(params)
    ws = _ws(dev, L.xr_kilo_workspace_bytes(R * S, N), 'kilo')
    reuse = reuse_generation is not None and reuse_generation == _KILO_WS_GEN[0] and ws.data_ptr() == _KILO_WS_GEN[1]
    if not reuse:
        _KILO_WS_GEN[0] += 1
    if occupancy is not None:
        occupancy = occupancy.reshape(-1)
        if occupancy.dtype == torch.bool:
            occupancy = occupancy.view(torch.uint8)
    f3 = (C.c_float * 3)
    i3 = (C.c_int32 * 3)
    with _span('xr_kilo_mlp_backward', R * S):
        _lib.check(L.xr_kilo_mlp_backward(_ptr(pts), _ptr(rays_o), _ptr(rays_d), _ptr(z_vals), _ptr(_f32c(viewdirs)), R, S,
                                          f3(*[float(v) for v in gmin]), f3(*[float(v) for v in gmax]),
                                          i3(*[int(v) for v in fixed_res]), i3(*[int(v) for v in occ_res]) if occ_res is not None else None,
                                          _ptr(occupancy), _ptr(_f32c(domain_mins)), _ptr(_f32c(domain_maxs)), _ptr(params),
                                          params.stride(0), N, int(pos_freqs), int(dir_freqs), int(n_hidden), _ptr(draw),
                                          _ptr(grad), 1 if reuse else 0, _ptr(ws), ws.numel(), _stream()), 'xr_kilo_mlp_backward')
    return grad


def nerf_render_forward(raw, z_vals, rays_d, white_bkgd):
    """NerfRender.forward (inference): -> rgb [R,3], disp [R], acc [R], weights [R,S]"""
    L = _lib.load()
    raw, z_vals = _f32c(raw), _f32c(z_vals)
    R, S = z_vals.shape
    assert tuple(raw.shape) == (R, S, 4)
    rgb, disp, acc, w = _render_outputs(R, S, raw.device)
    with _span('xr_nerf_render_forward', R * S):
        _lib.check(L.xr_nerf_render_forward(_ptr(raw), _ptr(z_vals), _ptr(_f32c(rays_d)), R, S, int(bool(white_bkgd)),
                                            _ptr(rgb), _ptr(disp), _ptr(acc), _ptr(w), _stream()), 'xr_nerf_render_forward')
    return rgb, disp, acc, w


def kilo_render_rays(rays_o, rays_d, viewdirs, near, far, n_samples, gmin, gmax, fixed_res, occ_res, occupancy, domain_mins,
                     domain_maxs, params, pos_freqs, dir_freqs, n_hidden, white_bkgd=True, lindisp=False):
    """GetZvals(not randomized) + GetPts + KiloNerfMLP.forward + NerfRender.forward in one call (the frame path of the
    real-time bench): -> rgb [R,3], disp [R], acc [R].  near / far: [R] device tensors."""
    L = _lib.load()
    rays_o, rays_d, viewdirs = _f32c(rays_o), _f32c(rays_d), _f32c(viewdirs)
    near, far = _f32c(near.reshape(-1)), _f32c(far.reshape(-1))
    R = rays_o.shape[0]
    dev = rays_o.device
    N = params.shape[0]
    rgb = torch.empty((R, 3), dtype=torch.float32, device=dev)
    disp = torch.empty((R,), dtype=torch.float32, device=dev)
    acc = torch.empty((R,), dtype=torch.float32, device=dev)
    ws = _ws(dev, L.xr_kilo_render_workspace_bytes(R, int(n_samples), N), 'kilo_frame')
    if occupancy is not None:
        occupancy = occupancy.reshape(-1)
        if occupancy.dtype == torch.bool:
            occupancy = occupancy.view(torch.uint8)
    f3 = (C.c_float * 3)
    i3 = (C.c_int32 * 3)
    with _span('xr_kilo_render_rays', R * n_samples):
        _lib.check(L.xr_kilo_render_rays(_ptr(rays_o), _ptr(rays_d), _ptr(viewdirs), _ptr(near), _ptr(far), R, int(n_samples),
                                         int(bool(lindisp)), f3(*[float(v) for v in gmin]), f3(*[float(v) for v in gmax]),
                                         i3(*[int(v) for v in fixed_res]), i3(*[int(v) for v in occ_res]) if occ_res is not None else None,
                                         _ptr(occupancy), _ptr(_f32c(domain_mins)), _ptr(_f32c(domain_maxs)), _ptr(params),
                                         params.stride(0), N, int(pos_freqs), int(dir_freqs), int(n_hidden),
                                         int(bool(white_bkgd)), _ptr(rgb), _ptr(disp), _ptr(acc), _ptr(ws), ws.numel(),
                                         _stream()), 'xr_kilo_render_rays')
    return rgb, disp, acc


# ---------------------------------------------------------------- fp32 MFMA linear layers (8x256 NeRF MLP)
def linear_ok(x, w):
    """shapes / alignment the MFMA kernel takes: fp32 device tensors, K and N multiples of 4"""
    return (_on_device(x) and x.dtype == torch.float32 and w.dtype == torch.float32 and x.dim() == 2
            and x.shape[1] % 4 == 0 and w.shape[0] % 4 == 0 and x.shape[0] > 0)


LINEAR_ARITHMETIC = {None: 0, 'split2': 1, 'bf16x3': 2, 'bf16x3all': 3, 'mfma': 4}      # xr_linear_arithmetic


class linear_arithmetic:
    """context manager: this thread's linear-kernel launches inside it use the given arithmetic whatever XR_GEMM_F32 says
    ('mfma' = the exact-fp32 MFMA kernel for all three products); the previous choice comes back on exit"""

    def __init__(self, kind):
        self.mode = LINEAR_ARITHMETIC[kind]

    def __enter__(self):
        self.prev = _lib.load().xr_linear_arithmetic(self.mode)
        if self.prev < 0:
            _lib.check(self.prev, 'xr_linear_arithmetic')
        return self

    def __exit__(self, *exc):
        _lib.load().xr_linear_arithmetic(self.prev)
        return False


def _rows(t):
    """(tensor as the linear kernels take it, row stride): a [M, C] fp32 matrix whose rows are contiguous and start on 16-byte boundaries --
    dense, or a column range of a wider buffer.  Anything else is copied."""
    if t.dtype != torch.float32:
        raise _lib.XrError('the linear kernels take float32 tensors (got %s)' % t.dtype)
    if not _on_device(t):
        raise _lib.XrError('xrnerf_amd ops need ROCm device tensors (got a %s tensor): there is no CPU fallback' % t.device)
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0:
        return t, t.stride(0)
    t = t.contiguous()
    return t, t.shape[1]


def linear_forward(x, w, bias, relu, out=None):
    """y [M,N] = act(x [M,K] . w [N,K]^T + bias).  x and `out` may be column ranges of wider buffers (row strides)."""
    x, ldx = _rows(x)
    w = _f32c(w)
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device) if out is None else out
    if tuple(y.shape) != (M, N) or y.stride(1) != 1 or y.stride(0) % 4 or y.data_ptr() % 16 or y.dtype != torch.float32:
        raise _lib.XrError('linear_forward: out must be an [M, N] float32 view with contiguous, 16-byte aligned rows')
    with _span('xr_linear_forward', M):
        _lib.check(_lib.load().xr_linear_forward(C.c_void_p(x.data_ptr()), ldx, _ptr(w), _ptr(_f32c(bias)) if bias is not None else None, M, N, K,
                                                 int(bool(relu)), C.c_void_p(y.data_ptr()), y.stride(0), _stream()), 'xr_linear_forward')
    return y


def _dy_and_mask(dy, mask_src):
    dy, ld = _rows(dy)
    if mask_src is not None:
        mask_src, ldm = _rows(mask_src)
        if ldm != ld:                                  # one stride for both in the kernel: bring them to dense rows
            dy, mask_src = dy.contiguous(), mask_src.contiguous()
            ld = dy.shape[1]
    return dy, mask_src, ld


def linear_backward_input(dy, mask_src, w, w_t=None):
    """dx [M,K] = (dy where mask_src > 0) . w.  The weight goes in transposed (one 64 K-element copy, or the caller's `w_t`): both operands
    of the product are then [rows, contraction] like the forward's and it runs on the forward's split-operand kernel instead of the fp32
    MFMA (1.6x).  dy / mask_src may be column ranges of wider buffers (same row stride)."""
    dy, mask_src, ld = _dy_and_mask(dy, mask_src)
    M, N = dy.shape
    K = w.shape[1]
    dx = torch.empty((M, K), dtype=torch.float32, device=dy.device)
    if w_t is None:
        w_t = _f32c(w).t().contiguous()
    with _span('xr_linear_backward_input', M):
        _lib.check(_lib.load().xr_linear_backward_input(C.c_void_p(dy.data_ptr()), ld, C.c_void_p(mask_src.data_ptr()) if mask_src is not None else None,
                                                        _ptr(w_t), 1, M, N, K, _ptr(dx), _stream()), 'xr_linear_backward_input')
    return dx


def sum_partials(part):
    """[splits, n] per-range partial sums -> [n]: one fixed-order launch (xr_sum_partials)"""
    if part.shape[0] == 1:
        return part[0]
    out = torch.empty((part.shape[1],), dtype=torch.float32, device=part.device)
    _lib.check(_lib.load().xr_sum_partials(_ptr(part), part.shape[0], part.stride(0), part.shape[1], _ptr(out), _stream()), 'xr_sum_partials')
    return out


def linear_backward_weight(dy, mask_src, x):
    """dw [N,K] = (dy where mask_src > 0)^T . x   (fixed-order sum of the per-M-range partials)"""
    L = _lib.load()
    dy, mask_src, ld = _dy_and_mask(dy, mask_src)
    x, ldx = _rows(x)
    M, N = dy.shape
    K = x.shape[1]
    splits = int(L.xr_linear_backward_splits(M, N, K))
    part = torch.empty((splits, N, K), dtype=torch.float32, device=dy.device)
    with _span('xr_linear_backward_weight', M):
        _lib.check(L.xr_linear_backward_weight(C.c_void_p(dy.data_ptr()), ld, C.c_void_p(mask_src.data_ptr()) if mask_src is not None else None,
                                               C.c_void_p(x.data_ptr()), ldx, M, N, K, splits, _ptr(part), None, 0, _stream()),
                   'xr_linear_backward_weight')
    return sum_partials(part.view(splits, N * K)).view(N, K)


def linear_backward_weight_bias(dy, mask_src, x):
    """(dw [N,K], db [N]) of one layer from ONE launch and ONE reduction: the bias gradient's column sums ride on the weight-gradient
    product, and both sets of per-M-range partials sit in one [splits, N K + N] buffer"""
    L = _lib.load()
    dy, mask_src, ld = _dy_and_mask(dy, mask_src)
    x, ldx = _rows(x)
    M, N = dy.shape
    K = x.shape[1]
    splits = int(L.xr_linear_backward_splits(M, N, K))
    part = torch.empty((splits, N * K + N), dtype=torch.float32, device=dy.device)
    with _span('xr_linear_backward_weight', M):
        _lib.check(L.xr_linear_backward_weight(C.c_void_p(dy.data_ptr()), ld, C.c_void_p(mask_src.data_ptr()) if mask_src is not None else None,
                                               C.c_void_p(x.data_ptr()), ldx, M, N, K, splits, _ptr(part), C.c_void_p(part.data_ptr() + 4 * N * K),
                                               N * K + N, _stream()), 'xr_linear_backward_weight')
    g = sum_partials(part)
    return g[:N * K].view(N, K), g[N * K:]


def linear_backward_bias(dy, mask_src):
    """db [N] = column sums of (dy where mask_src > 0)   (fixed-order sum of the per-M-range partials)"""
    L = _lib.load()
    dy = _f32c(dy)
    M, N = dy.shape
    splits = int(L.xr_linear_backward_splits(M, 0, 0))
    part = torch.empty((splits, N), dtype=torch.float32, device=dy.device)
    _lib.check(L.xr_linear_backward_bias(_ptr(dy), _ptr(mask_src), M, N, splits, _ptr(part), _stream()), 'xr_linear_backward_bias')
    return sum_partials(part)


# ---------------------------------------------------------------- BungeeNeRF (configs/bungeenerf/bungeenerf_multiscale_google.py)
_BUNGEE_BOUNDS = {None: 0, 'none': 0, 'sphere': 1, 'flat': 2}
EARTH_RADIUS = 6371011.0              # metres, as BungeeGetBounds; buildings are assumed below 250 m


def bungee_zvals(rays_o, viewdirs, near, far, n_z, ray_nearfar='sphere', scene_origin=(0., 0., 0.), scaling=1.0):
    """BungeeGetBounds + BungeeGetZvals in one launch -> (near [R,1], far [R,1], z_vals [R,n_z]).  With ray_nearfar 'sphere' / 'flat'
    near / far are computed (the arguments may be None); with None / 'none' they are inputs."""
    mode = _BUNGEE_BOUNDS[ray_nearfar]
    dev = viewdirs.device if viewdirs is not None else near.device
    R = (viewdirs if mode else near.reshape(-1)).shape[0]
    if mode:
        near = torch.empty((R, 1), dtype=torch.float32, device=dev)
        far = torch.empty((R, 1), dtype=torch.float32, device=dev)
    else:
        near, far = _f32c(near.reshape(R, 1)).clone(), _f32c(far.reshape(R, 1)).clone()
    z = torch.empty((R, n_z), dtype=torch.float32, device=dev)
    s = float(scaling)
    # the reference's float64 scalars, rounded to fp32 where its tensor ops round them
    gc = (C.c_float * 3)(*[float(v) * s for v in scene_origin])
    r2_top = ((EARTH_RADIUS + 250.0) * s) ** 2
    r2_earth = (EARTH_RADIUS * s) ** 2
    with _span('xr_bungee_zvals', R):
        _lib.check(_lib.load().xr_bungee_zvals(_ptr(_f32c(rays_o)) if mode else None, _ptr(_f32c(viewdirs)) if mode else None,
                                               _ptr(near), _ptr(far), R, n_z, mode, C.cast(gc, C.c_void_p), r2_top, r2_earth, s,
                                               _ptr(z), _stream()), 'xr_bungee_zvals')
    return near, far, z


def bungee_encode(viewdirs, multires, multires_dirs, frustum=None, gaussians=None, ray_shape='cone', out=None):
    """cast_rays + BungeeEmbedder.forward -> [M, 3+6 multires + 3+6 multires_dirs] (the reference's data['embedded']): a column range of
    a buffer whose rows are 16-byte aligned, so the MLP's linear kernels read it in place.  frustum = (rays_o, rays_d, radii, z_vals)
    or gaussians = (means, covs) [R, S, 3]: exactly one."""
    if (frustum is None) == (gaussians is None):
        raise _lib.XrError('bungee_encode: give exactly one of frustum and gaussians')
    R = viewdirs.shape[0]
    if frustum is not None:
        o, d, radii, z = frustum
        S = z.shape[1] - 1
        ptrs = (_ptr(_f32c(o)), _ptr(_f32c(d)), _ptr(_f32c(radii.reshape(-1))), _ptr(_f32c(z)), None, None)
    else:
        means, covs = gaussians
        S = means.shape[1]
        ptrs = (None, None, None, None, _ptr(_f32c(means)), _ptr(_f32c(covs)))
    cp, cd = 3 + 6 * multires, 3 + 6 * multires_dirs
    if out is None:
        out = torch.empty((R * S, (cp + cd + 3) // 4 * 4), dtype=torch.float32, device=viewdirs.device)
    if not _on_device(out) or out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[1] < cp + cd:
        raise _lib.XrError('bungee_encode: out must be a float32 device matrix with contiguous rows of >= %d channels' % (cp + cd))
    base = out.data_ptr()
    with _span('xr_bungee_encode', R * S):
        _lib.check(_lib.load().xr_bungee_encode(*ptrs, _ptr(_f32c(viewdirs)), R, S, multires, multires_dirs,
                                                {'cone': 0, 'cylinder': 1}[ray_shape], C.c_void_p(base), out.stride(0),
                                                C.c_void_p(base + 4 * cp), out.stride(0), _stream()), 'xr_bungee_encode')
    return out[:, :cp + cd]


def _bungee_render_common(raw, z_vals, viewdirs, noise):
    R, n_z = z_vals.shape
    raw = _f32c(raw)
    if raw.dim() != 4 or tuple(raw.shape[:2]) != (R, n_z - 1) or raw.shape[3] != 4:
        raise _lib.XrError('raw must be [R, n_z-1, heads, 4]')
    return raw, _f32c(z_vals), _f32c(viewdirs), _render_noise(noise, R, n_z - 1), R, n_z, raw.shape[2]


def bungee_render_forward(raw, z_vals, viewdirs, stage, density_bias=-1.0, rgb_padding=0.0, white_bkgd=False,
                          density_activation='softplus', noise=None):
    """BungeeNerfRender.forward: raw [R,S,H,4] -> rgb [R,3], disp [R], acc [R], weights [R,S]"""
    raw, z_vals, viewdirs, noise, R, n_z, H = _bungee_render_common(raw, z_vals, viewdirs, noise)
    rgb, disp, acc, w = _render_outputs(R, n_z - 1, raw.device)
    with _span('xr_bungee_render_forward', R * (n_z - 1)):
        _lib.check(_lib.load().xr_bungee_render_forward(_ptr(raw), _ptr(z_vals), _ptr(viewdirs), _ptr(noise), R, n_z, H, int(stage),
                                                        float(density_bias), float(rgb_padding), int(bool(white_bkgd)),
                                                        _MIP_ACT[density_activation], _ptr(rgb), _ptr(disp), _ptr(acc), _ptr(w),
                                                        _stream()), 'xr_bungee_render_forward')
    return rgb, disp, acc, w


def bungee_render_backward(raw, z_vals, viewdirs, grad_rgb, stage, density_bias=-1.0, rgb_padding=0.0, white_bkgd=False,
                           density_activation='softplus', noise=None):
    """dL/draw [R,S,H,4] given dL/drgb: equal for heads <= stage, zeros above"""
    raw, z_vals, viewdirs, noise, R, n_z, H = _bungee_render_common(raw, z_vals, viewdirs, noise)
    out = torch.empty_like(raw)
    with _span('xr_bungee_render_backward', R * (n_z - 1)):
        _lib.check(_lib.load().xr_bungee_render_backward(_ptr(raw), _ptr(z_vals), _ptr(viewdirs), _ptr(noise), _ptr(_f32c(grad_rgb)), R,
                                                         n_z, H, int(stage), float(density_bias), float(rgb_padding),
                                                         int(bool(white_bkgd)), _MIP_ACT[density_activation], _ptr(out), _stream()),
                   'xr_bungee_render_backward')
    return out


# ---------------------------------------------------------------- vanilla NeRF (configs/nerf/nerf_blender_base01.py)
def vanilla_kernels_available():
    """the loaded library handle has xr_vanilla.hip's entry points.  libxrnerf_mi355.so always has (load() fails otherwise); a handle
    made of the host builds of other sources (tests/hip_emu) may not, and the modules of vanilla.py then keep their tensor-op path"""
    return hasattr(_lib.load(), 'xr_nerf_encode')


def nerf_encode_channels(multires, multires_dirs):
    return 6 + 6 * int(multires) + 6 * int(multires_dirs)


def nerf_encode(pts, viewdirs, multires, multires_dirs, out=None):
    """BaseEmbedder.forward in one launch: pts [..., 3] (n_rows points), viewdirs [n_dirs, 3] with n_rows a multiple of n_dirs (row r
    takes direction r // (n_rows / n_dirs)) -> [n_rows, channels]: a column range of a buffer whose rows are padded to a multiple of
    4 floats (padding written as zeros), which the linear kernels read in place"""
    pts, viewdirs = _f32c(pts).reshape(-1, 3), _f32c(viewdirs).reshape(-1, 3)
    n, nd = pts.shape[0], viewdirs.shape[0]
    if n and (nd == 0 or n % nd):
        raise _lib.XrError('nerf_encode: %d points cannot share %d directions evenly' % (n, nd))
    ch = nerf_encode_channels(multires, multires_dirs)
    if out is None:
        out = torch.empty((n, (ch + 3) // 4 * 4), dtype=torch.float32, device=pts.device)
    if (not _on_device(out) or out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] != n
            or out.stride(0) < (ch + 3) // 4 * 4):
        raise _lib.XrError('nerf_encode: out must be a float32 device matrix of %d rows with a row stride of >= %d floats' % (n, (ch + 3) // 4 * 4))
    _ptr(viewdirs)                                                     # (host tensors are refused here)
    with _span('xr_nerf_encode', n):
        _lib.check(_lib.load().xr_nerf_encode(_ptr(pts), _ptr(viewdirs), n, n // nd if n else 1, int(multires), int(multires_dirs),
                                              C.c_void_p(out.data_ptr()), out.stride(0), _stream()), 'xr_nerf_encode')
    return out[:, :ch]


def _nerf_render_common(raw, z_vals, rays_d, noise):
    raw, z_vals, rays_d = _f32c(raw), _f32c(z_vals), _f32c(rays_d)
    R, S = z_vals.shape
    if tuple(raw.shape) != (R, S, 4) or tuple(rays_d.shape) != (R, 3):
        raise _lib.XrError('the NeRF renderer takes raw [R, S, 4], z_vals [R, S] and rays_d [R, 3]')
    return raw, z_vals, rays_d, _render_noise(noise, R, S), R, S


def nerf_render_train_forward(raw, z_vals, rays_d, white_bkgd, noise=None):
    """NerfRender.forward (relu density, no padding, no bias) with the optional density noise: -> rgb [R,3], disp [R], acc [R], weights [R,S]"""
    raw, z_vals, rays_d, noise, R, S = _nerf_render_common(raw, z_vals, rays_d, noise)
    rgb, disp, acc, w = _render_outputs(R, S, raw.device)
    with _span('xr_nerf_render_train_forward', R * S):
        _lib.check(_lib.load().xr_nerf_render_train_forward(_ptr(raw), _ptr(z_vals), _ptr(rays_d), _ptr(noise), R, S, int(bool(white_bkgd)),
                                                            _ptr(rgb), _ptr(disp), _ptr(acc), _ptr(w), _stream()),
                   'xr_nerf_render_train_forward')
    return rgb, disp, acc, w


def nerf_render_backward(raw, z_vals, rays_d, grad_rgb, white_bkgd, noise=None):
    """dL/draw [R,S,4] given dL/drgb [R,3] (recomputed from the forward's inputs)"""
    raw, z_vals, rays_d, noise, R, S = _nerf_render_common(raw, z_vals, rays_d, noise)
    grad_rgb = _f32c(grad_rgb)
    if tuple(grad_rgb.shape) != (R, 3):
        raise _lib.XrError('grad_rgb must be [R, 3]')
    out = torch.empty_like(raw)
    with _span('xr_nerf_render_backward', R * S):
        _lib.check(_lib.load().xr_nerf_render_backward(_ptr(raw), _ptr(z_vals), _ptr(rays_d), _ptr(noise), R, S, int(bool(white_bkgd)),
                                                       _ptr(grad_rgb), _ptr(out), _stream()), 'xr_nerf_render_backward')
    return out


def nerf_sample_pdf(z_vals, weights, rays_o, rays_d, n_new, u=None, want_samples=False):
    """sample_pdf + the merge with the coarse samples + GetPts in one launch: -> (z_all [R, S+n_new], pts [R, S+n_new, 3]) and, with
    want_samples, the new samples [R, n_new] before the merge.  u [R, n_new]: the uniform draws; None = linspace(0, 1, n_new)."""
    z_vals, weights = _f32c(z_vals), _f32c(weights.detach())
    rays_o, rays_d = _f32c(rays_o), _f32c(rays_d)
    R, S = z_vals.shape
    N = int(n_new)
    if tuple(weights.shape) != (R, S) or tuple(rays_o.shape) != (R, 3) or tuple(rays_d.shape) != (R, 3):
        raise _lib.XrError('nerf_sample_pdf takes z_vals / weights [R, S] and rays_o / rays_d [R, 3]')
    if u is not None:
        u = _f32c(u)
        if tuple(u.shape) != (R, N):
            raise _lib.XrError('u must be [R, n_new]')
    dev = z_vals.device
    z_all = torch.empty((R, S + max(N, 0)), dtype=torch.float32, device=dev)
    pts = torch.empty((R, S + max(N, 0), 3), dtype=torch.float32, device=dev)
    zs = torch.empty((R, max(N, 0)), dtype=torch.float32, device=dev) if want_samples else None
    with _span('xr_nerf_sample_pdf', R):
        _lib.check(_lib.load().xr_nerf_sample_pdf(_ptr(z_vals), _ptr(weights), _ptr(u), _ptr(rays_o), _ptr(rays_d), R, S, max(N, 0),
                                                  _ptr(z_all), _ptr(pts), _ptr(zs), _stream()), 'xr_nerf_sample_pdf')
    return (z_all, pts, zs) if want_samples else (z_all, pts)


# ---------------------------------------------------------------- Animatable NeRF (configs/animatable_nerf/an_h36m_s9_train_pose.py)
ANI_JOINTS = 24                 # XR_ANI_JOINTS
ANI_CLOSEST_TILE = 1024         # XR_ANI_CLOSEST_TILE: vertices staged in LDS at a time


def aninerf_kernels_available():
    """the loaded library handle has xr_aninerf.hip's entry points.  libxrnerf_mi355.so always has (load() fails otherwise); a handle
    made of the host builds of other sources (tests/hip_emu) may not, and the modules of aninerf.py then keep their tensor-op path"""
    return hasattr(_lib.load(), 'xr_ani_closest')


def _i32c(t):
    if t.dtype != torch.int32:
        raise _lib.XrError('expected an int32 tensor (got %s)' % t.dtype)
    return t if t.is_contiguous() else t.contiguous()


def ani_closest(pts, verts, th, R=None, T=None, want_d2=False):
    """nearest vertex of every point (knn_points with K = 1), after the optional world -> pose transform (p - T) R of points AND vertices:
    pts [N,3], verts [V,3] -> (q [N,3] the transformed points, idx [N] int32, dist [N], flag [N] int32 = dist < th) and, with want_d2,
    the squared distances [N]"""
    pts, verts = _f32c(pts).reshape(-1, 3), _f32c(verts).reshape(-1, 3)
    if (R is None) != (T is None):
        raise _lib.XrError('ani_closest: R and T come together')
    if R is not None:
        R, T = _f32c(R).reshape(3, 3), _f32c(T).reshape(3)
    N, V = pts.shape[0], verts.shape[0]
    dev = pts.device
    q = torch.empty((N, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((N,), dtype=torch.int32, device=dev)
    dist = torch.empty((N,), dtype=torch.float32, device=dev)
    flag = torch.empty((N,), dtype=torch.int32, device=dev)
    d2 = torch.empty((N,), dtype=torch.float32, device=dev) if want_d2 else None
    _ptr(verts)                                                        # (host tensors are refused here, N = 0 included)
    with _span('xr_ani_closest', N):
        _lib.check(_lib.load().xr_ani_closest(_ptr(pts), _ptr(verts), _ptr(R), _ptr(T), N, V, float(th), _ptr(q), _ptr(idx), _ptr(d2),
                                              _ptr(dist), _ptr(flag), _stream()), 'xr_ani_closest')
    return (q, idx, dist, flag, d2) if want_d2 else (q, idx, dist, flag)


def ani_select(flag, dist):
    """pind = flag; pind[argmin(dist)] = True; -> (list [N] int32 whose first `count` entries are nonzero(pind) in ascending order,
    count [1] int32), both on the device: the caller reads the count once"""
    flag, dist = _i32c(flag).reshape(-1), _f32c(dist).reshape(-1)
    N = flag.shape[0]
    if dist.shape[0] != N:
        raise _lib.XrError('ani_select: flag and dist differ in length')
    dev = flag.device
    lst = torch.empty((N,), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    nbytes = int(lib.xr_ani_select_workspace_bytes(N))
    ws = _ws(dev, nbytes, 'ani_select')
    _ptr(dist)
    with _span('xr_ani_select', N):
        _lib.check(lib.xr_ani_select(_ptr(flag), _ptr(dist), N, _ptr(lst), _ptr(count), C.c_void_p(ws.data_ptr()), ws.numel(), _stream()),
                   'xr_ani_select')
    return lst, count


def _bw_rows(t, what):
    t = _f32c(t)
    if t.dim() != 2 or t.shape[1] != ANI_JOINTS:
        raise _lib.XrError('%s must be [N, %d]' % (what, ANI_JOINTS))
    return t


def ani_blend_forward(smpl_bw, idx, logits):
    """softmax_j(log(smpl_bw[idx, j] + 1e-9) + logits[:, j]) -> [N,24]"""
    smpl_bw, logits, idx = _bw_rows(smpl_bw, 'smpl_bw'), _bw_rows(logits, 'logits'), _i32c(idx).reshape(-1)
    N = logits.shape[0]
    if idx.shape[0] != N:
        raise _lib.XrError('ani_blend_forward: idx and logits differ in length')
    out = torch.empty_like(logits)
    _ptr(smpl_bw)
    with _span('xr_ani_blend_forward', N):
        _lib.check(_lib.load().xr_ani_blend_forward(_ptr(smpl_bw), _ptr(idx), _ptr(logits), N, _ptr(out), _stream()), 'xr_ani_blend_forward')
    return out


def ani_blend_backward(bw, grad_bw):
    """dL/dlogits [N,24] from the head's output and dL/dbw"""
    bw, grad_bw = _bw_rows(bw, 'bw'), _bw_rows(grad_bw, 'grad_bw')
    if grad_bw.shape != bw.shape:
        raise _lib.XrError('ani_blend_backward: bw and grad_bw differ in shape')
    out = torch.empty_like(bw)
    _ptr(grad_bw)
    with _span('xr_ani_blend_backward', bw.shape[0]):
        _lib.check(_lib.load().xr_ani_blend_backward(_ptr(bw), _ptr(grad_bw), bw.shape[0], _ptr(out), _stream()), 'xr_ani_blend_backward')
    return out


def _skin_common(pts, dirs, bw, a_from, a_to):
    pts, bw = _f32c(pts).reshape(-1, 3), _bw_rows(bw, 'bw')
    a_from, a_to = _f32c(a_from).reshape(-1, 16), _f32c(a_to).reshape(-1, 16)
    N = pts.shape[0]
    if bw.shape[0] != N or a_from.shape[0] != ANI_JOINTS or a_to.shape[0] != ANI_JOINTS:
        raise _lib.XrError('skinning takes pts [N,3], bw [N,24] and two sets of 24 4x4 matrices')
    if dirs is not None:
        dirs = _f32c(dirs).reshape(-1, 3)
        if dirs.shape[0] != N:
            raise _lib.XrError('dirs must be [N,3]')
    return pts, dirs, bw, a_from, a_to, N


def ani_skin_forward(pts, dirs, bw, a_from, a_to):
    """p'' = B_R A_R^-1 (p - A_t) + B_t and d'' = B_R A_R^-1 d with A = sum_j bw_j a_from[j], B = sum_j bw_j a_to[j]
    -> (pts_out [N,3], dirs_out [N,3] or None)"""
    pts, dirs, bw, a_from, a_to, N = _skin_common(pts, dirs, bw, a_from, a_to)
    po = torch.empty_like(pts)
    do = torch.empty_like(dirs) if dirs is not None else None
    _ptr(a_from)
    with _span('xr_ani_skin_forward', N):
        _lib.check(_lib.load().xr_ani_skin_forward(_ptr(pts), _ptr(dirs), _ptr(bw), _ptr(a_from), _ptr(a_to), N, _ptr(po), _ptr(do), _stream()),
                   'xr_ani_skin_forward')
    return po, do


def ani_skin_backward(pts, dirs, bw, a_from, a_to, grad_pts, grad_dirs=None):
    """dL/dbw [N,24] from dL/dp'' and dL/dd'' (either may be None), recomputed from the forward's inputs"""
    pts, dirs, bw, a_from, a_to, N = _skin_common(pts, dirs, bw, a_from, a_to)
    if grad_pts is not None:
        grad_pts = _f32c(grad_pts).reshape(-1, 3)
    if grad_dirs is not None:
        grad_dirs = _f32c(grad_dirs).reshape(-1, 3)
    for g in (grad_pts, grad_dirs):
        if g is not None and g.shape[0] != N:
            raise _lib.XrError('the skinning gradients must be [N,3]')
    if grad_dirs is not None and dirs is None:
        raise _lib.XrError('grad_dirs given without dirs')
    out = torch.empty_like(bw)
    _ptr(a_from)
    with _span('xr_ani_skin_backward', N):
        _lib.check(_lib.load().xr_ani_skin_backward(_ptr(pts), _ptr(dirs), _ptr(bw), _ptr(a_from), _ptr(a_to), N, _ptr(grad_pts),
                                                    _ptr(grad_dirs), _ptr(out), _stream()), 'xr_ani_skin_backward')
    return out


def ani_encode_backward(pts, grad, multires):
    """input gradient of BaseEmbedder's point encoding: pts [N,3], grad [N, >= 3 + 6 multires] (a column range of a wider matrix is
    read in place, at its row stride) -> dL/dpts [N,3]"""
    pts = _f32c(pts).reshape(-1, 3)
    N, cp = pts.shape[0], 3 + 6 * int(multires)
    if grad.dtype != torch.float32 or grad.dim() != 2 or grad.shape[0] != N or grad.shape[1] < cp:
        raise _lib.XrError('ani_encode_backward: grad must be float32 [N, >= %d]' % cp)
    if N and (grad.stride(1) != 1 or grad.stride(0) < cp):
        grad = grad.contiguous()
    if not _on_device(grad):
        _ptr(grad)
    out = torch.empty_like(pts)
    _ptr(pts)
    with _span('xr_ani_encode_backward', N):
        _lib.check(_lib.load().xr_ani_encode_backward(_ptr(pts), C.c_void_p(grad.data_ptr()), grad.stride(0) if N else cp, N, int(multires),
                                                      _ptr(out), _stream()), 'xr_ani_encode_backward')
    return out


# ---------------------------------------------------------------- NeuralBody (configs/neuralbody/nb_zjumocap_*.py)
NB_LEVELS = 5                   # XR_NB_LEVELS
NB_TAPS = 27                    # XR_NB_TAPS
NB_MAX_CELLS = 1 << 26          # XR_NB_MAX_CELLS
NB_FEATURES = 352               # XR_NB_FEATURES
NB_LEVEL_CHANNELS = (32, 64, 128, 128)


def neuralbody_kernels_available():
    """the loaded library handle has xr_neuralbody.hip's entry points (a handle made of the host builds of other sources may not:
    the modules of neuralbody.py then keep their tensor-op path)"""
    return hasattr(_lib.load(), 'xr_nb_conv')


def _nb_dims(out_sh):
    D, H, W = (int(v) for v in out_sh)
    return D, H, W


def nb_layout(V, out_sh):
    """-> (volume offsets [5], row-list offsets [5], total volume ints, total list ints) of xr_nb_build_rows' two buffers"""
    D, H, W = _nb_dims(out_sh)
    out = (C.c_uint64 * 12)()
    _lib.check(_lib.load().xr_nb_layout(int(V), D, H, W, C.cast(out, C.c_void_p)), 'xr_nb_layout')
    return [int(v) for v in out[0:5]], [int(v) for v in out[5:10]], int(out[10]), int(out[11])


def nb_build_rows(coord, out_sh):
    """the five levels of a frame from the voxel coordinates coord [V,3] int32 (z, y, x) in the volume out_sh = (D, H, W):
    -> (vols: five int32 index volumes [cells_l] (row of each cell, -1 where empty), rows: five int32 lists of active cells in
    ascending linear index, vert_row [V] int32, counts: five ints).  ONE read of the counts from the device."""
    coord = _i32c(coord).reshape(-1, 3)
    V = coord.shape[0]
    D, H, W = _nb_dims(out_sh)
    lib = _lib.load()
    vo, ro, nv, nr = nb_layout(V, out_sh)
    dev = coord.device
    vol = torch.empty((nv,), dtype=torch.int32, device=dev)
    rows = torch.empty((max(nr, 1),), dtype=torch.int32, device=dev)
    vert_row = torch.empty((V,), dtype=torch.int32, device=dev)
    counts = torch.zeros((NB_LEVELS,), dtype=torch.int32, device=dev)
    ws = _ws(dev, int(lib.xr_nb_build_rows_workspace_bytes(D, H, W)), 'nb_rows')
    _ptr(coord)
    with _span('xr_nb_build_rows', V):
        _lib.check(lib.xr_nb_build_rows(_ptr(coord), V, D, H, W, _ptr(vol), _ptr(rows), _ptr(vert_row), _ptr(counts),
                                        C.c_void_p(ws.data_ptr()), ws.numel(), _stream()), 'xr_nb_build_rows')
    n = [int(v) for v in counts.tolist()]
    ends = vo[1:] + [nv]
    return [vol[vo[l]:ends[l]] for l in range(NB_LEVELS)], [rows[ro[l]:ro[l] + n[l]] for l in range(NB_LEVELS)], vert_row, n


def nb_subm_table(vol, rows, dims):
    """[n,27] int32: the row of cell p + k - 1 for every row p of a level with dims (D, H, W), -1 where empty or outside"""
    D, H, W = _nb_dims(dims)
    n = rows.shape[0]
    nbr = torch.empty((n, NB_TAPS), dtype=torch.int32, device=rows.device)
    _ptr(vol)
    with _span('xr_nb_subm_table', n):
        _lib.check(_lib.load().xr_nb_subm_table(_ptr(vol), _ptr(_i32c(rows)), n, D, H, W, _ptr(nbr), _stream()), 'xr_nb_subm_table')
    return nbr


def nb_down_tables(vol_in, rows_in, vol_out, rows_out, dims_in):
    """the strided step's tables: (out_tab [n_out,27] input row at 2 o - 1 + k, in_tab [n_in,27] output row whose tap k reads input i)"""
    D, H, W = _nb_dims(dims_in)
    n_in, n_out = rows_in.shape[0], rows_out.shape[0]
    dev = rows_in.device
    out_tab = torch.empty((n_out, NB_TAPS), dtype=torch.int32, device=dev)
    in_tab = torch.empty((n_in, NB_TAPS), dtype=torch.int32, device=dev)
    _ptr(vol_in)
    with _span('xr_nb_down_tables', n_in):
        _lib.check(_lib.load().xr_nb_down_tables(_ptr(vol_in), _ptr(_i32c(rows_in)), n_in, _ptr(vol_out), _ptr(_i32c(rows_out)), n_out,
                                                 D, H, W, _ptr(out_tab), _ptr(in_tab), _stream()), 'xr_nb_down_tables')
    return out_tab, in_tab


def _nb_weight(w):
    w = _f32c(w)
    if w.dim() == 5 and tuple(w.shape[1:4]) == (3, 3, 3):
        w = w.reshape(w.shape[0], NB_TAPS, w.shape[4])
    if w.dim() != 3 or w.shape[1] != NB_TAPS:
        raise _lib.XrError('a sparse-convolution weight is [Cout, 3, 3, 3, Cin]')
    return w


def nb_conv(x, tab, w, transposed=False, flip=False):
    """out [n, c_out] = sum_k x[tab[:, k']] Wk with rows of tab = -1 reading as 0; w [Cout, 3, 3, 3, Cin].  transposed: the input
    gradient (x = dL/dout [*, Cout], out [n, Cin]); flip: k' = 26 - k (the submanifold input gradient on the forward table)"""
    x, w, tab = _f32c(x), _nb_weight(w), _i32c(tab)
    n = tab.shape[0]
    cin, cout = (w.shape[0], w.shape[2]) if transposed else (w.shape[2], w.shape[0])
    if x.dim() != 2 or x.shape[1] != cin or tab.dim() != 2 or tab.shape[1] != NB_TAPS:
        raise _lib.XrError('nb_conv: x must be [*, %d] and tab [n, 27]' % cin)
    out = torch.empty((n, cout), dtype=torch.float32, device=x.device)
    _ptr(w)
    with _span('xr_nb_conv', n):
        _lib.check(_lib.load().xr_nb_conv(_ptr(x), _ptr(tab), _ptr(w), n, cin, cout, int(bool(transposed)), int(bool(flip)), _ptr(out),
                                          _stream()), 'xr_nb_conv')
    return out


def nb_conv_weight_grad(x, tab, g):
    """dW [Cout, 3, 3, 3, Cin] = sum_r g[r]^T x[tab[r, k]] per tap (tab: the forward table of the n rows of g)"""
    x, g, tab = _f32c(x), _f32c(g), _i32c(tab)
    n, cin, cout = tab.shape[0], x.shape[1], g.shape[1]
    if g.shape[0] != n or tab.shape[1] != NB_TAPS:
        raise _lib.XrError('nb_conv_weight_grad: g must be [n, Cout] for tab [n, 27]')
    dw = torch.zeros((cout, 3, 3, 3, cin), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    ws = _ws(x.device, int(lib.xr_nb_conv_weight_grad_workspace_bytes(n, cin, cout)), 'nb_wgrad')
    _ptr(g)
    with _span('xr_nb_conv_weight_grad', n):
        _lib.check(lib.xr_nb_conv_weight_grad(_ptr(x), _ptr(tab), _ptr(g), n, cin, cout, _ptr(dw), C.c_void_p(ws.data_ptr()), ws.numel(),
                                              _stream()), 'xr_nb_conv_weight_grad')
    return dw


def _nb_ptr4(ts):
    arr = (C.c_void_p * 4)()
    for l, t in enumerate(ts):
        arr[l] = t.data_ptr() if (t is not None and t.numel()) else None
    return arr


def _nb_sample_common(pts, R, T, min_xyz, vols, feats_or_counts):
    pts = _f32c(pts).reshape(-1, 3)
    R, T, min_xyz = _f32c(R).reshape(9), _f32c(T).reshape(3), _f32c(min_xyz).reshape(3)
    if len(vols) != 4 or len(feats_or_counts) != 4:
        raise _lib.XrError('sampling takes the four levels after conv1..conv4')
    for t in (pts, R, T, min_xyz) + tuple(vols):
        _ptr(t)
    return pts, R, T, min_xyz, [_i32c(v) for v in vols]


def nb_sample_forward(pts, R, T, min_xyz, voxel, out_sh, vols, feats, out=None):
    """grid_sample (zeros padding, align_corners) of the four levels' sparse rows at the world points pts [N,3], through the levels'
    index volumes: -> [N, 352], or written into the first 352 columns of `out` [N, >= 352] (a row stride that is a multiple of 4)"""
    pts, R, T, min_xyz, vols = _nb_sample_common(pts, R, T, min_xyz, vols, feats)
    feats = [_f32c(f) for f in feats]
    for f, c in zip(feats, NB_LEVEL_CHANNELS):
        if f.dim() != 2 or f.shape[1] != c:
            raise _lib.XrError('the sampled levels have 32, 64, 128 and 128 channels')
    N = pts.shape[0]
    D, H, W = _nb_dims(out_sh)
    if out is None:
        out = torch.empty((N, NB_FEATURES), dtype=torch.float32, device=pts.device)
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != N or out.shape[1] < NB_FEATURES or (N and out.stride(1) != 1):
        raise _lib.XrError('nb_sample_forward: out must be float32 [N, >= 352] with unit column stride')
    if not _on_device(out):
        _ptr(out)
    with _span('xr_nb_sample_forward', N):
        _lib.check(_lib.load().xr_nb_sample_forward(_ptr(pts), _ptr(R), _ptr(T), _ptr(min_xyz), float(voxel), D, H, W,
                                                    C.cast(_nb_ptr4(vols), C.c_void_p), C.cast(_nb_ptr4(feats), C.c_void_p), N,
                                                    C.c_void_p(out.data_ptr()), out.stride(0) if N else NB_FEATURES, _stream()),
                   'xr_nb_sample_forward')
    return out


def nb_sample_backward(pts, R, T, min_xyz, voxel, out_sh, vols, n_rows, grad):
    """the gradient of the four levels' rows from grad [N, >= 352] (read in place at its row stride): four tensors [n_rows[l], C_l]"""
    pts, R, T, min_xyz, vols = _nb_sample_common(pts, R, T, min_xyz, vols, n_rows)
    N = pts.shape[0]
    D, H, W = _nb_dims(out_sh)
    if grad.dtype != torch.float32 or grad.dim() != 2 or grad.shape[0] != N or grad.shape[1] < NB_FEATURES:
        raise _lib.XrError('nb_sample_backward: grad must be float32 [N, >= 352]')
    if N and (grad.stride(1) != 1 or grad.stride(0) % 4 or grad.data_ptr() % 16):
        grad = grad.contiguous()
    if not _on_device(grad):
        _ptr(grad)
    dev = pts.device
    outs = [torch.empty((int(n), c), dtype=torch.float32, device=dev) for n, c in zip(n_rows, NB_LEVEL_CHANNELS)]
    counts = (C.c_uint32 * 4)(*[int(n) for n in n_rows])
    lib = _lib.load()
    ws = _ws(dev, int(lib.xr_nb_sample_backward_workspace_bytes(C.cast(counts, C.c_void_p))), 'nb_sample_bwd')
    with _span('xr_nb_sample_backward', N):
        _lib.check(lib.xr_nb_sample_backward(_ptr(pts), _ptr(R), _ptr(T), _ptr(min_xyz), float(voxel), D, H, W,
                                             C.cast(_nb_ptr4(vols), C.c_void_p), C.cast(counts, C.c_void_p), C.c_void_p(grad.data_ptr()),
                                             grad.stride(0) if N else NB_FEATURES, N, C.cast(_nb_ptr4(outs), C.c_void_p),
                                             C.c_void_p(ws.data_ptr()), ws.numel(), _stream()), 'xr_nb_sample_backward')
    return outs


# ---------------------------------------------------------------- GNR body-shape queries (configs/gnr/gnr_genebody.py)
GNR_MAX_CELLS = 1 << 28         # XR_GNR_MAX_CELLS
GNR_EMBED_COLS = 10             # XR_GNR_EMBED_COLS


def gnr_kernels_available():
    """the loaded library handle has xr_gnr.hip's entry points (a handle made of the host builds of other sources may not: gnr.py then
    keeps its host path)"""
    return hasattr(_lib.load(), 'xr_gnr_nearest')


def _gnr_grid_args(verts, faces, step, min3, num3):
    """the seven leading arguments of the grid entry points; min3 / num3 are HOST values (kept alive by the returned tuple)"""
    verts, faces = _f32c(verts).reshape(-1, 3), _i32c(faces).reshape(-1, 3)
    mn = (C.c_float * 3)(*[float(v) for v in min3])
    nm = (C.c_int32 * 3)(*[int(v) for v in num3[:3]])
    return (_ptr(verts), _ptr(faces), verts.shape[0], faces.shape[0], float(step), C.cast(mn, C.c_void_p), C.cast(nm, C.c_void_p)), (verts, faces, mn, nm)


def gnr_grid_build(verts, faces, step, min3, num3):
    """-> (tri_num [cells] int32 inclusive prefix counts, tri_idx [total] int32 face id + 1, bad) with ONE blocking read (the slot total
    and the face-index flag together); bad: some face names a vertex outside [0, V)"""
    dev = verts.device
    cells = int(num3[0]) * int(num3[1]) * int(num3[2])
    args, keep = _gnr_grid_args(verts, faces, step, min3, num3)
    lib = _lib.load()
    tri_num = torch.empty((cells,), dtype=torch.int32, device=dev)
    status = torch.empty((2,), dtype=torch.int32, device=dev)
    with _span('xr_gnr_grid_count', args[3]):
        _lib.check(lib.xr_gnr_grid_count(*args, _ptr(tri_num), _ptr(status), _stream()), 'xr_gnr_grid_count')
    tri_num = torch.cumsum(tri_num, 0, dtype=torch.int32)
    status[0:1] = tri_num[-1:]
    total, bad = status.tolist()
    tri_idx = torch.empty((total,), dtype=torch.int32, device=dev)
    if total > 0 and not bad:
        cursor = _ws(dev, cells * 4, 'gnr_cursor')
        with _span('xr_gnr_grid_fill', args[3]):
            _lib.check(lib.xr_gnr_grid_fill(*args, _ptr(tri_num), total, _ptr(tri_idx), C.c_void_p(cursor.data_ptr()), _stream()),
                       'xr_gnr_grid_fill')
    return tri_num, tri_idx, bool(bad)


def gnr_nearest(verts, faces, step, min3, num3, tri_num, tri_idx, pts):
    """-> (near_faces [N] int32, near_pts [N,3], coeff [N,3])"""
    pts = _f32c(pts).reshape(-1, 3)
    N, dev = pts.shape[0], pts.device
    args, keep = _gnr_grid_args(verts, faces, step, min3, num3)
    near_faces = torch.empty((N,), dtype=torch.int32, device=dev)
    near_pts = torch.empty((N, 3), dtype=torch.float32, device=dev)
    coeff = torch.empty((N, 3), dtype=torch.float32, device=dev)
    with _span('xr_gnr_nearest', N):
        _lib.check(_lib.load().xr_gnr_nearest(*args, _ptr(_i32c(tri_num)), _ptr(_i32c(tri_idx)), tri_idx.numel(), _ptr(pts), N,
                                              _ptr(near_faces), _ptr(near_pts), _ptr(coeff), _stream()), 'xr_gnr_nearest')
    return near_faces, near_pts, coeff


def gnr_inside(verts, faces, step, min3, num3, tri_num, tri_idx, pts):
    """-> signs [N] float32 (+1 inside, -1 outside)"""
    pts = _f32c(pts).reshape(-1, 3)
    N = pts.shape[0]
    args, keep = _gnr_grid_args(verts, faces, step, min3, num3)
    signs = torch.empty((N,), dtype=torch.float32, device=pts.device)
    with _span('xr_gnr_inside', N):
        _lib.check(_lib.load().xr_gnr_inside(*args, _ptr(_i32c(tri_num)), _ptr(_i32c(tri_idx)), tri_idx.numel(), _ptr(pts), N, _ptr(signs),
                                             _stream()), 'xr_gnr_inside')
    return signs


def gnr_shape_embed(pts, near_faces, near_pts, signs, faces, t_verts, center3, rot9, scale, half, use_nml, use_t_pose, use_smpl_sdf):
    """the embedding half of make_nerf_input -> (out [N, 3 + 3 use_t_pose + 4 use_smpl_sdf], alpha_smpl [N] or None); center3 [3] / rot9 [3,3]
    are device tensors"""
    pts = _f32c(pts).reshape(-1, 3)
    N, dev = pts.shape[0], pts.device
    cols = 3 + (3 if use_t_pose else 0) + (4 if use_smpl_sdf else 0)
    out = torch.empty((N, cols), dtype=torch.float32, device=dev)
    alpha = torch.empty((N,), dtype=torch.float32, device=dev) if use_smpl_sdf else None
    c3 = _f32c(center3).reshape(3) if center3 is not None else None
    r9 = _f32c(rot9).reshape(9) if rot9 is not None else None
    F = V = 0
    if use_t_pose:
        faces, t_verts, near_faces = _i32c(faces).reshape(-1, 3), _f32c(t_verts).reshape(-1, 3), _i32c(near_faces)
        F, V = faces.shape[0], t_verts.shape[0]
    if use_smpl_sdf:
        near_pts, signs = _f32c(near_pts).reshape(-1, 3), _f32c(signs)
    with _span('xr_gnr_shape_embed', N):
        _lib.check(_lib.load().xr_gnr_shape_embed(
            _ptr(pts), N, _ptr(near_faces) if use_t_pose else None, _ptr(near_pts) if use_smpl_sdf else None,
            _ptr(signs) if use_smpl_sdf else None, _ptr(faces) if use_t_pose else None, F, _ptr(t_verts) if use_t_pose else None, V,
            _ptr(c3), _ptr(r9), float(scale), float(half),
            int(bool(use_nml)), int(bool(use_t_pose)), int(bool(use_smpl_sdf)), _ptr(out), cols, _ptr(alpha), _stream()), 'xr_gnr_shape_embed')
    return out, alpha


# ---------------------------------------------------------------- GNR renderer stages (csrc/xr_gnr_render.hip)
GNR_MAX_VIEWS = 8               # XR_GNR_MAX_VIEWS


def gnr_render_kernels_available():
    """the loaded library handle has xr_gnr_render.hip's entry points (see gnr_kernels_available)"""
    return hasattr(_lib.load(), 'xr_gnr_hull_count')


def gnr_hull(rays, t_vals, w2c, cams, masks, width, height, depth=None, cam_c=None, rot=None):
    """visual hull and compaction -> dict: M, table [R,2] int32 (count, base), idx [M] int32, pts [M,3], xy [M,V,2], z [M,V],
    vis [M,V] bool or None (with depth), attdirs [M,V+1,3] or None (with cam_c).  ONE blocking read (M).  masks / depth [V,H,W]."""
    rays, t_vals = _f32c(rays).reshape(-1, 6), _f32c(t_vals)
    R, dev = rays.shape[0], rays.device
    S = t_vals.shape[-1]
    w2c, cams = _f32c(w2c).reshape(-1, 4, 4), _f32c(cams)
    V, cam_cols = w2c.shape[0], cams.shape[-1]
    masks = _f32c(masks).reshape(V, masks.shape[-2], masks.shape[-1])
    H, W = masks.shape[-2:]
    if depth is not None:
        depth = _f32c(depth).reshape(V, H, W)
    lib = _lib.load()
    table = torch.empty((R, 2), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int32, device=dev)
    rank = _ws(dev, max(R * S, 1) * 4, 'gnr_hull_rank')
    head = (_ptr(rays), _ptr(t_vals), R, S, _ptr(w2c), _ptr(cams), cam_cols, V, _ptr(masks))
    with _span('xr_gnr_hull_count', R * S):
        _lib.check(lib.xr_gnr_hull_count(*head, H, W, float(width), float(height), C.c_void_p(rank.data_ptr()), _ptr(table), _ptr(total),
                                         _stream()), 'xr_gnr_hull_count')
    M = int(total.item())
    out = {'M': M, 'table': table,
           'idx': torch.empty((M,), dtype=torch.int32, device=dev), 'pts': torch.empty((M, 3), dtype=torch.float32, device=dev),
           'xy': torch.empty((M, V, 2), dtype=torch.float32, device=dev), 'z': torch.empty((M, V), dtype=torch.float32, device=dev),
           'vis': None, 'attdirs': None}
    vis = torch.empty((M, V), dtype=torch.uint8, device=dev) if depth is not None else None
    if cam_c is not None:
        cam_c = _f32c(cam_c).reshape(V, 3)
        out['attdirs'] = torch.empty((M, V + 1, 3), dtype=torch.float32, device=dev)
    r9 = _f32c(rot).reshape(9) if rot is not None else None
    if M > 0:
        with _span('xr_gnr_hull_write', R * S):
            _lib.check(lib.xr_gnr_hull_write(*head, _ptr(depth), H, W, float(width), float(height), _ptr(cam_c), _ptr(r9),
                                             C.c_void_p(rank.data_ptr()), _ptr(table), M, _ptr(out['pts']), _ptr(out['idx']), _ptr(out['xy']),
                                             _ptr(out['z']), _ptr(vis), _ptr(out['attdirs']), _stream()), 'xr_gnr_hull_write')
    if vis is not None:
        out['vis'] = vis.bool()
    return out


def gnr_gather(xy, feats_last, images, out=None, col0=0, images_channel_last=False):
    """pixel-aligned gather: xy [M,V,2], feats_last [V,h,w,C] (channel-last), images [V,3,H,W] (or [V,H,W,3]) ->
    (out [M,V,ld], source_rgb [M,V,3]); `out` (its last stride is the row stride ld) receives columns col0 .. col0 + C + 3 and zeros
    behind them; without `out` a fresh [M, V, C + 3 rounded up to 4] buffer is made"""
    xy = _f32c(xy)
    M, V = xy.shape[0], xy.shape[1]
    feats_last, images = _f32c(feats_last), _f32c(images)
    fh, fw, Cf = feats_last.shape[1:]
    ih, iw = (images.shape[1], images.shape[2]) if images_channel_last else (images.shape[2], images.shape[3])
    if out is None:
        out = torch.empty((M, V, (col0 + Cf + 3 + 3) // 4 * 4), dtype=torch.float32, device=xy.device)
    if not out.is_contiguous() or out.dtype != torch.float32 or out.shape[:2] != (M, V):
        raise ValueError('out must be a contiguous float32 [M, V, ld]')
    source_rgb = torch.empty((M, V, 3), dtype=torch.float32, device=xy.device)
    with _span('xr_gnr_gather', M * V):
        _lib.check(_lib.load().xr_gnr_gather(_ptr(xy), M, V, _ptr(feats_last), fh, fw, Cf, _ptr(images), ih, iw, int(bool(images_channel_last)),
                                             _ptr(out), out.shape[2], int(col0), _ptr(source_rgb), _stream()), 'xr_gnr_gather')
    return out, source_rgb


def gnr_gather_backward(xy, grad, col0, feats_shape):
    """the gather's gradient in the channel-last feature maps: xy [M,V,2], grad [M,V,ld] (columns col0 .. col0 + C are read),
    feats_shape = (V, h, w, C) -> d_feats [V,h,w,C]"""
    xy, grad = _f32c(xy), _f32c(grad)
    M, V = xy.shape[0], xy.shape[1]
    Vf, fh, fw, Cf = feats_shape
    if Vf != V or grad.shape[:2] != (M, V):
        raise ValueError('shapes of xy %r, grad %r and the feature maps %r disagree' % (tuple(xy.shape), tuple(grad.shape), tuple(feats_shape)))
    lib = _lib.load()
    d_feats = torch.empty((V, fh, fw, Cf), dtype=torch.float32, device=xy.device)
    nbytes = int(lib.xr_gnr_gather_backward_workspace_bytes(V, fh, fw, Cf))
    ws = _ws(xy.device, nbytes, 'gnr_gather_bwd')
    with _span('xr_gnr_gather_backward', M * V):
        _lib.check(lib.xr_gnr_gather_backward(_ptr(xy), M, V, _ptr(grad), grad.shape[2], int(col0), fh, fw, Cf, _ptr(d_feats),
                                              C.c_void_p(ws.data_ptr()), ws.numel(), _stream()), 'xr_gnr_gather_backward')
    return d_feats


def _gnr_comp_head(net, source_rgb, idx, table, t_vals, noise):
    if net.dim() != 2 or net.stride(1) != 1 or net.dtype != torch.float32:
        raise ValueError('net must be float32 [M, ld] with unit column stride')
    if net.shape[0] > 1 and net.stride(0) < net.shape[1]:
        raise ValueError('net rows overlap')
    source_rgb, idx, table, t_vals = _f32c(source_rgb), _i32c(idx), _i32c(table), _f32c(t_vals)
    noise = _f32c(noise) if noise is not None else None
    R, S = t_vals.shape
    M, V = net.shape[0], source_rgb.shape[1] if source_rgb.dim() == 3 else 0
    if net.shape[1] < 4 + V + 1 or idx.shape[0] != M or source_rgb.shape[0] != M or table.shape != (R, 2):
        raise ValueError('shapes of net %r, source_rgb %r, idx %r, table %r disagree' % (tuple(net.shape), tuple(source_rgb.shape),
                                                                                         tuple(idx.shape), tuple(table.shape)))
    ld = net.stride(0) if M > 1 else max(net.shape[1], 4 + V + 1)
    keep = (net, source_rgb, idx, table, t_vals, noise)
    return (C.c_void_p(net.data_ptr()) if M else None, ld, _ptr(source_rgb) if M else None, _ptr(idx) if M else None, _ptr(table),
            _ptr(t_vals), _ptr(noise), R, S, V, M), keep


def gnr_composite_forward(net, source_rgb, idx, table, t_vals, noise=None, z_near_far=None, white=False):
    """-> (rgb_map [R,6], depth [R], acc [R], weights [R,S], trans [M])"""
    head, keep = _gnr_comp_head(net, source_rgb, idx, table, t_vals, noise)
    R, S, M = head[7], head[8], head[10]
    dev = keep[4].device
    rgb_map = torch.empty((R, 6), dtype=torch.float32, device=dev)
    depth, acc = torch.empty((R,), dtype=torch.float32, device=dev), torch.empty((R,), dtype=torch.float32, device=dev)
    weights = torch.empty((R, S), dtype=torch.float32, device=dev)
    trans = torch.empty((M,), dtype=torch.float32, device=dev)
    zn, zf = (float(z_near_far[0]), float(z_near_far[1])) if z_near_far is not None else (0.0, 0.0)
    with _span('xr_gnr_composite_forward', R):
        _lib.check(_lib.load().xr_gnr_composite_forward(*head, int(z_near_far is not None), zn, zf, int(bool(white)), _ptr(rgb_map), _ptr(depth),
                                                        _ptr(acc), _ptr(weights), _ptr(trans), _stream()), 'xr_gnr_composite_forward')
    return rgb_map, depth, acc, weights, trans


def gnr_composite_backward(net, source_rgb, idx, table, t_vals, noise, white, d_rgb_map, trans):
    """-> d_net [M, 4 + V + 1]"""
    head, keep = _gnr_comp_head(net, source_rgb, idx, table, t_vals, noise)
    R, V, M = head[7], head[9], head[10]
    d_rgb_map, trans = _f32c(d_rgb_map).reshape(R, 6), _f32c(trans)
    d_net = torch.empty((M, 4 + V + 1), dtype=torch.float32, device=keep[4].device)
    with _span('xr_gnr_composite_backward', R):
        _lib.check(_lib.load().xr_gnr_composite_backward(*head, int(bool(white)), _ptr(d_rgb_map), _ptr(trans), _ptr(d_net), _stream()),
                                                         'xr_gnr_composite_backward')
    return d_net


# ---------------------------------------------------------------- GNR image encoder (csrc/xr_gnr_encoder.hip)
def gnr_encoder_kernels_available():
    """the loaded library handle has xr_gnr_encoder.hip's entry points (see gnr_kernels_available)"""
    return hasattr(_lib.load(), 'xr_hg_conv2d')


def _hg_map(t, what):
    """a channel-last map [N,H,W,C], or a column slice of one (`buf[..., a:b]`) -> (pointer of its channel 0, row stride)"""
    if not _on_device(t):
        raise _lib.XrError('xrnerf_amd ops need ROCm device tensors (got a %s tensor): there is no CPU fallback' % t.device)
    if t.dim() != 4 or t.dtype != torch.float32:
        raise ValueError('%s must be a float32 [N, H, W, C] map' % what)
    N, H, W, Cc = t.shape
    ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if N > 1 else Cc))
    if (Cc > 1 and t.stride(3) != 1) or ld < Cc or (W > 1 and H > 1 and t.stride(1) != W * ld) or (N > 1 and t.stride(0) != H * W * ld):
        raise ValueError('%s must be a channel-last map or a column slice of one (strides %r)' % (what, t.stride()))
    return C.c_void_p(t.data_ptr()), int(ld)


def hg_relay_weight(w):
    """nn.Conv2d.weight [Cout, Cin, k, k] -> the kernel's [k k Cin, Cout] (once per load, not per call)"""
    return w.detach().permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous().float()


def hg_conv2d(x, w_kc, ksize, stride=1, norm=None, bias=None, relu=False, out=None, accumulate=False):
    """x [N,H,W,Cin] (map or column slice), w_kc = hg_relay_weight(weight); norm = (mean [N,G], rstd [N,G], gamma [Cin], beta [Cin]):
    relu(group_norm(x)) is what the convolution reads, zero padding after it; -> out [N,Ho,Wo,Cout] (map or column slice; with
    `accumulate` the result is added to what it holds)"""
    xp, ldx = _hg_map(x, 'x')
    N, H, W, Cin = x.shape
    Cout = w_kc.shape[1]
    if w_kc.shape[0] != ksize * ksize * Cin:
        raise ValueError('weight %r does not fit k = %d, Cin = %d' % (tuple(w_kc.shape), ksize, Cin))
    pad = ksize // 2
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    if out is None:
        if accumulate:
            raise ValueError('accumulate needs an output to add to')
        out = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (N, Ho, Wo, Cout):
        raise ValueError('out must be [%d, %d, %d, %d], got %r' % (N, Ho, Wo, Cout, tuple(out.shape)))
    yp, ldy = _hg_map(out, 'out')
    mean = rstd = gamma = beta = None
    groups = 0
    if norm is not None:
        mean, rstd, gamma, beta = norm
        groups = mean.shape[1]
    with _span('xr_hg_conv2d', N * Ho * Wo):
        _lib.check(_lib.load().xr_hg_conv2d(xp, ldx, N, H, W, Cin, _ptr(w_kc), Cout, int(ksize), int(stride), _ptr(mean), _ptr(rstd), _ptr(gamma),
                                            _ptr(beta), groups, _ptr(bias), int(bool(relu)), int(bool(accumulate)), yp, ldy, _stream()), 'xr_hg_conv2d')
    return out


def hg_gn_stats(x, groups=32, eps=1e-5):
    """x [N,H,W,C] (map or column slice) -> (mean, rstd) [N, groups] of GroupNorm(groups, C): biased variance, fixed summation order"""
    xp, ldx = _hg_map(x, 'x')
    N, H, W, Cc = x.shape
    lib = _lib.load()
    mean = torch.empty((N, groups), dtype=torch.float32, device=x.device)
    rstd = torch.empty((N, groups), dtype=torch.float32, device=x.device)
    ws = _ws(x.device, int(lib.xr_hg_gn_stats_workspace_bytes(N, H * W, groups)) + 16, 'hg_gn_stats')
    off = (-ws.data_ptr()) % 16
    with _span('xr_hg_gn_stats', N * H * W):
        _lib.check(lib.xr_hg_gn_stats(xp, ldx, N, H * W, Cc, groups, float(eps), _ptr(mean), _ptr(rstd), C.c_void_p(ws.data_ptr() + off),
                                      ws.numel() - off, _stream()), 'xr_hg_gn_stats')
    return mean, rstd


def hg_gn_relu(x, mean, rstd, gamma, beta, out=None):
    """relu(group_norm(x)) from hg_gn_stats' statistics; out=x works in place"""
    xp, ldx = _hg_map(x, 'x')
    N, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((N, H, W, Cc), dtype=torch.float32, device=x.device)
    yp, ldy = _hg_map(out, 'out')
    if out.shape != x.shape:
        raise ValueError('out must have the shape of x')
    with _span('xr_hg_gn_relu', N * H * W):
        _lib.check(_lib.load().xr_hg_gn_relu(xp, ldx, N, H * W, Cc, mean.shape[1], _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), yp, ldy,
                                             _stream()), 'xr_hg_gn_relu')
    return out


def hg_avgpool2(x, out=None):
    """F.avg_pool2d(., 2, stride=2) on a channel-last map"""
    xp, ldx = _hg_map(x, 'x')
    N, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((N, H // 2, W // 2, Cc), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (N, H // 2, W // 2, Cc):
        raise ValueError('out must be [N, H / 2, W / 2, C]')
    yp, ldy = _hg_map(out, 'out')
    with _span('xr_hg_avgpool2', N * H * W):
        _lib.check(_lib.load().xr_hg_avgpool2(xp, ldx, N, H, W, Cc, yp, ldy, _stream()), 'xr_hg_avgpool2')
    return out


def hg_bicubic_up2(x, addend=None, out=None):
    """F.interpolate(., scale_factor=2, mode='bicubic', align_corners=True) on a channel-last map (+ addend; out=addend works in place)"""
    xp, ldx = _hg_map(x, 'x')
    N, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((N, 2 * H, 2 * W, Cc), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (N, 2 * H, 2 * W, Cc) or (addend is not None and addend.shape != out.shape):
        raise ValueError('out and addend must be [N, 2 H, 2 W, C]')
    yp, ldy = _hg_map(out, 'out')
    ap, lda = _hg_map(addend, 'addend') if addend is not None else (None, 0)
    with _span('xr_hg_bicubic_up2', N * H * W * 4):
        _lib.check(_lib.load().xr_hg_bicubic_up2(xp, ldx, N, H, W, Cc, ap, lda, yp, ldy, _stream()), 'xr_hg_bicubic_up2')
    return out


def hg_add(x, out):
    """out += x on channel-last maps (or column slices) of one shape"""
    xp, ldx = _hg_map(x, 'x')
    yp, ldy = _hg_map(out, 'out')
    if out.shape != x.shape:
        raise ValueError('out must have the shape of x')
    N, H, W, Cc = x.shape
    with _span('xr_hg_add', N * H * W):
        _lib.check(_lib.load().xr_hg_add(xp, ldx, N * H * W, Cc, yp, ldy, _stream()), 'xr_hg_add')
    return out


def hg_conv_block(x, weights, norms, out=None, groups=32, eps=1e-5):
    """one ConvBlock in one call: x [N,H,W,Cin]; weights = (w1, w2, w3, w_down or None), re-laid (hg_relay_weight); norms = the gamma and
    beta of bn1, bn2, bn3 and bn4 (eight tensors; bn4's are read with w_down only) -> out [N,H,W,Cout] = cat(out1, out2, out3) + residual"""
    xp, ldx = _hg_map(x, 'x')
    N, H, W, Cin = x.shape
    w1, w2, w3, wd = weights
    Cout = 2 * w1.shape[1]
    if out is None:
        out = torch.empty((N, H, W, Cout), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (N, H, W, Cout):
        raise ValueError('out must be [%d, %d, %d, %d], got %r' % (N, H, W, Cout, tuple(out.shape)))
    if w1.shape[0] != 9 * Cin or tuple(w2.shape) != (9 * (Cout // 2), Cout // 4) or tuple(w3.shape) != (9 * (Cout // 4), Cout // 4) or \
            (wd is not None and tuple(wd.shape) != (Cin, Cout)):
        raise ValueError('the weights do not fit a ConvBlock(%d, %d)' % (Cin, Cout))
    yp, ldy = _hg_map(out, 'out')
    lib = _lib.load()
    ws = _ws(x.device, int(lib.xr_hg_conv_block_workspace_bytes(N, H * W, groups)) + 16, 'hg_conv_block')
    off = (-ws.data_ptr()) % 16
    with _span('xr_hg_conv_block', N * H * W):
        _lib.check(lib.xr_hg_conv_block(xp, ldx, N, H, W, Cin, Cout, _ptr(w1), _ptr(w2), _ptr(w3), _ptr(wd), *[_ptr(t) for t in norms], groups, float(eps),
                                        yp, ldy, C.c_void_p(ws.data_ptr() + off), ws.numel() - off, _stream()), 'xr_hg_conv_block')
    return out


# ---------------------------------------------------------------- GNR mesh reconstruction (csrc/xr_gnr_recon.hip)
GNR_RECON_MAX_N = 1024          # XR_GNR_RECON_MAX_N


def gnr_recon_kernels_available():
    """the loaded library handle has xr_gnr_recon.hip's entry points (see gnr_kernels_available)"""
    return hasattr(_lib.load(), 'xr_gnr_recon_hull')


def gnr_recon_grid(N, bb_min, bb_max, spatial_freq, center, coords=None):
    """the grid's description for the entry points below: np.linspace(bb_min[a], bb_max[a], N) per axis as (start, stop, step) host
    doubles, spatial_freq, center [3] (device fp32); or `coords` [N^3,3] (device fp32), the caller's own points"""
    lin = (C.c_double * 9)()
    for a in range(3):
        lin[3 * a], lin[3 * a + 1] = float(bb_min[a]), float(bb_max[a])
        lin[3 * a + 2] = (float(bb_max[a]) - float(bb_min[a])) / (N - 1)
    if coords is not None:
        coords = _f32c(coords).reshape(-1, 3)
        if coords.shape[0] != N ** 3:
            raise _lib.XrError('gnr_recon_grid: coords must hold N^3 points')
    return {'N': int(N), 'lin': lin, 'sf': float(spatial_freq), 'center': _f32c(center).reshape(3), 'coords': coords}


def _gc_grid_args(grid):
    return (grid['lin'], grid['sf'], _ptr(grid['center']), _ptr(grid['coords']))


def _gc_views(w2c, cams):
    w2c, cams = _f32c(w2c).reshape(-1, 4, 4), _f32c(cams)
    return w2c, cams, (_ptr(w2c), _ptr(cams), cams.shape[-1], w2c.shape[0])


def gnr_recon_hull(grid, w2c, cams, masks, width, height):
    """-> state [N,N,N] uint8 (1 = inside the hull and below the last index of every axis)"""
    N, dev = grid['N'], grid['center'].device
    w2c, cams, views = _gc_views(w2c, cams)
    masks = _f32c(masks).reshape(w2c.shape[0], masks.shape[-2], masks.shape[-1])
    state = torch.empty((N, N, N), dtype=torch.uint8, device=dev)
    with _span('xr_gnr_recon_hull', N ** 3):
        _lib.check(_lib.load().xr_gnr_recon_hull(N, *_gc_grid_args(grid), *views, _ptr(masks), masks.shape[-2], masks.shape[-1], float(width),
                                                 float(height), _ptr(state), _stream()), 'xr_gnr_recon_hull')
    return state


def gnr_recon_select(grid, reso, state, w2c, cams, width, height):
    """the level's test set in C order -> (flat [M] int32, pts [M,3], xy [M,V,2]).  ONE blocking read (M)."""
    N, dev = grid['N'], state.device
    lib = _lib.load()
    w2c, cams, views = _gc_views(w2c, cams)
    nbytes = int(lib.xr_gnr_recon_select_workspace_bytes(N, int(reso)))
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int32, device=dev)
    with _span('xr_gnr_recon_select_count', N ** 3 // reso ** 3):
        _lib.check(lib.xr_gnr_recon_select_count(N, int(reso), _ptr(state), _ptr(ws), ws.numel() * 4, _ptr(total), _stream()), 'xr_gnr_recon_select_count')
    M = int(total.item())
    if M < 0:
        raise _lib.XrError('gnr_recon_select: more than 2^31 - 1 points')
    V = w2c.shape[0]
    flat = torch.empty((M,), dtype=torch.int32, device=dev)
    pts = torch.empty((M, 3), dtype=torch.float32, device=dev)
    xy = torch.empty((M, V, 2), dtype=torch.float32, device=dev)
    if M > 0:
        with _span('xr_gnr_recon_select_write', N ** 3 // reso ** 3):
            _lib.check(lib.xr_gnr_recon_select_write(N, int(reso), *_gc_grid_args(grid), *views, float(width), float(height), _ptr(state), _ptr(ws), M,
                                                     _ptr(flat), _ptr(pts), _ptr(xy), _stream()), 'xr_gnr_recon_select_write')
    return flat, pts, xy


def gnr_recon_scatter(flat, values, volume, state, gamma=None):
    """volume[flat] = values (sigmoid(gamma values) with a gamma), state[flat] = 0, in place"""
    M, N = flat.shape[0], volume.shape[0]
    values = _f32c(values).reshape(-1)
    if values.shape[0] != M:
        raise _lib.XrError('gnr_recon_scatter: one value per selected point')
    with _span('xr_gnr_recon_scatter', M):
        _lib.check(_lib.load().xr_gnr_recon_scatter(_ptr(_i32c(flat)), _ptr(values), M, int(gamma is not None), float(gamma or 0.0), N, _ptr(volume),
                                                    _ptr(state), _stream()), 'xr_gnr_recon_scatter')


def gnr_recon_fold(reso, volume, state):
    """the skip-and-fill step after a level with reso >= 2, in place"""
    N = volume.shape[0]
    lib = _lib.load()
    nbytes = int(lib.xr_gnr_recon_fold_workspace_bytes(N, int(reso)))
    ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.int32, device=volume.device)
    with _span('xr_gnr_recon_fold', N ** 3):
        _lib.check(lib.xr_gnr_recon_fold(N, int(reso), _ptr(volume), _ptr(state), _ptr(ws), ws.numel() * 4, _stream()), 'xr_gnr_recon_fold')


def gnr_recon_surface(volume, level):
    """iso-surface with welded vertices -> (verts_idx [Nv,3] fp32, faces [T,3] int32, normals [Nv,3] fp32).  ONE blocking read (Nv, T)."""
    volume = _f32c(volume)
    N, dev = volume.shape[0], volume.device
    lib = _lib.load()
    nbytes = int(lib.xr_gnr_recon_surface_workspace_bytes(N))
    ws = torch.empty((nbytes // 4,), dtype=torch.int32, device=dev)
    totals = torch.empty((2,), dtype=torch.int32, device=dev)
    with _span('xr_gnr_recon_surface_count', N ** 3):
        _lib.check(lib.xr_gnr_recon_surface_count(_ptr(volume), N, float(level), _ptr(ws), ws.numel() * 4, _ptr(totals), _stream()), 'xr_gnr_recon_surface_count')
    Nv, T = (int(v) for v in totals.tolist())
    if Nv < 0 or T < 0:
        raise _lib.XrError('gnr_recon_surface: more than 2^31 - 1 vertices or triangles')
    verts = torch.empty((Nv, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((Nv, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((T, 3), dtype=torch.int32, device=dev)
    if Nv > 0:
        with _span('xr_gnr_recon_surface_write', N ** 3):
            _lib.check(lib.xr_gnr_recon_surface_write(_ptr(volume), N, float(level), _ptr(ws), Nv, T, _ptr(verts), _ptr(normals), _ptr(faces), _stream()),
                       'xr_gnr_recon_surface_write')
    return verts, faces, normals


def gnr_recon_world(verts_idx, N, extent, spatial_freq, center):
    """index coordinates -> (verts [Nv,3] float64 in the reference's world coordinates, pts = their fp32 rounding)"""
    verts_idx = _f32c(verts_idx).reshape(-1, 3)
    Nv, dev = verts_idx.shape[0], verts_idx.device
    verts = torch.empty((Nv, 3), dtype=torch.float64, device=dev)
    pts = torch.empty((Nv, 3), dtype=torch.float32, device=dev)
    ext = (C.c_double * 3)(*[float(e) for e in extent])
    center = _f32c(center).reshape(3)
    with _span('xr_gnr_recon_world', Nv):
        _lib.check(_lib.load().xr_gnr_recon_world(_ptr(verts_idx), Nv, int(N), ext, float(spatial_freq), _ptr(center), _ptr(verts), _ptr(pts), _stream()),
                   'xr_gnr_recon_world')
    return verts, pts


def gnr_recon_point_rows(pts, dirs, w2c, cams, width, height, cam_c, rot=None):
    """-> (xy [n,V,2], attdirs [n,V+1,3]) of the points with the query directions `dirs`"""
    pts, dirs = _f32c(pts).reshape(-1, 3), _f32c(dirs).reshape(-1, 3)
    n, dev = pts.shape[0], pts.device
    w2c, cams, views = _gc_views(w2c, cams)
    V = w2c.shape[0]
    cam_c = _f32c(cam_c).reshape(V, 3)
    r9 = _f32c(rot).reshape(9) if rot is not None else None
    xy = torch.empty((n, V, 2), dtype=torch.float32, device=dev)
    attdirs = torch.empty((n, V + 1, 3), dtype=torch.float32, device=dev)
    with _span('xr_gnr_recon_point_rows', n):
        _lib.check(_lib.load().xr_gnr_recon_point_rows(_ptr(pts), _ptr(dirs), n, *views, float(width), float(height), _ptr(cam_c), _ptr(r9), _ptr(xy),
                                                       _ptr(attdirs), _stream()), 'xr_gnr_recon_point_rows')
    return xy, attdirs


def gnr_recon_smooth(verts, faces, rowptr, cols, iterations, lamb=0.5):
    """Laplacian filter with the volume constraint on float64 vertices -> a new [Nv,3] tensor"""
    if verts.dtype != torch.float64:
        raise _lib.XrError('gnr_recon_smooth takes float64 vertices')
    out = verts.contiguous().clone()
    Nv, T = out.shape[0], faces.shape[0]
    lib = _lib.load()
    nbytes = int(lib.xr_gnr_recon_smooth_workspace_bytes(Nv, T))
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=out.device)
    with _span('xr_gnr_recon_smooth', Nv * max(int(iterations), 0)):
        _lib.check(lib.xr_gnr_recon_smooth(_ptr(out), Nv, _ptr(_i32c(faces)), T, _ptr(_i32c(rowptr)), _ptr(_i32c(cols)), cols.shape[0], int(iterations),
                                           float(lamb), _ptr(ws), ws.numel() * 8, _stream()), 'xr_gnr_recon_smooth')
    return out


# ---------------------------------------------------------------- GNR body depth maps (csrc/xr_gnr_raster.hip)
GNR_RASTER_MAX_SIDE = 32768     # XR_GNR_RASTER_MAX_SIDE


def gnr_raster_kernels_available():
    """the loaded library handle has xr_gnr_raster.hip's entry points (see gnr_kernels_available)"""
    return hasattr(_lib.load(), 'xr_gnr_raster_forward')


def gnr_raster_workspace_bytes(V, N, H, W):
    """bytes of workspace one gnr_raster_forward call needs; 0 for sizes it refuses"""
    if min(V, N, H, W) < 0 or max(V, N, H, W) > 0xffffffff:
        return 0
    return int(_lib.load().xr_gnr_raster_workspace_bytes(int(V), int(N), int(H), int(W)))


def gnr_raster_forward(verts, faces, H, W, persp, double_face=False, eps=1e-6, out=None):
    """the z-buffer rasteriser over V views of one mesh: verts [V,N,3] fp32 as the reference's render_forward takes them (x and y
    are divided by z in the kernel with `persp`), faces [F,3] int32 -> (index [V,H,W] int64, -1 where empty; coeff [V,H,W,3];
    visual [V,N] bool; depth [V,H,W], 0 where empty).  `out`: the four tensors to write into (contiguous; slices of larger buffers
    along the first axis are)."""
    verts, faces = _f32c(verts), _i32c(faces)
    if verts.dim() != 3 or verts.shape[-1] != 3 or faces.dim() != 2 or faces.shape[-1] != 3:
        raise _lib.XrError('gnr_raster_forward: verts [V,N,3], faces [F,3]')
    V, N, F = verts.shape[0], verts.shape[1], faces.shape[0]
    H, W = int(H), int(W)
    lib = _lib.load()
    nbytes = gnr_raster_workspace_bytes(V, N, H, W) if min(H, W) >= 0 and F <= 0xffffffff else 0
    if nbytes == 0 or not float(eps) >= 0.0:
        raise _lib.XrError('gnr_raster_forward: refused (eps >= 0; 1 <= H, W <= %d; V H W and V N within int32; F < 2^32 - 1): V %d N %d F %d H %d W %d eps %r'
                           % (GNR_RASTER_MAX_SIDE, V, N, F, H, W, eps))
    dev = verts.device
    shapes = ((V, H, W), (V, H, W, 3), (V, N), (V, H, W))
    dtypes = (torch.int64, torch.float32, torch.bool, torch.float32)
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in zip(shapes, dtypes))
    if len(out) != 4 or any(tuple(t.shape) != s or t.dtype != d for t, s, d in zip(out, shapes, dtypes)):
        raise _lib.XrError('gnr_raster_forward: out = (index int64 [V,H,W], coeff fp32 [V,H,W,3], visual bool [V,N], depth fp32 [V,H,W])')
    ws = _ws(dev, nbytes + 8, 'gnr_raster')
    off = (-ws.data_ptr()) % 8
    with _span('xr_gnr_raster_forward', V * F):
        _lib.check(lib.xr_gnr_raster_forward(_ptr(verts), V, N, _ptr(faces), F, H, W, int(bool(persp)), int(bool(double_face)), float(eps),
                                             *[_ptr(t) for t in out], C.c_void_p(ws.data_ptr() + off), ws.numel() - off, _stream()),
                   'xr_gnr_raster_forward')
    return tuple(out)


# ---------------------------------------------------------------- test-set evaluation (csrc/xr_eval.hip)
EVAL_MAX_RADIUS = 5             # XR_EVAL_MAX_RADIUS
EVAL_MAX_CHANNELS = 4           # XR_EVAL_MAX_CHANNELS


def eval_kernels_available():
    """the loaded library handle has xr_eval.hip's entry points (see gnr_kernels_available)"""
    return hasattr(_lib.load(), 'xr_eval_ssim')


def eval_workspace_bytes(B, H, W, C):
    """bytes of workspace one eval_ssim call needs; 0 for sizes it refuses"""
    if min(B, H, W, C) < 0 or max(B, H, W, C) > 0xffffffff:
        return 0
    return int(_lib.load().xr_eval_workspace_bytes(int(B), int(H), int(W), int(C)))


def _eval_raw(t, what):
    """the data pointer of a strided fp32 device tensor (the eval entry points take element strides, so no copy is made)"""
    if not _on_device(t):
        raise _lib.XrError('%s: xrnerf_amd ops need ROCm device tensors (got a %s tensor): there is no CPU fallback' % (what, t.device))
    if t.dtype != torch.float32:
        raise _lib.XrError('%s: fp32 images (got %s)' % (what, t.dtype))
    return C.c_void_p(t.data_ptr())


def eval_ssim(x, y, taps, cov_norm, C1, C2, want_map=False):
    """x, y [B,H,W,C] fp32 device tensors of any (shared) strides -> (ssim_sum [B] double: the sum of the SSIM map S of every image,
    sq_sum [B] double: the sum of (x - y)^2 with the difference rounded to fp32, map [B,H,W,C] double or None).  taps: the 2 r + 1
    weights of the separable window (host floats); the arithmetic is xrnerf_mi355_eval.h's.  Nothing is read back."""
    if x.dim() != 4 or x.shape != y.shape:
        raise _lib.XrError('eval_ssim: x and y [B,H,W,C] of one shape (got %r, %r)' % (tuple(x.shape), tuple(y.shape)))
    px, py = _eval_raw(x, 'eval_ssim'), _eval_raw(y, 'eval_ssim')
    if x.stride() != y.stride():
        x, y = x.contiguous(), y.contiguous()
        px, py = _eval_raw(x, 'eval_ssim'), _eval_raw(y, 'eval_ssim')
    B, H, W, Cn = (int(v) for v in x.shape)
    taps = [float(t) for t in taps]
    r = (len(taps) - 1) // 2
    if len(taps) != 2 * r + 1 or r > EVAL_MAX_RADIUS:
        raise _lib.XrError('eval_ssim: an odd number of taps, at most %d (got %d)' % (2 * EVAL_MAX_RADIUS + 1, len(taps)))
    nbytes = eval_workspace_bytes(B, H, W, Cn)
    if nbytes == 0 or min(H, W) < 2 * r + 1:
        raise _lib.XrError('eval_ssim: refused (B >= 1; H, W >= 2 r + 1; 1 <= C <= %d; B H W C within int32): B %d H %d W %d C %d r %d'
                           % (EVAL_MAX_CHANNELS, B, H, W, Cn, r))
    dev = x.device
    sums = torch.empty((2, B), dtype=torch.float64, device=dev)
    smap = torch.empty((B, H, W, Cn), dtype=torch.float64, device=dev) if want_map else None
    ws = _ws(dev, nbytes + 8, 'eval')
    off = (-ws.data_ptr()) % 8
    sb, sr, sp, sc = (int(s) for s in x.stride())
    with _span('xr_eval_ssim', B * H * W * Cn, train=False):
        _lib.check(_lib.load().xr_eval_ssim(px, py, B, H, W, Cn, sb, sr, sp, sc, (C.c_double * len(taps))(*taps), r, float(cov_norm), float(C1), float(C2),
                                            _ptr(sums[0]), _ptr(sums[1]), _ptr(smap), C.c_void_p(ws.data_ptr() + off), ws.numel() - off, _stream()),
                   'xr_eval_ssim')
    return sums[0], sums[1], smap


def eval_to8b_pair(rgb, gt=None):
    """rgb (and gt) [H,W,C] fp32 device tensors -> uint8 [H, 2 W, C] = to8b(hstack(rgb, gt)), or [H,W,C] = to8b(rgb) without gt
    (to8b: the fp32 product 255 clip(v, 0, 1), truncated; NaN -> 0)"""
    if rgb.dim() != 3 or (gt is not None and gt.shape != rgb.shape):
        raise _lib.XrError('eval_to8b_pair: rgb (and gt) [H,W,C] of one shape')
    p = _eval_raw(rgb, 'eval_to8b_pair')
    q = None if gt is None else _eval_raw(gt, 'eval_to8b_pair')
    if gt is not None and gt.stride() != rgb.stride():
        rgb, gt = rgb.contiguous(), gt.contiguous()
        p, q = _eval_raw(rgb, 'eval_to8b_pair'), _eval_raw(gt, 'eval_to8b_pair')
    H, W, Cn = (int(v) for v in rgb.shape)
    if min(H, W) < 1 or not 1 <= Cn <= EVAL_MAX_CHANNELS or 2 * H * W * Cn > 0x7fffffff:
        raise _lib.XrError('eval_to8b_pair: refused (H, W >= 1; 1 <= C <= %d; 2 H W C within int32): H %d W %d C %d' % (EVAL_MAX_CHANNELS, H, W, Cn))
    out = torch.empty((H, W if gt is None else 2 * W, Cn), dtype=torch.uint8, device=rgb.device)
    sr, sp, sc = (int(s) for s in rgb.stride())
    with _span('xr_eval_to8b_pair', out.numel(), train=False):
        _lib.check(_lib.load().xr_eval_to8b_pair(p, q, H, W, Cn, sr, sp, sc, _ptr(out), _stream()), 'xr_eval_to8b_pair')
    return out


# ---------------------------------------------------------------- scene data pipelines (csrc/xr_pipeline.hip)
PIPE_MAX_CHANNELS = 4           # XR_PIPE_MAX_CHANNELS
PIPE_OUTPUTS = ('rays_o', 'rays_d', 'viewdirs', 'radii', 'near', 'far', 'z_vals', 'pts', 'target_s')


def pipeline_kernels_available():
    """the loaded library handle has xr_pipeline.hip's entry points (see gnr_kernels_available)"""
    return hasattr(_lib.load(), 'xr_pipe_ray_front')


def pipe_ndc_factors(H, W, focal):
    """the two factors of ndc_rays (transforms.py:37-43), evaluated in double as the reference's Python does"""
    return -1. / (W / (2. * focal)), -1. / (H / (2. * focal))


def pipe_ray_front(H, W, fx, fy, cx, cy, c2w=None, sel=None, pix0=0, R=None, image=None, table=None, with_viewdirs=False, ndc=False,
                   with_radii=False, near=0., far=1., S=0, lindisp=False, t_rand=None, want=None):
    """the fused ray front end (xrnerf_mi355_pipeline.h) -> dict of fp32 device tensors:
    rays_o, rays_d [R,3], viewdirs [R,3] (with_viewdirs), radii [R,1] (with_radii), near, far [R,1], z_vals [R,S] and pts [R,S,3] (S >= 1),
    target_s [R,C] (image or table).  c2w: [3,4] device tensor; sel: [R] int32 flat pixel indices or None (R consecutive pixels from
    pix0; R defaults to the rest of the frame); table: [R,3,3] rows (o, d, rgb).  want: the names to compute (default: all that apply);
    the others are not computed.  Nothing is read back."""
    H, W, S = int(H), int(W), int(S)
    src = c2w if c2w is not None else table
    if (c2w is None) == (table is None):
        raise _lib.XrError('pipe_ray_front: exactly one of c2w / table')
    if not _on_device(src) or src.dtype != torch.float32:
        raise _lib.XrError('pipe_ray_front: xrnerf_amd ops need fp32 ROCm device tensors (got %s on %s): there is no CPU fallback' % (src.dtype, src.device))
    dev = src.device
    if c2w is not None:
        if tuple(c2w.shape) != (3, 4):
            raise _lib.XrError('pipe_ray_front: c2w [3,4] (got %r)' % (tuple(c2w.shape),))
        if with_radii and H < 3:
            raise ValueError('pipe_ray_front: radii need H >= 3 (below that the reference returns fewer radii than rays)')
        if sel is not None:
            if sel.dtype != torch.int32 or sel.dim() != 1:
                raise _lib.XrError('pipe_ray_front: sel [R] int32')
            n = int(sel.shape[0])
        else:
            n = H * W - int(pix0) if R is None else int(R)
        if n < 0 or min(H, W) < 1 or (sel is None and int(pix0) + n > H * W) or int(pix0) < 0:
            raise _lib.XrError('pipe_ray_front: pixels %d .. %d of a %d x %d frame' % (pix0, int(pix0) + n, H, W))
        Cn = 0
        if image is not None:
            if image.dtype != torch.float32 or image.dim() != 3 or tuple(image.shape[:2]) != (H, W) or not 1 <= image.shape[2] <= PIPE_MAX_CHANNELS:
                raise _lib.XrError('pipe_ray_front: image [H,W,C] fp32, 1 <= C <= %d (got %r %s)' % (PIPE_MAX_CHANNELS, tuple(image.shape), image.dtype))
            Cn = int(image.shape[2])
    else:
        if table.dim() != 3 or tuple(table.shape[1:]) != (3, 3) or sel is not None or image is not None or with_radii:
            raise _lib.XrError('pipe_ray_front: table [R,3,3] without sel, image or radii')
        n, Cn = int(table.shape[0]), 3
    if t_rand is not None and (S < 1 or t_rand.dtype != torch.float32 or tuple(t_rand.shape) != (n, S)):
        raise _lib.XrError('pipe_ray_front: t_rand [R,S] fp32 (got %r %s at R %d S %d)' % (tuple(t_rand.shape), t_rand.dtype, n, S))
    have = {'rays_o': (n, 3), 'rays_d': (n, 3), 'near': (n, 1), 'far': (n, 1)}
    if with_viewdirs:
        have['viewdirs'] = (n, 3)
    if with_radii:
        have['radii'] = (n, 1)
    if S >= 1:
        have['z_vals'], have['pts'] = (n, S), (n, S, 3)
    if Cn:
        have['target_s'] = (n, Cn)
    names = [k for k in PIPE_OUTPUTS if k in have and (want is None or k in want or k in ('viewdirs', 'radii'))]
    if want is not None and [k for k in want if k not in have]:
        raise _lib.XrError('pipe_ray_front: %r asked for, the switches give %r' % (list(want), list(have)))
    out = {k: torch.empty(have[k], dtype=torch.float32, device=dev) for k in names}
    if n == 0:                  # nothing to launch (and an empty tensor has no pointer to hand over)
        return out
    fw, fh = pipe_ndc_factors(H, W, float(fx)) if ndc else (0., 0.)
    cont = lambda t: None if t is None else (t if t.is_contiguous() else t.contiguous())
    c2w, sel, image, table, t_rand = cont(c2w), cont(sel), cont(image), cont(table), cont(t_rand)
    with _span('xr_pipe_ray_front', n * max(S, 1), train=False):
        _lib.check(_lib.load().xr_pipe_ray_front(_ptr(c2w), float(fx), float(fy), float(cx), float(cy), H, W, _ptr(sel), int(pix0), n, _ptr(image), Cn,
                                                _ptr(table), int(bool(with_viewdirs)), int(bool(ndc)), int(bool(with_radii)), fw, fh, 1.0, float(near),
                                                float(far), S, int(bool(lindisp)), _ptr(t_rand), *[_ptr(out.get(k)) for k in PIPE_OUTPUTS], _stream()),
                   'xr_pipe_ray_front')
    return out


# ---------------------------------------------------------------- Mip-NeRF multiscale data (csrc/xr_multiscale.hip)
MS_CAM_DOUBLES = 24             # XR_MS_CAM_DOUBLES: pix2cam (9), cam2world rows 0..2 (12), lossmult, near, far
MS_MAX_DOWN = 8                 # XR_MS_MAX_DOWN
MS_OUTPUTS = ('rays_o', 'rays_d', 'viewdirs', 'radii', 'lossmult', 'near', 'far', 'z_vals', 'target_s')


def multiscale_kernels_available():
    """the loaded library handle has xr_multiscale.hip's entry points (see gnr_kernels_available)"""
    lib = _lib.load()
    return hasattr(lib, 'xr_ms_rays') and hasattr(lib, 'xr_ms_pyramid')


def ms_rays(cams, hw, prefix, sizes, images=None, idx=None, image=None, first_pixel=0, R=None, S=0, lindisp=False, t_rand=None, want=None):
    """rays of selected pixels of a multi-camera, multi-resolution image set (xrnerf_mi355_multiscale.h) -> dict of fp32 device tensors:
    rays_o, rays_d, viewdirs [R,3], radii, lossmult, near, far [R,1], z_vals [R,S] (S >= 1), target_s [R,3] (images given).
    cams [n,24] double, hw [n,2] int32, prefix [n+1] int64, images [total,3] fp32: device tensors; sizes: the host's list of (H, W), the
    same numbers as hw (nothing is read back to check a call).  Exactly one selection: idx, an int64 [R] device tensor of flat ray
    indices (an index outside [0, total) gives a NaN ray), or image (+ first_pixel, R: default the rest of the frame).  want: the names
    to compute (default: all that apply)."""
    S, n = int(S), len(sizes)
    if n < 1:
        raise _lib.XrError('ms_rays: an empty camera table')
    if min(int(h) for h, _ in sizes) < 3:             # dx[-2:-1] is empty below 3 rows: the reference returns fewer radii than rays
        raise ValueError('ms_rays: every image needs H >= 3 (got %r)' % (sorted({int(h) for h, _ in sizes})[0],))
    for t, dt, shape, name in ((cams, torch.float64, (n, MS_CAM_DOUBLES), 'cams'), (hw, torch.int32, (n, 2), 'hw'), (prefix, torch.int64, (n + 1,), 'prefix')):
        if not isinstance(t, torch.Tensor) or not _on_device(t) or t.dtype != dt or tuple(t.shape) != shape:
            raise _lib.XrError('ms_rays: %s must be a %s ROCm device tensor of shape %r: there is no CPU fallback' % (name, dt, shape))
    total = sum(int(h) * int(w) for h, w in sizes)
    dev = cams.device
    if images is not None and (not _on_device(images) or images.dtype != torch.float32 or tuple(images.shape) != (total, 3)):
        raise _lib.XrError('ms_rays: images [%d,3] fp32 on the device (got %r %s)' % (total, tuple(images.shape), images.dtype))
    if (idx is None) == (image is None):
        raise _lib.XrError('ms_rays: exactly one of idx / image')
    if idx is not None:
        if not isinstance(idx, torch.Tensor) or not _on_device(idx) or idx.dtype != torch.int64 or idx.dim() != 1:
            raise _lib.XrError('ms_rays: idx [R] int64 on the device')
        rays, image, first_pixel = int(idx.shape[0]), 0, 0
    else:
        image, first_pixel = int(image), int(first_pixel)
        if not 0 <= image < n:
            raise _lib.XrError('ms_rays: image %d of %d' % (image, n))
        frame = int(sizes[image][0]) * int(sizes[image][1])
        rays = frame - first_pixel if R is None else int(R)
        if first_pixel < 0 or rays < 0 or first_pixel + rays > frame:
            raise _lib.XrError('ms_rays: pixels %d .. %d of a frame of %d' % (first_pixel, first_pixel + rays, frame))
    if t_rand is not None and (S < 1 or t_rand.dtype != torch.float32 or tuple(t_rand.shape) != (rays, S) or not _on_device(t_rand)):
        raise _lib.XrError('ms_rays: t_rand [R,S] fp32 (got %r %s at R %d S %d)' % (tuple(t_rand.shape), t_rand.dtype, rays, S))
    have = {'rays_o': (rays, 3), 'rays_d': (rays, 3), 'viewdirs': (rays, 3), 'radii': (rays, 1), 'lossmult': (rays, 1), 'near': (rays, 1), 'far': (rays, 1)}
    if S >= 1:
        have['z_vals'] = (rays, S)
    if images is not None:
        have['target_s'] = (rays, 3)
    if want is not None and [k for k in want if k not in have]:
        raise _lib.XrError('ms_rays: %r asked for, the arguments give %r' % (list(want), list(have)))
    out = {k: torch.empty(have[k], dtype=torch.float32, device=dev) for k in MS_OUTPUTS if k in have and (want is None or k in want)}
    if rays == 0:               # nothing to launch (and an empty tensor has no pointer to hand over)
        return out
    cont = lambda t: None if t is None else (t if t.is_contiguous() else t.contiguous())
    cams, hw, prefix, images, idx, t_rand = cont(cams), cont(hw), cont(prefix), cont(images), cont(idx), cont(t_rand)
    with _span('xr_ms_rays', rays * max(S, 1), train=False):
        _lib.check(_lib.load().xr_ms_rays(_ptr(cams), _ptr(hw), _ptr(prefix), n, total, _ptr(images), _ptr(idx), image, first_pixel, rays, S,
                                         int(bool(lindisp)), _ptr(t_rand), *[_ptr(out.get(k)) for k in MS_OUTPUTS], _stream()), 'xr_ms_rays')
    return out


def ms_pyramid_sizes(H, W, n_down):
    """[(H >> j, W >> j)] of the n_down levels; ValueError when the base does not halve n_down - 1 times (the reference's reshape raises)"""
    H, W, n_down = int(H), int(W), int(n_down)
    if not 1 <= n_down <= MS_MAX_DOWN:
        raise ValueError('ms_pyramid: n_down must be 1 .. %d (got %d)' % (MS_MAX_DOWN, n_down))
    if min(H, W) < 1 or H % (1 << (n_down - 1)) or W % (1 << (n_down - 1)):
        raise ValueError('ms_pyramid: a %d x %d image cannot be halved %d times' % (H, W, n_down - 1))
    return [(H >> j, W >> j) for j in range(n_down)]


def ms_pyramid(base, n_down, white_bkgd=True, want=('bytes', 'pixels')):
    """the multiscale converter's image side (xrnerf_mi355_multiscale.h): base [N,H,W,C] uint8 device tensor (C = 3 or 4) ->
    {'bytes': [N per_view, C] uint8 (what the converter saves), 'pixels': [N per_view, 3] fp32 (what load_multiscale_data loads)}, packed
    view-major with a view's levels consecutive; per_view = sum of the level sizes (ms_pyramid_sizes)."""
    if not isinstance(base, torch.Tensor) or not _on_device(base) or base.dtype != torch.uint8 or base.dim() != 4 or base.shape[3] not in (3, 4):
        raise _lib.XrError('ms_pyramid: base must be a [N,H,W,3 or 4] uint8 ROCm device tensor: there is no CPU fallback')
    N, H, W, Cn = (int(v) for v in base.shape)
    per_view = sum(h * w for h, w in ms_pyramid_sizes(H, W, n_down))
    out = {}
    if 'bytes' in want:
        out['bytes'] = torch.empty((N * per_view, Cn), dtype=torch.uint8, device=base.device)
    if 'pixels' in want:
        out['pixels'] = torch.empty((N * per_view, 3), dtype=torch.float32, device=base.device)
    if not out:
        raise _lib.XrError('ms_pyramid: nothing asked for')
    if N == 0:
        return out
    base = base if base.is_contiguous() else base.contiguous()
    with _span('xr_ms_pyramid', N * per_view, train=False):
        _lib.check(_lib.load().xr_ms_pyramid(_ptr(base), N, H, W, Cn, int(n_down), int(bool(white_bkgd)), _ptr(out.get('bytes')), _ptr(out.get('pixels')),
                                            _stream()), 'xr_ms_pyramid')
    return out


# ---------------------------------------------------------------- ZJU-MoCap / H36M human data (csrc/xr_bodydata.hip)
BODY_CAM_DOUBLES = 30           # XR_BODY_CAM_DOUBLES: inv(K) (9), R (9), T (3), rays_o (3), bounds min (3), bounds max (3)
BODY_ROUNDS = 8                 # XR_BODY_ROUNDS
BODY_MAX_SEL = 65536            # XR_BODY_MAX_SEL
BODY_MAX_SHRINK = 16            # XR_BODY_MAX_SHRINK
_BODY_ENTRIES = ('xr_body_prepare', 'xr_body_masks', 'xr_body_sample', 'xr_body_points', 'xr_body_frame_count', 'xr_body_frame_write')


def bodydata_kernels_available():
    """the loaded library handle has xr_bodydata.hip's entry points (see gnr_kernels_available)"""
    lib = _lib.load()
    return all(hasattr(lib, name) for name in _BODY_ENTRIES)


def _body_dev(t, dtype, shape, what):
    if not isinstance(t, torch.Tensor) or not _on_device(t) or t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise _lib.XrError('%s must be a %s ROCm device tensor%s: there is no CPU fallback' % (what, dtype, '' if shape is None else ' of shape %r' % (tuple(shape),)))
    return t if t.is_contiguous() else t.contiguous()


def body_shrink(ratio):
    """the integer s = 1 / ratio the block mean is defined for; anything else is refused by name"""
    s = int(round(1. / float(ratio))) if float(ratio) > 0 else 0
    if s < 1 or s > BODY_MAX_SHRINK or abs(s * float(ratio) - 1.) > 1e-12:
        raise NotImplementedError('body_prepare: ratio %r is not supported (1 / ratio must be an integer 1 .. %d)' % (ratio, BODY_MAX_SHRINK))
    return s


def body_prepare(img8, msk8, K, D, ratio, white_bkgd):
    """the prepared picture (xrnerf_mi355_bodydata.h): img8 [Hs,Ws,3] and msk8 [Hm,Wm] uint8 device tensors, K [3,3] (unscaled) and D (5)
    host values -> (img [H,W,3] fp32, msk [H,W] uint8) on the device, H = Hs ratio, W = Ws ratio.  One launch, nothing read back."""
    s = body_shrink(ratio)
    img8, msk8 = _body_dev(img8, torch.uint8, None, 'body_prepare: img8'), _body_dev(msk8, torch.uint8, None, 'body_prepare: msk8')
    if img8.dim() != 3 or img8.shape[2] != 3 or msk8.dim() != 2:
        raise _lib.XrError('body_prepare: img8 [Hs,Ws,3] and msk8 [Hm,Wm] (got %r, %r)' % (tuple(img8.shape), tuple(msk8.shape)))
    Hs, Ws = int(img8.shape[0]), int(img8.shape[1])
    if Hs % s or Ws % s:
        raise ValueError('body_prepare: a %d x %d picture cannot be shrunk by %d' % (Hs, Ws, s))
    kd = np.concatenate([np.asarray(K, np.float64).reshape(9), np.asarray(D, np.float64).reshape(-1)[:5]])
    if kd.shape[0] != 14:
        raise _lib.XrError('body_prepare: K [3,3] and D of 5 coefficients')
    img = torch.empty((Hs // s, Ws // s, 3), dtype=torch.float32, device=img8.device)
    msk = torch.empty((Hs // s, Ws // s), dtype=torch.uint8, device=img8.device)
    with _span('xr_body_prepare', img.numel() // 3, train=False):
        _lib.check(_lib.load().xr_body_prepare(_ptr(img8), _ptr(msk8), Hs, Ws, int(msk8.shape[0]), int(msk8.shape[1]), kd.ctypes.data_as(C.c_void_p), s,
                                              int(bool(white_bkgd)), _ptr(img), _ptr(msk), _stream()), 'xr_body_prepare')
    return img, msk


def body_masks(msk, corners):
    """the two candidate lists of a prepared picture: msk [H,W] uint8 device tensor, corners [8,2] host integers (x, y) ->
    (bound_list, body_list) int32 device tensors in argwhere order.  ONE blocking read, of the two lengths (made once per picture)."""
    msk = _body_dev(msk, torch.uint8, None, 'body_masks: msk')
    if msk.dim() != 2:
        raise _lib.XrError('body_masks: msk [H,W]')
    H, W = int(msk.shape[0]), int(msk.shape[1])
    c = np.ascontiguousarray(np.asarray(corners).reshape(16), dtype=np.int64)
    if np.abs(c).max() > (1 << 30):
        raise ValueError('body_masks: a projected corner lies beyond +-2^30 pixels')
    c = c.astype(np.int32)
    lib = _lib.load()
    nbytes = int(lib.xr_body_masks_workspace_bytes(H, W))
    ws = _ws(msk.device, nbytes, 'bodymasks')
    bound = torch.empty(H * W, dtype=torch.int32, device=msk.device)
    body = torch.empty(H * W, dtype=torch.int32, device=msk.device)
    totals = torch.empty(2, dtype=torch.int32, device=msk.device)
    with _span('xr_body_masks', H * W, train=False):
        _lib.check(lib.xr_body_masks(_ptr(msk), H, W, c.ctypes.data_as(C.c_void_p), _ptr(bound), _ptr(body), _ptr(totals), _ptr(ws), nbytes, _stream()),
                   'xr_body_masks')
    nb, nh = (int(v) for v in totals.tolist())
    if nb < 0 or nh < 0:
        raise _lib.XrError('body_masks: a list total beyond int32')
    return bound[:nb].clone(), body[:nh].clone()


def body_sample(cam, H, W, img, body_list, bound_list, draws, short_items, S=0, t_rand=None, fused_points=False, want_target=True):
    """one training item (xrnerf_mi355_bodydata.h) -> dict of fp32 device tensors rays_o, rays_d [n,3], near, far [n,1], target_s [n,3],
    and with S >= 1 z_vals [n,S], pts [n,S,3].  cam [30] double, img [H,W,3] fp32, the lists int32, draws [8,n] int64, short_items [1]
    uint32 (the persistent counter): device tensors.  fused_points: z_vals and pts by the sampling workgroup itself (one launch) instead
    of a second wide launch.  Empty lists raise ValueError before anything is launched.  Nothing is read back."""
    H, W, S = int(H), int(W), int(S)
    cam = _body_dev(cam, torch.float64, (BODY_CAM_DOUBLES,), 'body_sample: cam')
    body_list = _body_dev(body_list, torch.int32, None, 'body_sample: body_list')
    bound_list = _body_dev(bound_list, torch.int32, None, 'body_sample: bound_list')
    draws = _body_dev(draws, torch.int64, None, 'body_sample: draws')
    short_items = _body_dev(short_items, torch.int32, (1,), 'body_sample: short_items')
    if draws.dim() != 2 or draws.shape[0] != BODY_ROUNDS:
        raise _lib.XrError('body_sample: draws [%d, sel_n] int64 (got %r)' % (BODY_ROUNDS, tuple(draws.shape)))
    n = int(draws.shape[1])
    if body_list.numel() == 0 or bound_list.numel() == 0:
        raise ValueError('body_sample: an empty candidate list (body %d, bound %d): the reference\'s randint(0, 0) raises too' % (body_list.numel(), bound_list.numel()))
    if want_target:
        img = _body_dev(img, torch.float32, (H, W, 3), 'body_sample: img')
    if t_rand is not None:
        t_rand = _body_dev(t_rand, torch.float32, (n, S), 'body_sample: t_rand')
    dev = cam.device
    out = {'rays_o': torch.empty((n, 3), dtype=torch.float32, device=dev), 'rays_d': torch.empty((n, 3), dtype=torch.float32, device=dev),
           'near': torch.empty((n, 1), dtype=torch.float32, device=dev), 'far': torch.empty((n, 1), dtype=torch.float32, device=dev)}
    if want_target:
        out['target_s'] = torch.empty((n, 3), dtype=torch.float32, device=dev)
    zp = {}
    if S >= 1:
        zp = {'z_vals': torch.empty((n, S), dtype=torch.float32, device=dev), 'pts': torch.empty((n, S, 3), dtype=torch.float32, device=dev)}
    inside = bool(fused_points) and S >= 1
    with _span('xr_body_sample', n * (S if inside else 1), train=False):
        _lib.check(_lib.load().xr_body_sample(_ptr(cam), H, W, _ptr(img) if want_target else None, _ptr(body_list), int(body_list.numel()), _ptr(bound_list),
                                             int(bound_list.numel()), _ptr(draws), n, S if inside else 0, _ptr(t_rand) if inside else None,
                                             _ptr(out['rays_o']), _ptr(out['rays_d']), _ptr(out['near']), _ptr(out['far']), _ptr(out.get('target_s')),
                                             _ptr(zp.get('z_vals')) if inside else None, _ptr(zp.get('pts')) if inside else None, _ptr(short_items),
                                             _stream()), 'xr_body_sample')
    if S >= 1 and not inside:
        with _span('xr_body_points', n * S, train=False):
            _lib.check(_lib.load().xr_body_points(_ptr(out['rays_o']), _ptr(out['rays_d']), _ptr(out['near']), _ptr(out['far']), n, S, _ptr(t_rand),
                                                 _ptr(zp['z_vals']), _ptr(zp['pts']), _stream()), 'xr_body_points')
    out.update(zp)
    return out


def body_points(rays_o, rays_d, near, far, S, t_rand=None):
    """z_vals [R,S] and pts [R,S,3] of R rays with per-ray near / far (xr_body_points): one launch"""
    S, R = int(S), int(rays_o.shape[0])
    rays_o, rays_d = _body_dev(rays_o, torch.float32, (R, 3), 'body_points: rays_o'), _body_dev(rays_d, torch.float32, (R, 3), 'body_points: rays_d')
    near, far = _body_dev(near, torch.float32, (R, 1), 'body_points: near'), _body_dev(far, torch.float32, (R, 1), 'body_points: far')
    if S < 1:
        raise _lib.XrError('body_points: S >= 1')
    if t_rand is not None:
        t_rand = _body_dev(t_rand, torch.float32, (R, S), 'body_points: t_rand')
    out = {'z_vals': torch.empty((R, S), dtype=torch.float32, device=rays_o.device), 'pts': torch.empty((R, S, 3), dtype=torch.float32, device=rays_o.device)}
    if R == 0:
        return out
    with _span('xr_body_points', R * S, train=False):
        _lib.check(_lib.load().xr_body_points(_ptr(rays_o), _ptr(rays_d), _ptr(near), _ptr(far), R, S, _ptr(t_rand), _ptr(out['z_vals']), _ptr(out['pts']),
                                             _stream()), 'xr_body_points')
    return out


def body_frame(cam, H, W, img=None):
    """a whole frame (NBSelectRays(sel_all=True)) -> dict: mask_at_box [H W] bool, rays_o, rays_d [M,3], near, far [M,1], target_s [M,3]
    (img given), the M survivors in nonzero order.  ONE blocking read, of M."""
    H, W = int(H), int(W)
    cam = _body_dev(cam, torch.float64, (BODY_CAM_DOUBLES,), 'body_frame: cam')
    if img is not None:
        img = _body_dev(img, torch.float32, (H, W, 3), 'body_frame: img')
    if min(H, W) < 1 or H * W > 0x7fffffff:
        raise _lib.XrError('body_frame: H, W >= 1 and H W within int32 (got %d x %d)' % (H, W))
    lib, dev = _lib.load(), cam.device
    nbytes = int(lib.xr_body_frame_workspace_bytes(H, W))
    ws = _ws(dev, nbytes, 'bodyframe')
    mask = torch.empty(H * W, dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    with _span('xr_body_frame_count', H * W, train=False):
        _lib.check(lib.xr_body_frame_count(_ptr(cam), H, W, _ptr(mask), _ptr(total), _ptr(ws), nbytes, _stream()), 'xr_body_frame_count')
    M = int(total.item())
    if M < 0:
        raise _lib.XrError('body_frame: the survivor count does not fit int32')
    out = {'mask_at_box': mask.view(torch.bool),
           'rays_o': torch.empty((M, 3), dtype=torch.float32, device=dev), 'rays_d': torch.empty((M, 3), dtype=torch.float32, device=dev),
           'near': torch.empty((M, 1), dtype=torch.float32, device=dev), 'far': torch.empty((M, 1), dtype=torch.float32, device=dev)}
    if img is not None:
        out['target_s'] = torch.empty((M, 3), dtype=torch.float32, device=dev)
    if M:
        with _span('xr_body_frame_write', M, train=False):
            _lib.check(lib.xr_body_frame_write(_ptr(cam), H, W, _ptr(img), _ptr(mask), _ptr(ws), nbytes, M, _ptr(out['rays_o']), _ptr(out['rays_d']),
                                              _ptr(out['near']), _ptr(out['far']), _ptr(out.get('target_s')), _stream()), 'xr_body_frame_write')
    return out


# ---------------------------------------------------------------- GeneBody data (csrc/xr_genebody.hip)
GB_MAX_VIEWS = 64               # XR_GB_MAX_VIEWS
GB_MAX_DIST = 8                 # XR_GB_MAX_DIST
_GB_ENTRIES = ('xr_gb_crop_box', 'xr_gb_resize', 'xr_gb_assemble', 'xr_gb_calib')


def genebody_kernels_available():
    """the loaded library handle has xr_genebody.hip's entry points (see gnr_kernels_available)"""
    lib = _lib.load()
    return all(hasattr(lib, name) for name in _GB_ENTRIES)


def gb_pack(arrays, dtype, device, align=16):
    """host arrays -> (one device tensor holding them back to back, each on `align` bytes; their ELEMENT offsets)"""
    item = np.dtype(dtype).itemsize
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += -(-a.size * item // align) * align // item
    flat = np.zeros(max(total, 1), dtype)
    for a, o in zip(arrays, offs):
        flat[o:o + a.size] = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    if flat.dtype == np.uint16:
        flat = flat.view(np.int16)          # the bits travel as int16: the kernel reads them as uint16
    return torch.from_numpy(flat).to(device), offs


def _gb_ptrs(tensors):
    """a host array of device pointers (the entry points copy it into their kernel arguments)"""
    return (C.c_void_p * len(tensors))(*[_ptr(t).value for t in tensors])


def gb_crop_box(masks, device=None):
    """the crop boxes of raw masks: a list of host uint8 [h,w] arrays, or (device bytes, [(offset, h, w)]) -> [n,4] int32 device tensor
    (top, left, bottom, right).  ONE launch, nothing read back."""
    if isinstance(masks, tuple):
        flat, entries = masks
    else:
        flat, offs = gb_pack(masks, np.uint8, device)
        entries = [(o, m.shape[0], m.shape[1]) for o, m in zip(offs, masks)]
    flat = _body_dev(flat, torch.uint8, None, 'gb_crop_box: masks')
    n = len(entries)
    if n < 1 or n > GB_MAX_VIEWS:
        raise _lib.XrError('gb_crop_box: 1 .. %d masks a launch (got %d)' % (GB_MAX_VIEWS, n))
    for o, h, w in entries:
        if o < 0 or o + h * w > flat.numel():
            raise _lib.XrError('gb_crop_box: a mask of %d x %d at %d leaves the buffer of %d bytes' % (h, w, o, flat.numel()))
    table = np.ascontiguousarray(np.array(entries, np.int64).reshape(n, 3))
    boxes = torch.empty((n, 4), dtype=torch.int32, device=flat.device)
    with _span('xr_gb_crop_box', n, train=False):
        _lib.check(_lib.load().xr_gb_crop_box(_ptr(flat), table.ctypes.data_as(C.c_void_p), n, _ptr(boxes), _stream()), 'xr_gb_crop_box')
    return boxes


def gb_resize(imgs, masks, depths, entries, boxes, S):
    """the resized planes of n views.  imgs, masks: device uint8 buffers, depths: device int16 buffer holding uint16 bits (or None);
    entries: [(img_off, mask_off, depth_off or -1, h, w)] in elements; boxes [n,4] int32 device -> (rgb [n,S,S,3] uint8, m8 [n,S,S] uint8,
    depth [n,S,S] fp32 or None).  ONE launch, nothing read back."""
    S, n = int(S), len(entries)
    imgs, masks = _body_dev(imgs, torch.uint8, None, 'gb_resize: imgs'), _body_dev(masks, torch.uint8, None, 'gb_resize: masks')
    boxes = _body_dev(boxes, torch.int32, (n, 4), 'gb_resize: boxes')
    any_depth = any(e[2] >= 0 for e in entries)
    if any_depth:
        depths = _body_dev(depths, torch.int16, None, 'gb_resize: depths')
    if n < 1 or n > GB_MAX_VIEWS:
        raise _lib.XrError('gb_resize: 1 .. %d views a launch (got %d)' % (GB_MAX_VIEWS, n))
    for io, mo, do, h, w in entries:
        if io < 0 or mo < 0 or io + h * w * 3 > imgs.numel() or mo + h * w > masks.numel() or (do >= 0 and do + h * w > depths.numel()):
            raise _lib.XrError('gb_resize: a view of %d x %d leaves its buffer' % (h, w))
    table = np.ascontiguousarray(np.array(entries, np.int64).reshape(n, 5))
    dev = imgs.device
    rgb = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
    m8 = torch.empty((n, S, S), dtype=torch.uint8, device=dev)
    depth = torch.zeros((n, S, S), dtype=torch.float32, device=dev) if any_depth else None
    with _span('xr_gb_resize', n * S * S, train=False):
        _lib.check(_lib.load().xr_gb_resize(_ptr(imgs), _ptr(masks), _ptr(depths) if any_depth else None, table.ctypes.data_as(C.c_void_p), n, _ptr(boxes), S,
                                           _ptr(rgb), _ptr(m8), _ptr(depth), _stream()), 'xr_gb_resize')
    return rgb, m8, depth


def gb_assemble(rgb, m8, depth, num_views, S, white_bkgd):
    """one item's V views in their roles.  rgb, m8: lists of V device tensors ([S,S,3], [S,S] uint8); depth: list of num_views fp32 [S,S]
    device tensors or None -> (img [V,3,S,S], mask [num_views,1,S,S], smpl_depth [num_views,S,S] or None, acc [2,V,2] int32).
    Two memsets and ONE launch, nothing read back."""
    V, S, num_views = len(rgb), int(S), int(num_views)
    if V < 1 or V > GB_MAX_VIEWS or len(m8) != V or num_views > V or (depth is not None and len(depth) != num_views):
        raise _lib.XrError('gb_assemble: 1 .. %d views, as many masks, num_views depth maps' % GB_MAX_VIEWS)
    rgb = [_body_dev(t, torch.uint8, (S, S, 3), 'gb_assemble: rgb') for t in rgb]
    m8 = [_body_dev(t, torch.uint8, (S, S), 'gb_assemble: m8') for t in m8]
    if depth is not None:
        depth = [_body_dev(t, torch.float32, (S, S), 'gb_assemble: depth') for t in depth]
    dev = rgb[0].device
    img = torch.empty((V, 3, S, S), dtype=torch.float32, device=dev)
    mask = torch.empty((num_views, 1, S, S), dtype=torch.float32, device=dev)
    smpl_depth = torch.empty((num_views, S, S), dtype=torch.float32, device=dev) if depth is not None else None
    acc = torch.empty((2, V, 2), dtype=torch.int32, device=dev)
    with _span('xr_gb_assemble', V * S * S, train=False):
        _lib.check(_lib.load().xr_gb_assemble(_gb_ptrs(rgb), _gb_ptrs(m8), _gb_ptrs(depth) if depth is not None else None, V, num_views, S, int(bool(white_bkgd)),
                                             _ptr(img), _ptr(mask), _ptr(smpl_depth), _ptr(acc), _stream()), 'xr_gb_assemble')
    return img, mask, smpl_depth, acc


def gb_calib(verts, K, D, w2c, crops, acc, num_views, S):
    """one item's camera rows and scalars.  verts [N,3], K [V,3,3], D [V,nd], w2c [V,4,4] fp32 device tensors, crops: list of V int32 [4]
    device tensors, acc: gb_assemble's -> dict persps [V,4+nd+2] fp32, vboxes [V,4] int32, sf_views [num_views] fp64, bbox [4] fp64,
    spatial_freq [] fp64, center [3] fp32.  ONE launch, nothing read back."""
    V, S, num_views = len(crops), int(S), int(num_views)
    verts = _body_dev(verts, torch.float32, None, 'gb_calib: verts')
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] < 1:
        raise _lib.XrError('gb_calib: verts [N,3] with N >= 1')
    K, w2c = _body_dev(K, torch.float32, (V, 3, 3), 'gb_calib: K'), _body_dev(w2c, torch.float32, (V, 4, 4), 'gb_calib: w2c')
    D = _body_dev(D, torch.float32, None, 'gb_calib: D')
    nd = int(D.numel() // V) if V else 0
    if V < 2 or V > GB_MAX_VIEWS or not 1 <= num_views < V or D.numel() != V * nd or nd > GB_MAX_DIST:
        raise _lib.XrError('gb_calib: 2 .. %d views, 1 <= num_views < V, at most %d distortion coefficients' % (GB_MAX_VIEWS, GB_MAX_DIST))
    crops = [_body_dev(t, torch.int32, (4,), 'gb_calib: crop') for t in crops]
    acc = _body_dev(acc, torch.int32, (2, V, 2), 'gb_calib: acc')
    dev = verts.device
    out = {'persps': torch.empty((V, 4 + nd + 2), dtype=torch.float32, device=dev), 'vboxes': torch.empty((V, 4), dtype=torch.int32, device=dev),
           'sf_views': torch.empty(num_views, dtype=torch.float64, device=dev), 'bbox': torch.empty(4, dtype=torch.float64, device=dev),
           'spatial_freq': torch.empty((), dtype=torch.float64, device=dev), 'center': torch.empty(3, dtype=torch.float32, device=dev)}
    with _span('xr_gb_calib', V * int(verts.shape[0]), train=False):
        _lib.check(_lib.load().xr_gb_calib(_ptr(verts), int(verts.shape[0]), _ptr(K), _ptr(D), nd, _ptr(w2c), _gb_ptrs(crops), _ptr(acc), V, num_views, S,
                                          _ptr(out['persps']), _ptr(out['vboxes']), _ptr(out['sf_views']), _ptr(out['bbox']), _ptr(out['spatial_freq']),
                                          _ptr(out['center']), _stream()), 'xr_gb_calib')
    return out


# ---------------------------------------------------------------- BungeeNeRF data (csrc/xr_bungeedata.hip)
BGD_CAM_DOUBLES = 12            # XR_BGD_CAM_DOUBLES: cam2world rows 0..2
BGD_MAX_SAMPLES = 1024          # XR_BGD_MAX_SAMPLES
BGD_ITEM_OUTPUTS = ('rays_o', 'rays_d', 'target_s', 'radii', 'scale_code', 'viewdirs', 'near', 'far', 'z_vals')
BGD_FRAME_OUTPUTS = ('rays_o', 'rays_d', 'radii', 'viewdirs', 'near', 'far', 'z_vals')


def bungeedata_kernels_available():
    """the loaded library handle has xr_bungeedata.hip's entry points (see gnr_kernels_available)"""
    lib = _lib.load()
    return hasattr(lib, 'xr_bgd_item') and hasattr(lib, 'xr_bgd_frame')


def _bgd_bounds(ray_nearfar, scene_origin, scaling, S, who):
    """the bounds arguments both entry points take, from bungee_zvals' own: (mode, globe centre, r2_top, r2_earth, scaling)"""
    if ray_nearfar not in ('sphere', 'flat'):
        raise _lib.XrError("%s: ray_nearfar must be 'sphere' or 'flat' (got %r)" % (who, ray_nearfar))
    if S and not 2 <= S <= BGD_MAX_SAMPLES:
        raise _lib.XrError('%s: 2 <= N_samples <= %d (got %d)' % (who, BGD_MAX_SAMPLES, S))
    s = float(scaling)
    gc = (C.c_float * 3)(*[float(v) * s for v in scene_origin])
    return _BUNGEE_BOUNDS[ray_nearfar], gc, ((EARTH_RADIUS + 250.0) * s) ** 2, (EARTH_RADIUS * s) ** 2, s


def bgd_item(cams, codes, images, i_train, H, W, focal, perm, start, R, S=0, ray_nearfar='sphere', scene_origin=(0., 0., 0.), scaling=1.0, t_rand=None,
             want=None):
    """one BungeeNeRF training item (xrnerf_mi355_bungeedata.h) -> dict: rays_o, rays_d, target_s, viewdirs [n,3], radii, near, far [n,1]
    fp32, scale_code [n,1] int64, z_vals [n,S] (S >= 2).  cams [N,12] double, codes [N] int64, images [N,H,W,3] fp32, i_train [T] int32,
    perm int64 [.]: device tensors.  The rays are perm[start : start + R], cut where perm ends (n <= R, as slicing gives); an entry
    outside [0, T H W) gives a NaN ray.  want: the names to compute (default: all that apply)."""
    H, W, S, start, R = int(H), int(W), int(S), int(start), int(R)
    if H < 3:                    # dx[:, -2:-1] is empty below 3 rows: the reference returns fewer radii than rays
        raise ValueError('bgd_item: H >= 3 (got %d)' % H)
    cams = _body_dev(cams, torch.float64, None, 'bgd_item: cams')
    N = int(cams.shape[0])
    if cams.dim() != 2 or cams.shape[1] != BGD_CAM_DOUBLES or N < 1 or W < 1:
        raise _lib.XrError('bgd_item: cams [N,12] with N >= 1, W >= 1')
    codes, images = _body_dev(codes, torch.int64, (N,), 'bgd_item: codes'), _body_dev(images, torch.float32, (N, H, W, 3), 'bgd_item: images')
    i_train, perm = _body_dev(i_train, torch.int32, None, 'bgd_item: i_train'), _body_dev(perm, torch.int64, None, 'bgd_item: perm')
    T = int(i_train.numel())
    if i_train.dim() != 1 or T < 1 or perm.dim() != 1 or start < 0 or R < 0:
        raise _lib.XrError('bgd_item: i_train [T] with T >= 1, perm [.], start and R >= 0')
    n = max(0, min(R, int(perm.shape[0]) - start))
    have = {'rays_o': (n, 3), 'rays_d': (n, 3), 'target_s': (n, 3), 'radii': (n, 1), 'scale_code': (n, 1), 'viewdirs': (n, 3), 'near': (n, 1), 'far': (n, 1)}
    if S >= 1:
        have['z_vals'] = (n, S)
    if want is not None and [k for k in want if k not in have]:
        raise _lib.XrError('bgd_item: %r asked for, the arguments give %r' % (list(want), list(have)))
    mode, gc, r2_top, r2_earth, s = _bgd_bounds(ray_nearfar, scene_origin, scaling, S, 'bgd_item')
    if t_rand is not None:
        t_rand = _body_dev(t_rand, torch.float32, (n, S), 'bgd_item: t_rand')
    dev = cams.device
    out = {k: torch.empty(have[k], dtype=torch.int64 if k == 'scale_code' else torch.float32, device=dev)
           for k in BGD_ITEM_OUTPUTS if k in have and (want is None or k in want)}
    if n == 0:                  # nothing to launch (and an empty tensor has no pointer to hand over)
        return out
    with _span('xr_bgd_item', n * max(S, 1), train=False):
        _lib.check(_lib.load().xr_bgd_item(_ptr(cams), _ptr(codes), _ptr(images), _ptr(i_train), N, T, H, W, float(focal), float(W * .5), float(H * .5),
                                          _ptr(perm), start, n, S if 'z_vals' in out else 0, mode, C.cast(gc, C.c_void_p), r2_top, r2_earth, s,
                                          _ptr(t_rand) if 'z_vals' in out else None, *[_ptr(out.get(k)) for k in BGD_ITEM_OUTPUTS], _stream()), 'xr_bgd_item')
    return out


def bgd_frame(c2w, H, W, K, S=0, ray_nearfar='sphere', scene_origin=(0., 0., 0.), scaling=1.0, want=None):
    """one BungeeNeRF validation frame (xrnerf_mi355_bungeedata.h): GetRays(include_radius=True) + FlattenRays + GetViewdirs +
    BungeeGetBounds + BungeeGetZvals of pose c2w [3,4] fp32 (device) -> dict of fp32 device tensors rays_o, rays_d (not normalised),
    viewdirs [H W,3], radii, near, far [H W,1], z_vals [H W,S] (S >= 2).  want: the names to compute (default: all that apply)."""
    H, W, S = int(H), int(W), int(S)
    if H < 3:                    # dx[-2:-1] is empty below 3 rows: the reference returns fewer radii than rays
        raise ValueError('bgd_frame: GetRays(include_radius=True) needs H >= 3 (got %d)' % H)
    c2w = _body_dev(c2w, torch.float32, (3, 4), 'bgd_frame: c2w')
    if W < 1:
        raise _lib.XrError('bgd_frame: W >= 1')
    n = H * W
    have = {'rays_o': (n, 3), 'rays_d': (n, 3), 'radii': (n, 1), 'viewdirs': (n, 3), 'near': (n, 1), 'far': (n, 1)}
    if S >= 1:
        have['z_vals'] = (n, S)
    if want is not None and [k for k in want if k not in have]:
        raise _lib.XrError('bgd_frame: %r asked for, the arguments give %r' % (list(want), list(have)))
    mode, gc, r2_top, r2_earth, s = _bgd_bounds(ray_nearfar, scene_origin, scaling, S, 'bgd_frame')
    out = {k: torch.empty(have[k], dtype=torch.float32, device=c2w.device) for k in BGD_FRAME_OUTPUTS if k in have and (want is None or k in want)}
    with _span('xr_bgd_frame', n * max(S, 1), train=False):
        _lib.check(_lib.load().xr_bgd_frame(_ptr(c2w), H, W, float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]), S if 'z_vals' in out else 0,
                                           mode, C.cast(gc, C.c_void_p), r2_top, r2_earth, s, *[_ptr(out.get(k)) for k in BGD_FRAME_OUTPUTS], _stream()),
                   'xr_bgd_frame')
    return out


# ------------------------------------------------------------------ KiloNeRF distillation's validation numbers (xrnerf_mi355_kilotree.h)
KILOTREE_COLS = 16                       # XR_KILOTREE_COLS
KILOTREE_MAX_POINTS = 1 << 24            # XR_KILOTREE_MAX_POINTS
KT_MSE, KT_MAE, KT_MAPE, KT_QUANTILE, KT_SATURATION, KT_THRESHOLD, KT_METRIC_MAX = 0, 3, 6, 9, 12, 13, 14
KILOTREE_METRICS = {'mse': 0, 'mae': 1, 'mape': 2}


def kilotree_kernels_available():
    """the loaded library handle has xr_kilotree.hip's entry point (see gnr_kernels_available)"""
    return hasattr(_lib.load(), 'xr_kilotree_val_metrics')


def _kt_rows(t, cols, N, P, what):
    """(data pointer, network stride, row stride) of an [N, P, cols] fp32 device view whose rows are contiguous: no copy is made of a
    column slice of wider example rows"""
    if not _on_device(t):
        raise _lib.XrError('xrnerf_amd ops need ROCm device tensors (got a %s tensor): there is no CPU fallback' % t.device)
    if t.dtype != torch.float32 or tuple(t.shape) != (N, P, cols):
        raise _lib.XrError('kilo_val_metrics: %s [%d, %d, %d] fp32 (got %s %r)' % (what, N, P, cols, t.dtype, tuple(t.shape)))
    if t.stride(2) != 1 or t.stride(1) < 0 or t.stride(0) < 0:
        t = t.contiguous()
    return t, C.c_void_p(t.data_ptr()), int(t.stride(0)), int(t.stride(1))


def kilo_val_metrics(out, targets, quantile_index, points=None, split_axis=None, split_metric='mse', want_point_metric=False):
    """one validation pass of N student networks -> (table [N, KILOTREE_COLS] fp32 on the device, point_metric [N, P] or None).
    out [N,P,4]; targets [N,P,4] and points [N,P,3] may be column slices of the example rows.  split_axis: [N] int32 device tensor (or a
    list of ints), -1 = no split wanted for that network.  The columns (KT_*) and their arithmetic are xrnerf_mi355_kilotree.h's.
    quantile_index outside [0, P) is refused (-22).  Nothing is read back."""
    if out.dim() != 3 or out.shape[2] != 4 or out.dtype != torch.float32:
        raise _lib.XrError('kilo_val_metrics: out [N, P, 4] fp32 (got %s %r)' % (out.dtype, tuple(out.shape)))
    if split_metric not in KILOTREE_METRICS:
        raise _lib.XrError('kilo_val_metrics: split_metric is one of %r (got %r)' % (sorted(KILOTREE_METRICS), split_metric))
    N, P = int(out.shape[0]), int(out.shape[1])
    if not out.is_contiguous() or out.data_ptr() % 16:
        out = out.contiguous().clone() if out.data_ptr() % 16 else out.contiguous()
    targets, pt, t_net, t_row = _kt_rows(targets, 4, N, P, 'targets')
    pp, p_net, p_row = None, 0, 0
    axis = None
    if split_axis is not None:
        if points is None:
            raise _lib.XrError('kilo_val_metrics: split_axis needs points')
        points, pp, p_net, p_row = _kt_rows(points, 3, N, P, 'points')
        axis = split_axis if torch.is_tensor(split_axis) else torch.tensor([int(v) for v in split_axis], dtype=torch.int32)
        axis = axis.to(device=out.device, dtype=torch.int32).contiguous()
        if tuple(axis.shape) != (N,):
            raise _lib.XrError('kilo_val_metrics: split_axis [%d] (got %r)' % (N, tuple(axis.shape)))
    table = torch.empty((N, KILOTREE_COLS), dtype=torch.float32, device=out.device)
    pm = torch.empty((N, P), dtype=torch.float32, device=out.device) if want_point_metric else None
    with _span('xr_kilotree_val_metrics', N * P, train=False):
        _lib.check(_lib.load().xr_kilotree_val_metrics(_ptr(out), pt, t_net, t_row, pp, p_net, p_row, N, P, int(quantile_index), _ptr(axis),
                                                       KILOTREE_METRICS[split_metric], _ptr(table), _ptr(pm), _stream()), 'xr_kilotree_val_metrics')
    return table, pm


# ------------------------------------------------------------------ the optimiser step over a work list, the log window (xrnerf_mi355_optim.h)
LOG_WINDOW_SLOTS = 16                    # XR_LOG_WINDOW_SLOTS


def optim_kernels_available():
    """the loaded library handle has xr_optim.hip's entry points (see gnr_kernels_available)"""
    return hasattr(_lib.load(), 'xr_adam_step_list')


def adam_list_capacity():
    """tensors per launch of adam_step_list (XR_ADAM_LIST_CAPACITY)"""
    return int(_lib.load().xr_adam_list_capacity())


def adam_step_list(ps, gs, ms, vs, step, lr=1e-2, beta1=0.9, beta2=0.99, eps=1e-15, weight_decay=1e-6, emas=None, ema_momentum=0.05,
                   grad_scale=1.0):
    """adam_step_multi's update for ANY number of tensors that share `step` and the constants: one launch per adam_list_capacity() tensors,
    small tensors sharing workgroups.  A tensor that is not 16-byte aligned (a view at an odd offset) is updated by 4-byte accesses."""
    k = len(ps)
    arr = lambda ts: (C.c_void_p * k)(*[t.data_ptr() if t is not None else None for t in ts])
    for t in list(ps) + list(gs) + list(ms) + list(vs) + [e for e in (emas or ()) if e is not None]:
        _ptr(t)     # validates device / contiguity
        if t.dtype != torch.float32:
            raise _lib.XrError('adam_step_list takes float32 tensors (got %s)' % t.dtype)
    ns = (C.c_size_t * k)(*[p.numel() for p in ps])
    with _span('xr_adam_step', sum(p.numel() for p in ps)):
        _lib.check(_lib.load().xr_adam_step_list(k, arr(ps), arr(gs), arr(ms), arr(vs), arr(emas) if emas else None, ns, int(step), lr, beta1,
                                                 beta2, eps, weight_decay, ema_momentum, float(grad_scale), _stream()), 'xr_adam_step_list')


def log_window_add(values, num_samples, window, first_slot=0):
    """window [2 * LOG_WINDOW_SLOTS] float64 on the device: window[s] += values[i] * num_samples, window[LOG_WINDOW_SLOTS + s] += num_samples,
    s = first_slot + i, for the one-element fp32 device tensors `values` (first_slot + len(values) <= LOG_WINDOW_SLOTS), one launch, nothing
    read back"""
    k = len(values)
    if not (0 <= first_slot and 1 <= k and first_slot + k <= LOG_WINDOW_SLOTS):
        raise _lib.XrError('log_window_add: slots %d .. %d of %d' % (first_slot, first_slot + k - 1, LOG_WINDOW_SLOTS))
    for t in values:
        _ptr(t)
        if t.dtype != torch.float32 or t.numel() != 1:
            raise _lib.XrError('log_window_add takes one-element float32 tensors (got %s %r)' % (t.dtype, tuple(t.shape)))
    if window.dtype != torch.float64 or window.numel() != 2 * LOG_WINDOW_SLOTS:
        raise _lib.XrError('log_window_add: window is [%d] float64' % (2 * LOG_WINDOW_SLOTS))
    arr = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in values])
    _ptr(window)
    _lib.check(_lib.load().xr_log_window_add(k, arr, int(num_samples), C.c_void_p(window.data_ptr() + 8 * first_slot), _stream()),
               'xr_log_window_add')


# ------------------------------------------------------------------------------------------ the instant-ngp loop's log sums (xr_ngprun.hip)
def ngprun_kernels_available():
    """the loaded library handle has xr_ngprun.hip's entry point (see gnr_kernels_available)"""
    return hasattr(_lib.load(), 'xr_ngp_log_add')


def ngp_log_add(loss_mse, n_rays, window, slot_loss, slot_psnr):
    """one training iteration's loss and psnr into a log window (LogWindow's layout), one launch, nothing read back:
    window[slot_loss] += loss_mse[0] * n_rays, window[slot_psnr] += -10 log10(loss_mse[1] / (3 n_rays)) * n_rays (in double), and n_rays
    into both slots' counts.  loss_mse: the two fp32 scalars of a training step (HashNerfNetwork._last['loss_mse'])."""
    _ptr(loss_mse)
    _ptr(window)
    if loss_mse.dtype != torch.float32 or loss_mse.numel() < 2:
        raise _lib.XrError('ngp_log_add: loss_mse is the step\'s two float32 scalars (got %s %r)' % (loss_mse.dtype, tuple(loss_mse.shape)))
    if window.dtype != torch.float64 or window.numel() != 2 * LOG_WINDOW_SLOTS:
        raise _lib.XrError('ngp_log_add: window is [%d] float64' % (2 * LOG_WINDOW_SLOTS))
    if not (1 <= int(n_rays) < (1 << 29) and 0 <= int(slot_loss) < LOG_WINDOW_SLOTS and 0 <= int(slot_psnr) < LOG_WINDOW_SLOTS):
        raise _lib.XrError('ngp_log_add: n_rays is 1 .. 2^29 - 1 and the slots lie inside the window (got %r, %r, %r)' % (n_rays, slot_loss, slot_psnr))
    _lib.check(_lib.load().xr_ngp_log_add(C.c_void_p(loss_mse.data_ptr()), int(n_rays), C.c_void_p(window.data_ptr()), int(slot_loss),
                                          int(slot_psnr), _stream()), 'xr_ngp_log_add')
