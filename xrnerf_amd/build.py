"""Builds xrnerf_amd/libxrnerf_mi355.so (gfx950 only) with hipcc, in-tree.

`python -m xrnerf_amd.build [--force]`.  hipcc cross-compiles without a GPU; the built .so
travels to the GPU box with the repo snapshot (it is git-ignored, not gpurun-ignored).
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OUT = os.path.join(HERE, 'libxrnerf_mi355.so')
OBJ = os.path.join(HERE, 'build')
COMMON = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-munsafe-fp-atomics', '-Wall',
          '-Wno-unused-variable', '-Wno-unused-but-set-variable']
# K1/K6/K11 make index decisions on `o + t*d`-style expressions: keep mul and add un-fused so they
# agree bit for bit with the CPU-compiled reference.
SOURCES = {
    'xr_raymarch.hip': ['-ffp-contract=off'],
    'xr_grid.hip': ['-ffp-contract=off'],
    # the hash-grid cell index is floor(x*scale+0.5): an index decision at scale up to 2047
    'xr_encode.hip': ['-ffp-contract=off'],
    # same index decisions and the same weight products as the gather
    # (-simplifycfg-sink-common=false: LLVM otherwise merges the `rank slot k` stores of different unrolled items into one
    # block with a dynamic slot index, which turns the per-thread rank registers of k_scatter_bin3 into scratch memory)
    'xr_scatter.hip': ['-ffp-contract=off', '-mllvm', '-simplifycfg-sink-common=false'],
    'xr_mlp.hip': [],
    'xr_misc.hip': ['-ffp-contract=off'],
    # Mip-NeRF stages: fp32 in the reference's operation order (lower + (upper-lower)*rand etc.)
    'xr_mip.hip': ['-ffp-contract=off'],
    # KiloNeRF: sample positions o + d*z and the cell index arithmetic must round like the reference's tensor ops
    # (the MLP's FMAs are explicit fmaf calls)
    'xr_kilo.hip': ['-ffp-contract=off'],
    # BungeeNeRF stages: fp32 in the reference's operation order, like xr_mip.hip
    'xr_bungee.hip': ['-ffp-contract=off'],
    # vanilla-NeRF stages (encode, training renderer, sample_pdf): fp32 in the reference's operation order as well
    'xr_vanilla.hip': ['-ffp-contract=off'],
    # Animatable-NeRF stages (closest vertex, selection, blend head, skinning, encode backward): the nearest-vertex decision is made on
    # d2 = (dx dx + dy dy) + dz dz, which must round like its fp32 tensor-op restatement
    'xr_aninerf.hip': ['-ffp-contract=off'],
    # NeuralBody stages (sparse structure, 3x3x3 sparse convolution, feature sampling): the sampling coordinates ((c + 1) / 2) (size - 1)
    # and the trilinear weights must round like torch's grid_sample, whose corner decision is a floorf of them
    'xr_neuralbody.hip': ['-ffp-contract=off'],
    # GNR body-shape queries (mesh grid, closest point, inside test, embedding): cell decisions are floors of (x - min) / step and the
    # closest-point solve ranks candidates with strict `<`, so every product and sum must round like the reference's un-fused fp32
    # (-simplifycfg-sink-common=false, as for xr_scatter.hip: sinking the arms of `if (pivot == 1) swap(a0, a1) else if ...` into one
    # block leaves a select between element ADDRESSES, which turns the solve's per-thread matrices into scratch memory)
    'xr_gnr.hip': ['-ffp-contract=off', '-mllvm', '-simplifycfg-sink-common=false'],
    # GNR renderer stages (visual hull, pixel-aligned gather, blend compositor): the hull's decision is a rounding to the nearest mask
    # pixel of a projected coordinate and the gather's corner a floorf of one, so the projection must round like its un-fused fp32
    # tensor-op restatement
    'xr_gnr_render.hip': ['-ffp-contract=off'],
    # GNR mesh reconstruction (grid hull, octree bookkeeping, iso-surface, Laplacian filter): a grid point is (i step + start) / f + c in
    # double, rounded once, and must equal numpy's bit for bit -- no fused multiply-add; the projection is the hull's
    'xr_gnr_recon.hip': ['-ffp-contract=off'],
    # GNR body depth maps (z-buffer rasteriser, vertex visibility): inside / outside is a comparison of A0 u + A3 v + A6 with -eps and the
    # stored coefficients and depths equal the reference's host build bit for bit -- no fused multiply-add
    'xr_gnr_raster.hip': ['-ffp-contract=off'],
    # GNR image encoder (hourglass convolutions on the fp32 MFMA, GroupNorm statistics, pool, bicubic upsampling): the only index
    # decision on a float is the bicubic tap, the floor of ONE product (scale * dst), which contraction cannot change: contraction stays on
    'xr_gnr_encoder.hip': [],
    # test-set evaluation (windowed moments, SSIM map, squared error, 8-bit image): double arithmetic whose bits the host build of the
    # same source (tests/hip_emu) reproduces -- no fused multiply-add
    'xr_eval.hip': ['-ffp-contract=off'],
    # scene data pipelines (the fused ray front end): un-fused fp32 in the reference's operation order -- o + t d, near (1 - t) + far t,
    # lower + (upper - lower) rand -- bit for bit the host tensor ops' results
    'xr_pipeline.hip': ['-ffp-contract=off'],
    # Mip-NeRF multiscale data (ray sampler over a camera table, box pyramid): the rays are double arithmetic in the reference's operation
    # order, rounded to fp32 once, and the pyramid is (((a + b) + c) + d) / 4 in fp32 -- bit for bit numpy's results, nothing fused
    'xr_multiscale.hip': ['-ffp-contract=off'],
    # ZJU-MoCap / H36M human data (prepared pictures, box silhouette lists, body-box ray sampler): the rays and the box test are double
    # arithmetic in the reference's operation order, rounded to fp32 once, the undistortion map is double whose floor picks the bilinear
    # taps, z_vals and pts are un-fused fp32 -- bit for bit numpy's and torch's results, nothing fused
    'xr_bodydata.hip': ['-ffp-contract=off'],
    # GeneBody data (crop box, OpenCV's nearest and 8-bit fixed-point cubic resize, a view in its role, camera rows): the crop rule and the
    # resize coordinates are double, the cubic coefficients, the adjusted K and the pixels are fp32, each written in explicitly rounded
    # single operations in the reference's order -- bit for bit numpy's and torch's results, nothing fused
    'xr_genebody.hip': ['-ffp-contract=off'],
    # BungeeNeRF data (a training item, a validation frame): the training rays are double arithmetic in numpy's operation order, rounded
    # to fp32 once, the frame's rays and every bound and z-value are un-fused fp32 in torch's -- bit for bit their results, nothing fused
    'xr_bungeedata.hip': ['-ffp-contract=off'],
    # KiloNeRF distillation's validation numbers (error means, quantile and equal-error split selects, saturation): the per-element errors
    # d d, |d| and |d| / (|t| + 0.1f) are fp32 in torch's operation order and rank the points -- bit for bit its results, nothing fused
    'xr_kilotree.hip': ['-ffp-contract=off'],
    # the optimiser step over a work list and the log window: adam1 / ema1 un-fused exactly as xr_misc.hip compiles them, so a tensor updated
    # by the list kernel is bit for bit what xr_adam_step_multi makes of it
    'xr_optim.hip': ['-ffp-contract=off'],
    # the instant-ngp loop's per-iteration log sums: double products and sums that the host build of the same source (tests/hip_emu) rounds
    # alike -- no fused multiply-add
    'xr_ngprun.hip': ['-ffp-contract=off'],
    'xr_gemm.hip': [],
    # host-side step executor (calls the entry points above in sequence)
    'xr_step.hip': [],
    # RCCL driven from native code (dlopen'ed on first use): the data-parallel loop's gradient exchange
    'xr_dist.hip': [],
}


def _hipcc():
    for c in ('/opt/rocm/bin/hipcc', 'hipcc'):
        if os.path.exists(c) or c == 'hipcc':
            return c


INCLUDE = os.path.join(HERE, '..', 'include')


def _headers():
    """every header a source may include (csrc/*.h, include/*.h), from the directory listings: a new one needs no entry anywhere"""
    return [os.path.join(d, f) for d in (CSRC, INCLUDE) for f in sorted(os.listdir(d)) if f.endswith('.h')]


def sources_hash():
    """sha256 over the library's sources (csrc/*.hip, csrc/*.h, the public headers, this recipe) in a fixed order"""
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.hip'))
    for f in files + _headers() + [os.path.abspath(__file__)]:
        h.update(os.path.basename(f).encode() + b'\0')
        with open(f, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


STAMP = OUT + '.stamp'          # "<sources hash> <library hash>" written by the build that produced OUT


def _file_hash(path):
    import hashlib
    with open(path, 'rb') as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def _stale(dst, srcs):
    if not os.path.exists(dst):
        return True
    t = os.path.getmtime(dst)
    return any(os.path.getmtime(s) > t for s in srcs)


def build(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    have_src = all(os.path.exists(os.path.join(CSRC, s)) for s in SOURCES)
    if not have_src:
        if os.path.exists(OUT):
            return OUT
        raise RuntimeError('xrnerf_amd/csrc sources missing and no prebuilt library')
    headers = _headers() + [os.path.abspath(__file__)]
    jobs = []
    for src, extra in SOURCES.items():
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace('.hip', '.o'))
        if force or _stale(o, [s] + headers):
            jobs.append((s, o, extra))

    def cc(job):
        s, o, extra = job
        cmd = [_hipcc()] + COMMON + extra + os.environ.get('XR_EXTRA_HIPCC_FLAGS', '').split() + ['-c', s, '-o', o]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError('hipcc failed: %s\n%s' % (' '.join(cmd), r.stdout + r.stderr))
        if verbose and (r.stdout or r.stderr):
            sys.stderr.write(r.stdout + r.stderr)
        return o

    if jobs:
        with ThreadPoolExecutor(len(jobs)) as ex:
            list(ex.map(cc, jobs))
    objs = [os.path.join(OBJ, s.replace('.hip', '.o')) for s in SOURCES]
    if force or jobs or _stale(OUT, objs):
        cmd = [_hipcc(), '--offload-arch=gfx950', '-shared', '-fPIC', '-o', OUT] + objs + ['-ldl']
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError('link failed: %s\n%s' % (' '.join(cmd), r.stdout + r.stderr))
        with open(STAMP, 'w') as fh:
            fh.write('%s %s\n' % (sources_hash(), _file_hash(OUT)))
        global BUILT_HERE
        BUILT_HERE = True
    return OUT


BUILT_HERE = False


def info():
    """where the loaded binary comes from: was it compiled in this process, and is it the build of exactly the sources beside it?"""
    out = {'library': os.path.basename(OUT), 'compiled_in_this_process': BUILT_HERE}
    try:
        src, lib = open(STAMP).read().split()
        out['library_sha16'] = _file_hash(OUT)[:16]
        out['binary_is_the_stamped_build'] = lib == _file_hash(OUT)
        out['sources_match_the_stamped_build'] = src == sources_hash() if os.path.isdir(CSRC) else None
        out['sources_sha16'] = src[:16]
    except (OSError, ValueError):
        out['stamp'] = 'missing'
    return out


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
