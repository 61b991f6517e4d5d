// Scene data pipelines for gfx950: the ray front end of a training item or a test frame in one launch.  The
// reference runs it on the host, per item: GetRays over the whole image, np.random.choice, three gathers, about thirty small tensor
// ops, collate and a copy to the device.  Here an item only touches the pixels it selected:
//   k_pipe_ray_front   thread = one (ray, sample) item of the flat R x max(S, 1) range, 256-thread workgroups.  The chain is a map: no
//                      scan, no atomics, no LDS, no cross-lane traffic.  Every thread recomputes its ray's few dozen flops (the pose is
//                      twelve uniform loads) and z[k-1], z[k], z[k+1] straight from the linspace formula, so no lane needs a neighbour;
//                      the thread with k == 0 writes the per-ray outputs.  All index arithmetic is size_t.
// Reference lines (xrnerf/datasets/pipelines/):
//   create.py:217-235    GetRays: pixel grid, dirs, rays_d = sum(dirs * c2w[:3,:3], -1), rays_o
//   create.py:237-243    include_radius: dx between vertically adjacent rays, the last row takes dx[-2:-1], * 2 / sqrt(12)
//   augment.py:63-75     SelectRays: the gathers        transforms.py:73-81  FlattenRays        create.py:100-107  BatchSample
//   create.py:444-446    GetViewdirs                      transforms.py:32-47  ndc_rays            create.py:475-478  GetBounds
//   create.py:510-528    GetZvals (and randomized=True)   augment.py:276-282   PerturbZvals        create.py:595-596  GetPts
// Built with -ffp-contract=off: nothing is fused, and the host build of this file (tests/hip_emu) produces the same bits.
#include "xr_common.h"
#include "xr_mip_math.h"      // xr_torch_linspace / xr_mip_zval: GetZvals' t and z, the code sample_pdf's u = NULL runs
#include "../../include/xrnerf_mi355_pipeline.h"

#define PIPE_BLOCK 256

struct PipeArgs {
    const float *c2w, *image, *table, *t_rand;
    const int32_t* sel;
    float fx, fy, cx, cy, ndc_w, ndc_h, ndc_near, near, far, radius_div;
    uint32_t H, W, C, S, Sd;
    uint64_t pix0, R;
    int with_viewdirs, ndc, with_radii, lindisp;
    float *rays_o, *rays_d, *viewdirs, *radii, *near_out, *far_out, *z_vals, *pts, *target_s;
};

// rays_d of pixel (h, w): create.py:223-230, the three products added in index order
static __device__ inline void pipe_dir(const PipeArgs& a, const float* c, uint32_t h, uint32_t w, float d[3]) {
    const float dx = ((float)w - a.cx) / a.fx, dy = -((float)h - a.cy) / a.fy, dz = -1.f;
    for (int r = 0; r < 3; ++r) d[r] = (dx * c[4 * r] + dy * c[4 * r + 1]) + dz * c[4 * r + 2];
}

static __global__ void __launch_bounds__(PIPE_BLOCK) k_pipe_ray_front(PipeArgs a) {
    const size_t item = (size_t)blockIdx.x * PIPE_BLOCK + threadIdx.x;
    if (item >= (size_t)a.R * a.Sd) return;
    const size_t r = item / a.Sd;
    const uint32_t k = (uint32_t)(item - r * a.Sd);
    const bool first = k == 0;
    float o[3], d[3];
    bool valid = true;
    if (a.table) {
        const float* row = a.table + r * 9;
        for (int c = 0; c < 3; ++c) { o[c] = row[c]; d[c] = row[3 + c]; }
        if (first && a.target_s)
            for (int c = 0; c < 3; ++c) a.target_s[r * 3 + c] = row[6 + c];
    } else {
        size_t pix = a.pix0 + r;
        if (a.sel) {
            const int32_t s = a.sel[r];
            valid = s >= 0 && (size_t)s < (size_t)a.H * a.W;
            pix = valid ? (size_t)s : 0;
        }
        const uint32_t h = (uint32_t)(pix / a.W), w = (uint32_t)(pix - (size_t)h * a.W);
        float c[12];
        for (int i = 0; i < 12; ++i) c[i] = a.c2w[i];
        pipe_dir(a, c, h, w, d);
        for (int i = 0; i < 3; ++i) o[i] = c[4 * i + 3];
        if (first && a.radii) {                                    // create.py:239-243
            const uint32_t hp = h + 1 < a.H ? h : a.H - 3;          // torch.cat([dx, dx[-2:-1]]): the last row repeats dx[H - 3]
            float da[3], db[3], sq[3];
            pipe_dir(a, c, hp, w, da);
            pipe_dir(a, c, hp + 1, w, db);
            for (int i = 0; i < 3; ++i) { const float e = da[i] - db[i]; sq[i] = e * e; }
            const float dx = sqrtf((sq[0] + sq[1]) + sq[2]);
            a.radii[r] = valid ? (dx * 2.f) / a.radius_div : NAN;
        }
        if (first && a.target_s && a.image)
            for (uint32_t ch = 0; ch < a.C; ++ch) a.target_s[r * a.C + ch] = valid ? a.image[pix * a.C + ch] : NAN;
        if (!valid)
            for (int i = 0; i < 3; ++i) o[i] = d[i] = NAN;
    }
    if (first && a.viewdirs) {                                      // create.py:445; torch.norm accumulates acc = fma(x, x, acc) in index order
        const float n = sqrtf(fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0])));
        for (int i = 0; i < 3; ++i) a.viewdirs[r * 3 + i] = d[i] / n;
    }
    if (a.ndc) {                                                    // transforms.py:34-46
        const float t = -(a.ndc_near + o[2]) / d[2];
        float on[3];
        for (int i = 0; i < 3; ++i) on[i] = o[i] + t * d[i];
        const float two_near = 2.f * a.ndc_near;
        o[0] = a.ndc_w * on[0] / on[2];
        o[1] = a.ndc_h * on[1] / on[2];
        o[2] = 1.f + two_near / on[2];
        const float d0 = a.ndc_w * (d[0] / d[2] - on[0] / on[2]);
        const float d1 = a.ndc_h * (d[1] / d[2] - on[1] / on[2]);
        const float d2 = -two_near / on[2];
        d[0] = d0; d[1] = d1; d[2] = d2;
    }
    if (first) {
        for (int i = 0; i < 3; ++i) {
            if (a.rays_o) a.rays_o[r * 3 + i] = o[i];
            if (a.rays_d) a.rays_d[r * 3 + i] = d[i];
        }
        if (a.near_out) a.near_out[r] = a.near;
        if (a.far_out) a.far_out[r] = a.far;
    }
    if (a.S == 0 || !(a.z_vals || a.pts)) return;
    float z = xr_mip_zval(a.near, a.far, a.S, k, a.lindisp);         // create.py:510-516
    if (a.t_rand) {                                                 // augment.py:278-282, create.py:519-525
        const float lower = k == 0 ? z : .5f * (z + xr_mip_zval(a.near, a.far, a.S, k - 1, a.lindisp));
        const float upper = k + 1 == a.S ? z : .5f * (xr_mip_zval(a.near, a.far, a.S, k + 1, a.lindisp) + z);
        z = lower + (upper - lower) * a.t_rand[item];
    }
    if (a.z_vals) a.z_vals[item] = z;
    if (a.pts)                                                      // create.py:595-596
        for (int i = 0; i < 3; ++i) a.pts[item * 3 + i] = o[i] + d[i] * z;
}

extern "C" int xr_pipe_ray_front(const float* c2w, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W, const int32_t* sel, uint64_t pix0,
                                 uint64_t R, const float* image, uint32_t C, const float* table, int with_viewdirs, int ndc, int with_radii,
                                 float ndc_w, float ndc_h, float ndc_near, float near, float far, uint32_t S, int lindisp, const float* t_rand,
                                 float* rays_o, float* rays_d, float* viewdirs, float* radii, float* near_out, float* far_out, float* z_vals,
                                 float* pts, float* target_s, void* stream) {
    XR_REQUIRE((c2w != nullptr) != (table != nullptr), "exactly one of c2w / table");
    if (c2w) {
        XR_REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W <= 0x7fffffffull, "H, W >= 1 and H W within int32");
        XR_REQUIRE(fx != 0.f && fy != 0.f && fx - fx == 0.f && fy - fy == 0.f && cx - cx == 0.f && cy - cy == 0.f, "finite intrinsics, fx and fy not 0");
        XR_REQUIRE(sel || (pix0 <= (uint64_t)H * W && R <= (uint64_t)H * W - pix0), "pix0 + R exceeds H W");
        XR_REQUIRE(!with_radii || H >= 3, "radii need H >= 3");
        XR_REQUIRE(!image || (C >= 1 && C <= XR_PIPE_MAX_CHANNELS), "1 .. XR_PIPE_MAX_CHANNELS image channels");
    } else {
        XR_REQUIRE(!sel && !image && !with_radii && !radii, "a table carries its own selection and targets and has no radii");
    }
    XR_REQUIRE((with_radii != 0) == (radii != nullptr), "with_radii and the radii output go together");
    XR_REQUIRE((with_viewdirs != 0) == (viewdirs != nullptr), "with_viewdirs and the viewdirs output go together");
    XR_REQUIRE(!ndc || (H >= 1 && W >= 1), "ndc needs H and W");
    XR_REQUIRE(S >= 1 || (!z_vals && !pts && !t_rand), "z_vals, pts and t_rand need S >= 1");
    const uint32_t Sd = S ? S : 1u;
    XR_REQUIRE(R <= (0x7fffffffull * PIPE_BLOCK) / Sd, "more than 2^31 - 1 workgroups");
    if (R == 0) return 0;
    PipeArgs a;
    a.c2w = c2w; a.image = image; a.table = table; a.t_rand = t_rand; a.sel = sel;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.ndc_w = ndc_w; a.ndc_h = ndc_h; a.ndc_near = ndc_near; a.near = near; a.far = far;
    a.radius_div = sqrtf(12.f);                                     // torch.sqrt(torch.tensor(12)): fp32
    a.H = H; a.W = W; a.C = C; a.S = S; a.Sd = Sd; a.pix0 = pix0; a.R = R;
    a.with_viewdirs = with_viewdirs; a.ndc = ndc; a.with_radii = with_radii; a.lindisp = lindisp;
    a.rays_o = rays_o; a.rays_d = rays_d; a.viewdirs = viewdirs; a.radii = radii; a.near_out = near_out; a.far_out = far_out;
    a.z_vals = z_vals; a.pts = pts; a.target_s = target_s;
    const uint32_t blocks = (uint32_t)((R * Sd + PIPE_BLOCK - 1) / PIPE_BLOCK);
    hipLaunchKernelGGL(k_pipe_ray_front, dim3(blocks), dim3(PIPE_BLOCK), 0, (hipStream_t)stream, a);
    XR_LAUNCH_CHECK();
    return 0;
}
