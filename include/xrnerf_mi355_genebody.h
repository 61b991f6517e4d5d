/* GeneBody data: the crop-and-resize frame preparation of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_genebody.hip) -- what the reference's
 * GeneBodyDataset.get_image (datasets/genebody_dataset.py:184-374) does on the host for every view of every item, split into what depends
 * on the view alone (crop box, resized picture, mask byte and depth: made once, kept on the device) and what depends on the view's role in
 * an item.  A header of its own, bound by its own ctypes table (xrnerf_amd/_lib.py GENEBODY_SIGNATURES).
 * Conventions of xrnerf_mi355_pipeline.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw
 * device pointers unless a parameter says "host"; the launches go to `stream`.  XR_EINVAL launches nothing and leaves every output
 * untouched.  The only atomics are int32 atomicMin / atomicMax (order-free): the same input gives the same bits.
 * The two resizes restate OpenCV's INTER_NEAREST and 8-bit INTER_CUBIC from memory (tests/genebody_restatement.py is the specification);
 * their equality with OpenCV itself is unverified. */
#ifndef XRNERF_MI355_GENEBODY_H
#define XRNERF_MI355_GENEBODY_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_GB_MAX_VIEWS 64u        /* views of one launch (an evaluation item of the config has 4 + 48) */
#define XR_GB_MAX_DIST 8u          /* distortion coefficients carried through persps */
#define XR_GB_MAX_SIDE 32768u      /* picture height / width and S */

/* The crop box of n raw masks, ONE launch, one workgroup per mask.
 *   masks   device bytes; mask i is [h_i, w_i] uint8 at byte offset table[3 i]
 *   table   HOST, n x 3 int64: offset, h, w
 *   boxes   device [n, 4] int32: top, left, bottom, right
 * min / max row and column of mask != 0, then GeneBodyDataset.image_cropping's rule with its quirks kept: the 10 % padding in double,
 * truncated; `left` padded by the box HEIGHT; the square-up with three placement branches per axis (clamped low, clamped high, centred);
 * an empty mask gives (0, 0, h, w), which is not square.  A box may leave the picture (a side beyond the other dimension): the caller checks.
 * Refused: a null pointer; n of 0 or above XR_GB_MAX_VIEWS; a negative offset; h or w of 0 or above XR_GB_MAX_SIDE. */
int xr_gb_crop_box(const uint8_t* masks, const int64_t* table, uint32_t n, int32_t* boxes, void* stream);

/* The three resized planes of n views, ONE launch over (S x S tiles, views); the crop box is read from device memory.
 *   imgs, masks, depths   device; view i: picture [h, w, 3] uint8 at imgs + table[5 i], mask [h, w] uint8 at masks + table[5 i + 1],
 *                         depth [h, w] uint16 at depths + table[5 i + 2] ELEMENTS, or no depth when that entry is negative
 *   table   HOST, n x 5 int64: the three offsets, h, w
 *   rgb [n, S, S, 3] uint8, m8 [n, S, S] uint8, depth [n, S, S] float (rows of views without depth are left untouched; may be NULL when
 *   no view has depth)
 * Mask and depth: INTER_NEAREST, sx = min(floor(x scale), n - 1), scale = 1 / (S / (double) n); depth is uint16 / 1000 in fp32.
 * Picture: 8-bit INTER_CUBIC in fixed point: fx = (float)((x + 0.5) scale - 0.5), sx = floor(fx), f = fx - sx; with A = -0.75f and
 * t = f + 1, g = 1 - f, all fp32 and un-fused: c0 = ((A t + 3.75) t - 6) t + 3, c1 = ((1.25 f - 2.25) f) f + 1, c2 = ((1.25 g - 2.25) g) g + 1,
 * c3 = ((1 - c0) - c1) - c2; each becomes short(rint(c 2048)); taps sx - 1 .. sx + 2 clamped to the crop; the horizontal int32 sum is not
 * shifted, the vertical sum of those is (v + 2^21) >> 22 saturated to 0 .. 255.
 * A box that leaves the picture is clipped to it (nothing is read out of bounds); an empty clipped box writes zeros.
 * Refused: a null pointer; n of 0 or above XR_GB_MAX_VIEWS; S of 0 or above XR_GB_MAX_SIDE; sizes as above; depth offsets without depths / depth. */
int xr_gb_resize(const uint8_t* imgs, const uint8_t* masks, const uint16_t* depths, const int64_t* table, uint32_t n, const int32_t* boxes, uint32_t S,
                 uint8_t* rgb, uint8_t* m8, float* depth, void* stream);

/* One item's V views in their roles, ONE launch over (S S pixels, V) after two memsets of `acc`.
 *   rgb, m8   HOST arrays of V device pointers ([S,S,3] uint8, [S,S] uint8);  depth  HOST array of num_views device pointers ([S,S] float)
 *             or NULL (no body depth)
 *   img [V,3,S,S], mask [num_views,1,S,S], smpl_depth [num_views,S,S] (NULL without depth) floats
 *   acc [2,V,2] int32: min (row, col) then max (row, col) of every view's final mask; an empty mask leaves 0x7f7f7f7f / -1
 * mask = m8 > 128, OR'ed with depth > 0 for the first num_views views.  pixel = byte / 255 (fp32); the first num_views views are
 * (x - 0.5) / 0.5, the others x mask + (1 - mask) with white_bkgd; then mask x pixel.
 * Refused: a null pointer; V of 0 or above XR_GB_MAX_VIEWS; num_views above V; S of 0 or above XR_GB_MAX_SIDE; smpl_depth without depth or the reverse. */
int xr_gb_assemble(const void* const* rgb, const void* const* m8, const void* const* depth, uint32_t V, uint32_t num_views, uint32_t S, int white_bkgd,
                   float* img, float* mask, float* smpl_depth, int32_t* acc, void* stream);

/* One item's camera rows and scalars, ONE launch, one workgroup per view over the N body vertices; workgroup 0 also makes the item's values.
 *   verts [N,3], K [V,3,3] (as stored), D [V,nd], w2c [V,4,4]: device floats;  crop: HOST array of V device pointers to int32[4];
 *   acc: xr_gb_assemble's
 *   persps [V, 4 + nd + 2] floats: fx, fy, cx, cy of the adjusted K, D, near, far
 *   vboxes [V,4] int32: r0, c0, r1, c1 of the final mask, (0, 0, S, S) when it is empty
 *   sf_views [num_views], bbox [4], spatial_freq [1] doubles;  center [3] floats
 * Adjusted K, exact fp32: K[0][2] -= left, K[1][2] -= top, row 0 times (float)(S / (double)(right - left)), row 1 likewise.
 * Camera coordinates in fp32, ((v0 R0 + v1 R1) + v2 R2) + t; near / far = zmin -+ (zmax - zmin) / 2.  spatial_freq of an input view:
 * 180 / (side / (float)(pmax - pmin) * (float)(vmax - vmin)) / 0.5 in double over the longer side of the view's mask box (height only
 * when strictly longer), p = projection through the adjusted K divided by (z + 1e-8f).  bbox from views num_views .. V - 1:
 * b = (int)(max |box - S / 2| x [1, sqrt 2]), (S/2 - b0, S/2 + b0, S/2 - b1, S/2 + b1) clipped to [0, S].  center = (max + min) / 2.
 * Refused: a null pointer; N of 0; V of 0 or above XR_GB_MAX_VIEWS; num_views of 0 or not below V; nd above XR_GB_MAX_DIST; S as above. */
int xr_gb_calib(const float* verts, uint32_t N, const float* K, const float* D, uint32_t nd, const float* w2c, const void* const* crop, const int32_t* acc,
                uint32_t V, uint32_t num_views, uint32_t S, float* persps, int32_t* vboxes, double* sf_views, double* bbox, double* spatial_freq,
                float* center, void* stream);

#ifdef __cplusplus
}
#endif
#endif
