/* NeuralBody entry points of libxrnerf_mi355.so (xrnerf_amd/csrc/xr_neuralbody.hip): what `spconv` and the dense feature volumes are to
 * configs/neuralbody/nb_zjumocap_*.py -- the per-frame sparse structure (row lists, index volumes, neighbour tables), the 3x3x3 sparse
 * convolution with its two gradients, and trilinear sampling of the sparse rows through the index volumes with its row gradient.
 * A header of their own, bound by their own ctypes table (xrnerf_amd/_lib.py NEURALBODY_SIGNATURES), like xrnerf_mi355_aninerf.h.
 * Conventions of xrnerf_mi355.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw device
 * pointers (a few four-entry HOST arrays of device pointers / counts are marked), fp32, indices int32, contiguous unless a row stride
 * is given; the launch goes to `stream`.  A count of 0 is a no-op that returns 0 (xr_nb_build_rows: empty levels).  The same input gives the same bits.
 *
 * Geometry.  Level 0 is the volume out_sh = (D, H, W) of cells (z, y, x), each a multiple of 32, D H W <= XR_NB_MAX_CELLS; level l has
 * (D, H, W) >> l, l = 0..4.  A cell's linear index is (z H_l + y) W_l + x.  A level's rows are its active cells in ascending linear
 * index; its index volume holds the row of every cell, -1 where the cell is empty.  Semantics of the two convolutions (spconv is not
 * pinned here): tap k = (kz 3 + ky) 3 + kx;
 *   submanifold   out[p] = sum_k W[k] x[p + k - 1] over the active p, the active set unchanged;
 *   strided       out[o] = sum_k W[k] x[2 o - 1 + k], o active when any of its 27 inputs is, extent halved.
 * Weights are [Cout, 27, Cin] (spconv 2.x's [Cout, 3, 3, 3, Cin]); channels are 16, 32, 64 or 128. */
#ifndef XRNERF_MI355_NEURALBODY_H
#define XRNERF_MI355_NEURALBODY_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_NB_LEVELS 5
#define XR_NB_TAPS 27
#define XR_NB_MAX_CELLS (1u << 26)   /* level-0 cells: 6 x the 128 x 224 x 384 body at 5 mm voxels; its index volume is then 256 MiB */
#define XR_NB_TILE 64                /* rows of a convolution workgroup */
#define XR_NB_FEATURES 352           /* 32 + 64 + 128 + 128 sampled channels */

/* Layout of the two buffers xr_nb_build_rows fills, for V vertices in (D, H, W): out[0..4] = first int of level l's index volume
 * (cells_l ints each), out[5..9] = first int of level l's row list (capacity min(V 8^l, cells_l) ints each), out[10] / out[11] = total
 * ints of the volumes / the lists.  XR_EINVAL for a bad (D, H, W). */
int xr_nb_layout(uint32_t V, int D, int H, int W, uint64_t* out12);
size_t xr_nb_build_rows_workspace_bytes(int D, int H, int W);
/* The five row lists and index volumes of a frame from the integer voxel coordinates coord [V,3] (z, y, x; a vertex outside the volume
 * is left out and gets vert_row = -1).  vol / rows: laid out as xr_nb_layout says; vert_row [V] = level 0's row of each vertex (vertices
 * in one voxel share it); counts [5] = rows per level.  The volumes are cleared with ONE memset of all five (-1) and only the marked
 * cells are written afterwards: clearing the touched cells instead would need the previous frame's lists (the memset's time has
 * not been measured on its own: 50 to 100 MB per frame, i.e. tens of microseconds if it runs at memory bandwidth).  V = 0 gives five
 * empty levels: the volumes are cleared and counts zeroed, nothing else is written.  22 launches; the caller reads `counts` once. */
int xr_nb_build_rows(const int32_t* coord, uint32_t V, int D, int H, int W, int32_t* vol, int32_t* rows, int32_t* vert_row,
                     int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
/* nbr [n,27]: the row of cell p + k - 1 for every row p of a level with dims (D, H, W), -1 where empty or outside.  Its transpose
 * (the table of the input gradient) is itself with k -> 26 - k. */
int xr_nb_subm_table(const int32_t* vol, const int32_t* rows, uint32_t n, int D, int H, int W, int32_t* nbr, void* stream);
/* strided step from a level with dims (D, H, W) to the next: out_tab [n_out,27] = input row at 2 o - 1 + k, in_tab [n_in,27] = the
 * output row whose tap k reads input i ((i + 1 - k) / 2 per axis where that is an integer inside the output), -1 otherwise. */
int xr_nb_down_tables(const int32_t* vol_in, const int32_t* rows_in, uint32_t n_in, const int32_t* vol_out, const int32_t* rows_out,
                      uint32_t n_out, int D, int H, int W, int32_t* out_tab, int32_t* in_tab, void* stream);
/* out [n, cout] = sum_k x[tab[r, k'], :] Wk, rows with tab = -1 reading as 0.  fp32 throughout (v_mfma_f32_32x32x2_f32: exact products),
 * summed in three levels of fixed order: an fma chain over each slice of 32 channels, the slices of a tap, the taps ascending.
 * x [*, cin]; w is the layer's weight tensor:
 *   transposed = 0: w [cout, 27, cin], Wk[c][j] = w[j, k, c]   (forward)
 *   transposed = 1: w [cin, 27, cout], Wk[c][j] = w[c, k, j]   (input gradient: x = dL/dout, tab = the input-stationary table)
 *   flip: k' = 26 - k instead of k (the submanifold input gradient on the forward table).
 * x, w, out 16-byte aligned; cin, cout in {16, 32, 64, 128}.  One launch. */
int xr_nb_conv(const float* x, const int32_t* tab, const float* w, uint32_t n, int cin, int cout, int transposed, int flip, float* out,
               void* stream);
size_t xr_nb_conv_weight_grad_workspace_bytes(uint32_t n, int cin, int cout);
/* dW [cout, 27, cin]: dW[o, k, c] = sum_r g[r, o] x[tab[r, k], c] over the n output rows (tab: the forward, output-stationary table).
 * Row chunks are summed into partial slabs in the workspace, which a second launch folds in chunk order: no atomics. */
int xr_nb_conv_weight_grad(const float* x, const int32_t* tab, const float* g, uint32_t n, int cin, int cout, float* dw, void* workspace,
                           size_t workspace_bytes, void* stream);
/* F.grid_sample(volume_l, grid, padding_mode='zeros', align_corners=True) of levels 1..4 for n world points pts [n,3]:
 *   q_j = sum_k (p_k - T_k) R_kj (k ascending, un-fused), c = (q - min_xyz) / voxel / (W, H, D) * 2 - 1, the same c for every level,
 *   f = ((c + 1) / 2) (size_l - 1), floorf, weights and corner order of torch's trilinear sampler, corners outside or empty read 0.
 * R [9], T [3], min_xyz [3] on the device.  vols / feats: HOST arrays of four device pointers (levels 1..4: index volume, rows
 * [n_l, 32 | 64 | 128 | 128]); out row i = out + i ld, 352 floats written (ld >= 352, ld % 4 == 0, out 16-byte aligned). */
int xr_nb_sample_forward(const float* pts, const float* R, const float* T, const float* min_xyz, float voxel, int D, int H, int W,
                         const void* const* vols, const void* const* feats, uint32_t n, float* out, uint32_t ld, void* stream);
size_t xr_nb_sample_backward_workspace_bytes(const uint32_t* n_rows);
/* the gradient of the four levels' rows from grad (row i = grad + i ld, 352 floats read): grad_feats = HOST array of four device
 * pointers [n_rows[l], C_l], n_rows = HOST array of the four row counts.  Summed in 64-bit fixed point (integer adds commute, so the
 * bits repeat): with gmax = max |grad| < 2^e and n <= 2^b every contribution w g is rounded to a multiple of 2^(b + e - 61), so a row
 * element's error is at most (its contributions) x 2^(b - 61) gmax before the final rounding to fp32.  Points get no gradient.
 * A NaN or infinite gradient entry contributes nothing.  Five launches (clear, max |grad|, the scale, scatter, convert). */
int xr_nb_sample_backward(const float* pts, const float* R, const float* T, const float* min_xyz, float voxel, int D, int H, int W,
                          const void* const* vols, const uint32_t* n_rows, const float* grad, uint32_t ld, uint32_t n,
                          void* const* grad_feats, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
