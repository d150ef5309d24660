// szn_upcell.h -- the geometry of one cell of a stride-S bilinear deconv, shared by the head files.
//
// upscore = fixed bilinear ConvTranspose2d(C, C, 2 S, stride S) (models.py:11-24,94): every pixel of the S x S cell (I, J) of the
// uncropped output blends the same four coarse vectors, its taps t = 0..3 in the order (I-1,J-1), (I-1,J), (I,J-1), (I,J) (zero
// outside the map), with its own four weights.  szn_head.hip (materialised upscore), szn_fused_head.hip and szn_ce_head.hip take
// the weights and the tap mappings from here; szn_seenmask_head.hip (a learned filter) only the combine and align256.
#pragma once
#include "szn_common.h"

// 1-D bilinear tap of get_upsampling_weight(k = 2 S): factor S, center S - 0.5 (models.py:13-20), in double
template <int S>
__device__ __forceinline__ double bil1d(int t) { return 1.0 - fabs((double)t - ((double)S - 0.5)) / (double)S; }

// the four weights of pixel (ty, tx) of a cell, in tap order: double products rounded to float (models.py:13-24)
template <int S>
__device__ __forceinline__ void cell_weights(int ty, int tx, float (&wt)[4]) {
    const double fy1 = bil1d<S>(ty), fy0 = bil1d<S>(ty + S), fx1 = bil1d<S>(tx), fx0 = bil1d<S>(tx + S);
    wt[0] = (float)(fy0 * fx0); wt[1] = (float)(fy0 * fx1); wt[2] = (float)(fy1 * fx0); wt[3] = (float)(fy1 * fx1);
}

// tap t of cell (I, J) is coarse position (tap_i(I, t), tap_j(J, t)) ...
__host__ __device__ __forceinline__ int tap_i(int I, int t) { return I - 1 + (t >> 1); }
__host__ __device__ __forceinline__ int tap_j(int J, int t) { return J - 1 + (t & 1); }
// ... and coarse position (i, j) is tap t of cell (tap_cell_I(i, t), tap_cell_J(j, t))
__host__ __device__ __forceinline__ int tap_cell_I(int i, int t) { return i + 1 - (t >> 1); }
__host__ __device__ __forceinline__ int tap_cell_J(int j, int t) { return j + 1 - (t & 1); }
// tap t of cell (I, J) of image b as a linear position of the (B, h, w) map, -1 where the tap lies outside it
__device__ __forceinline__ long tap_pos(int b, int h, int w, int I, int J, int t) {
    const int i = tap_i(I, t), j = tap_j(J, t);
    return (i >= 0 && i < h && j >= 0 && j < w) ? ((long)b * h + i) * w + j : -1;
}

// the four wave totals of a block (or any four partials), always in this order
template <typename T>
__host__ __device__ __forceinline__ T combine4(T a0, T a1, T a2, T a3) { return (a0 + a1) + (a2 + a3); }

// the embedding tables szn_fused_head_prepare writes to the head of a workspace: embT [E][KP] | en [KP] (0 -> 1) | ent [KP] floats,
// KP = the class count padded (K <= 256).  szn_fused_head.hip writes and reads them, szn_msinfer.hip reads them.
inline int kp_of(int K) { return K <= 24 ? 24 : (K <= 40 ? 40 : (K <= 64 ? 64 : (K + 63) / 64 * 64)); }
__host__ __device__ inline size_t prep_floats(int E, int KP) { return (size_t)E * KP + 2 * KP; }

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
