// szn_fused_head.hip -- the SZN head evaluated from the 1/32-resolution projection map without ever
// materialising the (B,E,H,W) score: bilinear x32 upsample + crop (models.py:146-147), cosine loss
// (utils.py:75-102), nearest-class-embedding argmax (utils.py:159-185) and the gradient back to the
// coarse map, per 32x32 output cell.  The same kernels are instantiated for stride 8 (8x8 cells of the 1/8 map: the last
// stage of the FCN8s skip head, upscore8 + crop 31).  The cell geometry (bilinear weights, tap <-> position) is szn_upcell.h's.
//
// Inside one cell (Y / S, X / S fixed) every pixel's score vector is a blend of the SAME four coarse
// vectors C_t with per-pixel bilinear weights w_t, so
//     s . e_k = sum_t w_t (C_t . e_k)            -> per-cell table G[4][K]
//     |s|^2   = sum_{t,t'} w_t w_t' (C_t . C_t') -> per-cell Gram matrix Q[4][4]
// and the gradient wrt the coarse vectors collapses to
//     dC_t = -sum_k A[t][k] e_k + sum_t' Bm[t][t'] C_t',  A[t][k] = sum_{px: label k} w_t / (|s||e_k|),
//                                                         Bm[t][t'] = sum_px w_t w_t' cos / |s|^2
// (all scaled by 1/(B N_b)).  HBM traffic: labels in, prediction out (16 B/px) + the coarse map.
//
// Kernels, in launch order (all reductions are fixed-order: bit-reproducible):
//   fh_prep_kernel       the class matrix transposed + its norms, to the head of the workspace (szn_fused_head_prepare, or every call)
//   fh_cell_kernel       stride 32: one block per (image, cell) builds G, Q from the four tap vectors, walks its 1024 pixels
//   fh_tables_kernel     stride 8: per-POSITION tables D, N, from which ...
//   fh_cell_tab_kernel   ... one wave per 8x8 cell looks its G, Q up, then walks its 64 pixels
//   fh_image_sums_kernel per-image sums of the cells' loss partials -> stats;  fh_finalize_kernel: the images -> loss
//   fh_gather_kernel     one block per coarse position sums the <= 4 cells that use it as a tap and writes dcoarse
//   calib_cell_kernel / calib_cell_tab_kernel / calib_hist_kernel   szn_calib_head (calibrated stacking): the cell kernels' G and Q (fh_load_taps,
//                        fh_build_GQ, fh_lookup_GQ), two running bests per pixel (fh_two_best), crossing tables, prefix sums -> hist
//                        (calib_count and calib_hist_kernel live in szn_calib.h, shared with szn_conse_head.hip)
//   sweep_cell_kernel / sweep_cell_tab_kernel   szn_seen_sweep_head (seen-mask threshold sweep): the calibrated kernels with the grouped
//                        head's two answers per pixel (fh_group_bests) and the seen-mask margin as the switch; then calib_hist_kernel
//   gate_cell_kernel / gate_cell_tab_kernel   szn_soft_gate_head (soft seen/unseen gating): the sweep kernels with the true in-group bests and
//                        an online log-sum-exp per group (fh_gate_bests); the switch is margin - weight * (l_S - l_U); then calib_hist_kernel
//   hub_stats_cell_kernel / hub_stats_cell_tab_kernel / hub_table_kernel   szn_hub_stats (hubness correction): the cells' G and Q, exact int64
//                        moments of every class's similarity per image, then the (scale, shift) table
//   hub_cell_kernel / hub_cell_tab_kernel   szn_hub_head: the calibrated kernels on fmaf(sim, scale, -shift); then calib_hist_kernel
//   pseudo_cell_kernel / pseudo_cell_tab_kernel / pseudo_thr_kernel / pseudo_relabel_kernel   szn_pseudo_head (self-training): the same G, Q
//                        and fh_two_best on the pixels labelled cand_label, a per-class confidence histogram, thresholds, the relabelled target
//   ohem_cell_kernel / ohem_cell_tab_kernel / ohem_cut_kernel / ohem_relabel_kernel   szn_ohem_head (hard-pixel mining), in launch order: the
//                        same G and Q, fh_pixel's own-class cosine of every labelled pixel, a per-image histogram counted in LDS, the cut
//                        (a prefix scan), the target with the easy pixels dropped
//   sce_cell_kernel / sce_cell_tab_kernel   szn_fused_simce_head (similarity cross-entropy): the same G and Q, a softmax over the classes per
//                        pixel (sce_pixel) and a dense A through a per-wave LDS tile (sce_dense_A); sums, finalize and gather as above
//                        The same two kernels over RankArgs: szn_fused_rank_head (hinge ranking loss), one walk over the classes per pixel
//                        and over BiasArgs: szn_fused_simce_bias_head (sim_ce plus the unseen-bias term on hidden pixels)
// Both cell kernels run the same per-pixel body (fh_pixel) and the same label loop (fh_scatter_A), and write per cell: pred, the
// loss partial, A and Bm.
//
// MSE variant (template flag MSE; szn_fused_mse_head, utils.py:50-73): L_b = sum_px |s - e_lbl|^2 / N_b.  Prediction, G, Q and the
// grouped modes are the cosine head's, bit for bit.  The gradient has the same shape with per-pixel coefficients 1,
//     dC_t = 2/(B N_b) ( sum_u Bm[t][u] C_u - sum_k A[t][k] e_k ),   A[t][k] = sum_{px: label k} w_t,  Bm[t][u] = sum_{valid px} w_t w_u,
// so fh_gather_kernel serves both (numerator 2 instead of 1).  The per-pixel LOSS is not formed from G and Q as
// |s|^2 - 2 s.e + |e|^2: that cancels once the net has learnt something (2e-2 of a cell's loss at C = e + 1e-3 |e| noise in fp32).
// Layout chosen instead: the bilinear weights of a pixel sum to exactly 1 (multiples of 1/(2S)^2), so s - e_k = sum_t w_t (C_t - e_k) and
//     |s - e_k|^2 = sum_{t,u} w_t w_u P_k[t][u],   P_k[t][u] = (C_t - e_k) . (C_u - e_k)      (10 distinct dot products of length E)
// built from the vectors (fh_pk: differences first, then products: nothing large is subtracted) only for the classes that occur in
// the cell; missing border taps are C_t = 0.  Stride 32: a first pass over the block's labels marks the classes present in
// LDS, the four waves share the present classes round-robin and store P_k in LDS [KP][10] (each class built once per cell).
// Stride 8: one wave owns the cell and already visits its labels class by class for A, so P_k lives in registers for the duration
// of that class's turn, read from the coarse vectors themselves (the per-position tables D, N would only give the cancelling form).
#include "szn_upcell.h"
#include "szn_calib.h"

namespace {

// index of the pair (t, u), t <= u, among the 10 distinct entries of a symmetric 4 x 4 matrix
__device__ __forceinline__ constexpr int sym10(int t, int u) {
    return t <= u ? (t * 4 - t * (t - 1) / 2) + (u - t) : (u * 4 - u * (u - 1) / 2) + (t - u);
}

// |s - e_k|^2 of one pixel from the cell's P_k (MSE variant): fixed-order chain over the 16 (t, u) pairs
__device__ __forceinline__ float mse_px(const float (&wt)[4], const float* P) {
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) l = fmaf(wt[t] * wt[u], P[sym10(t, u)], l);
    return l;
}

// P_k of one class (row ek of the class matrix) by one wave: 64 strided partial chains + xor butterfly; tap(t, c) is C_t[c]
template <typename Tap>
__device__ __forceinline__ void fh_pk(const float* __restrict__ ek, int E, int lane, Tap tap, float (&p)[10]) {
#pragma unroll
    for (int v = 0; v < 10; ++v) p[v] = 0.f;
    for (int c = lane; c < E; c += 64) {
        const float e = ek[c];
        float d[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) d[t] = tap(t, c) - e;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int u = t; u < 4; ++u) p[sym10(t, u)] = fmaf(d[t], d[u], p[sym10(t, u)]);
    }
#pragma unroll
    for (int v = 0; v < 10; ++v) p[v] = wave_sum(p[v]);
}

struct FhArgs {
    const float* coarse; const float* embed; const int64_t* target;
    int64_t* pred; float* ws_f; double* part;
    int B, h, w, E, ldc, c0, H, W, crop, K, KP;
    const int64_t* gmap; int gmode; ClassBits unseen;      // grouped class assignment (gmode 1 | 2), see fh_argmax
};

// |s|^2 of one pixel from the cell's Gram matrix, and its similarity to class k from the cell's G: the arithmetic every head shares
__device__ __forceinline__ float fh_ss(const float (&wt)[4], const float* Q) {
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) ss = fmaf(wt[t] * wt[u], Q[t * 4 + u], ss);
    return ss;
}
template <int KP>
__device__ __forceinline__ float fh_sim(const float (&wt)[4], const float* G, float sn, const float* __restrict__ en, int k) {
    float d = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) d = fmaf(wt[t], G[t * KP + k], d);
    return d / (sn * en[k]);
}

// Nearest class embedding of one pixel: ascending classes, strictly larger replaces: the first index wins.
// GROUPED (szn_fused_head_grouped; trainer_fcn.py:123-147, utils.py:188-204): the pixel competes among the classes
// of ITS group only -- the unseen classes when it takes the unseen group, the others otherwise -- and every class outside that group
// scores 0 / (sn * 1), exactly what a zeroed row of the seen-only / unseen-only matrix scores (trainer_fcn.py:56-64): it still
// competes, and a zero-norm pixel gives NaN for every class like szn_embed_argmax_k mode 1.  The group bits stay in the kernel
// arguments: k is wave-uniform, so the word select and the bit test are scalar instructions next to the per-class loop, no LDS
// read.  The plain instantiation does not touch them.
template <int KP, bool GROUPED>
__device__ __forceinline__ int fh_argmax(const FhArgs& a, const float (&wt)[4], const float* G, float sn,
                                         const float* __restrict__ en, size_t pix, long lbl) {
    bool take_unseen = false;
    if constexpr (GROUPED) take_unseen = (a.gmode == 1) ? (a.gmap[pix] == 0) : in_set(a.unseen, lbl);
    const float zero_sim = 0.f / (sn * 1.f);
    int best = 0;
    float bv = 0.f;
    for (int k = 0; k < a.K; ++k) {
        bool in_group = true;
        if constexpr (GROUPED) in_group = (bool)((class_word(a.unseen, k >> 6) >> (k & 63)) & 1ull) == take_unseen;
        float sim = zero_sim;
        if (in_group) sim = fh_sim<KP>(wt, G, sn, en, k);
        if (k == 0 || sim > bv) { bv = sim; best = k; }
    }
    return best;
}

// The same trip through the classes with two running bests (szn_calib_head): ia / va over the classes outside `unseen`, ib / vb over
// its members, each the first index holding its group's maximum.  The group bit is wave-uniform like in_group above: a scalar select,
// no divergence, no second pass.  Both groups are non-empty (checked on the host).
// HUB (szn_hub_head): the value that enters the running bests is fmaf(sim, scale_k, -shift_k).  T [K] in LDS holds (en[k], scale_k, shift_k, 0)
// of the pixel's image (hub_stage): one 16-byte LDS read per class next to G's, in place of the scalar load of en[k] -- as two more scalar
// loads per class the table cost the stride-8 head 49 % (each is a wait of its own in a loop the compiler does not pipeline).
struct FhTwoBest { int ia, ib; float va, vb; };
template <int KP, bool HUB = false>
__device__ __forceinline__ FhTwoBest fh_two_best(const FhArgs& a, const float (&wt)[4], const float* G, float sn,
                                                 const float* __restrict__ en, const float4* T = nullptr) {
    FhTwoBest r = {-1, -1, 0.f, 0.f};
    for (int k = 0; k < a.K; ++k) {
        const bool u = (bool)((class_word(a.unseen, k >> 6) >> (k & 63)) & 1ull);
        float sim;
        if constexpr (HUB) {
            const float4 t = T[k];
            float d = 0.f;
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) d = fmaf(wt[tp], G[tp * KP + k], d);
            sim = fmaf(d / (sn * t.x), t.y, -t.z);                  // fh_sim's operations on the staged en[k], then the correction
        } else {
            sim = fh_sim<KP>(wt, G, sn, en, k);
        }
        const bool first = u ? r.ib < 0 : r.ia < 0;
        const bool take = first || sim > (u ? r.vb : r.va);
        if (take && u) { r.vb = sim; r.ib = k; }
        if (take && !u) { r.va = sim; r.ia = k; }
    }
    return r;
}

// Both answers of the GROUPED fh_argmax in one trip (szn_seen_sweep_head): ia = what it returns for a pixel that takes the seen group,
// ib = for one that takes the unseen group.  Each running best sees fh_argmax's own sequence of values -- the similarity for a class of
// its group, zero_sim for every other class -- and replaces on k == 0 or a strictly larger value, so the two agree with it bit for bit,
// zeroed rows, ties, NaN and zero norms included.  One division per class serves both.
struct FhGroupBest { int ia, ib; };
template <int KP>
__device__ __forceinline__ FhGroupBest fh_group_bests(const FhArgs& a, const float (&wt)[4], const float* G, float sn,
                                                      const float* __restrict__ en) {
    const float zero_sim = 0.f / (sn * 1.f);
    FhGroupBest r = {0, 0};
    float va = 0.f, vb = 0.f;
    for (int k = 0; k < a.K; ++k) {
        const bool u = (bool)((class_word(a.unseen, k >> 6) >> (k & 63)) & 1ull);
        const float sim = fh_sim<KP>(wt, G, sn, en, k);
        const float sa = u ? zero_sim : sim, sb = u ? sim : zero_sim;
        if (k == 0 || sa > va) { va = sa; r.ia = k; }
        if (k == 0 || sb > vb) { vb = sb; r.ib = k; }
    }
    return r;
}

// what one pixel hands to the label loop (lbl < 0: nothing)
struct FhPx { float wt[4]; long lbl; float aco; };

// Pixel (ty, tx) of cell (I, J) of image b (live == false: the lane has none): its weights, |s|, the prediction, the loss term
// and the Bm update; bm, cos_sum, cnt are what a lane sums over its pixels.  Pk: the cell's P_k rows (MSE, block kernel); null
// where the caller adds the MSE loss term itself, in the class's turn of fh_scatter_A (wave kernel).
template <int KP, int S, bool GROUPED, bool MSE>
__device__ __forceinline__ FhPx fh_pixel(const FhArgs& a, int b, int I, int J, int ty, int tx, bool live, const float* G,
                                         const float* Q, const float* __restrict__ en, const float* __restrict__ ent,
                                         const float* Pk, float (&bm)[16], double& cos_sum, double& cnt) {
    FhPx px = {{0.f, 0.f, 0.f, 0.f}, -1, 0.f};
    const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;        // image coords y = Y - crop
    if (live && y >= 0 && y < a.H && x >= 0 && x < a.W) {
        cell_weights<S>(ty, tx, px.wt);
        const float (&wt)[4] = px.wt;
        const float ss = fh_ss(wt, Q);
        const float sn = sqrtf(ss);
        const size_t pix = ((size_t)b * a.H + y) * a.W + x;
        px.lbl = a.target ? a.target[pix] : -1;
        if (GROUPED || a.pred) a.pred[pix] = fh_argmax<KP, GROUPED>(a, wt, G, sn, en, pix, px.lbl);
        if (MSE && px.lbl >= 0) {
            const int kl = px.lbl < a.K ? (int)px.lbl : 0;
            if (Pk) cos_sum += (double)mse_px(wt, Pk + kl * 10);
            cnt += 1.0;
            px.aco = 1.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < 4; ++u) bm[t * 4 + u] += wt[t] * wt[u];
        } else if (px.lbl >= 0) {
            const int kl = px.lbl < a.K ? (int)px.lbl : 0;
            float d = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) d = fmaf(wt[t], G[t * KP + kl], d);
            const float nt = ent[kl];
            const float cosv = d / (sn * nt);
            cos_sum += (double)cosv;
            cnt += 1.0;
            px.aco = 1.f / (sn * nt);
            const float bco = cosv / ss;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < 4; ++u) bm[t * 4 + u] = fmaf(wt[t] * wt[u], bco, bm[t * 4 + u]);
        }
    }
    return px;
}

// A[t][label] += w_t * aco over the pixels of a wave, label by label in a fixed order (wave-uniform loop).  class_turn(kl, mine)
// runs first in the turn of every label kl; `mine`: this lane's pixel carries it.
template <int KP, typename F>
__device__ __forceinline__ void fh_scatter_A(const FhPx& px, int K, int lane, float* myA, F class_turn) {
    unsigned long long todo = __ballot(px.lbl >= 0);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const int kl = (int)__shfl((int)(px.lbl < K ? px.lbl : 0), src, 64);
        const bool mine = (px.lbl >= 0) && ((int)(px.lbl < K ? px.lbl : 0) == kl);
        class_turn(kl, mine);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float s = wave_sum(mine ? px.wt[t] * px.aco : 0.f);
            if (lane == 0) myA[t * KP + kl] += s;
        }
        todo &= ~__ballot(mine);
    }
}

// workspace: floats embT [E][KP] | en [KP] (0 -> 1, for the argmax) | ent [KP] (raw norms, for the loss)
//                   | per cell: A [4][KP] , Bm [16]
//            doubles (8-B aligned) part [cells][2] | sums [B][2] (per-image {sum, count})
//            floats the per-position tables of the small-cell path: D [pos][KP] | N [pos][8]
__host__ __device__ inline size_t ws_cell_off(int E, int KP) { return prep_floats(E, KP); }
__host__ __device__ inline size_t ws_cell_stride(int KP) { return (size_t)4 * KP + 16; }
struct FhWorkspace { size_t part, sums, tabD, tabN, bytes; };       // byte offsets
inline FhWorkspace fh_workspace(int B, int h, int w, int E, int KP) {
    const size_t cells = (size_t)B * (h + 1) * (w + 1), npos = (size_t)B * h * w;
    FhWorkspace L;
    L.part = (ws_cell_off(E, KP) + cells * ws_cell_stride(KP)) * sizeof(float);
    L.part = (L.part + alignof(double) - 1) / alignof(double) * alignof(double);
    L.sums = L.part + cells * 2 * sizeof(double);
    L.tabD = L.sums + (size_t)B * 2 * sizeof(double);
    L.tabN = L.tabD + npos * KP * sizeof(float);
    L.bytes = L.tabN + npos * 8 * sizeof(float);
    return L;
}

// dynamic LDS of fh_cell_kernel, offsets in floats
struct FhLds {
    int Ct;         // [4][E]
    int G;          // [4][KP]
    int Q;          // [16]
    int Aw;         // [4 waves][4][KP]
    int red;        // [4 waves][16]
    int dred;       // [4 waves][2] doubles
    int Pk;         // MSE only: [KP][10], rows of the classes present in this cell
    int present;    // MSE only: [KP] ints
    int end;
    __host__ __device__ size_t bytes() const { return (size_t)end * sizeof(float); }
};
__host__ __device__ inline FhLds fh_lds(int E, int KP, bool mse) {
    constexpr int kPerDouble = sizeof(double) / sizeof(float);
    FhLds L;
    L.Ct = 0;
    L.G = L.Ct + 4 * E;
    L.Q = L.G + 4 * KP;
    L.Aw = L.Q + 16;
    L.red = L.Aw + 16 * KP;
    L.dred = (L.red + 64 + kPerDouble - 1) / kPerDouble * kPerDouble;
    L.Pk = L.dred + 8 * kPerDouble;
    L.present = L.Pk + (mse ? 10 * KP : 0);
    L.end = L.present + (mse ? KP : 0);
    return L;
}

// the four tap vectors of cell (I, J) of image b into LDS Ct [4][E] (missing taps are zero); the caller synchronises
__device__ __forceinline__ void fh_load_taps(const FhArgs& a, int b, int I, int J, int tid, float* Ct) {
    for (int i = tid; i < 4 * a.E; i += 256) {
        const int t = i / a.E, c = i - t * a.E;
        const long tp = tap_pos(b, a.h, a.w, I, J, t);
        Ct[i] = (tp >= 0) ? a.coarse[(size_t)tp * a.ldc + a.c0 + c] : 0.f;
    }
}

// G [4][KP] and Q [4][4] of a block's cell from its tap vectors in LDS: wave t builds row t of both; the caller synchronises
template <int KP>
__device__ __forceinline__ void fh_build_GQ(const FhArgs& a, const float* __restrict__ embT, const float* Ct, int lane, int wave,
                                            float* G, float* Q) {
    // G[t][k]: wave t, lane k (+ 64, + 128, + 192 when KP > 64)
    for (int k = lane; k < KP; k += 64) {
        float g = 0.f;
        const float* ct = Ct + wave * a.E;
        // (the chain is sequential by contract; 20 independent L2 loads per batch keep it fed)
        int c = 0;
        for (; c + 20 <= a.E; c += 20) {
            float ev[20];
#pragma unroll
            for (int u = 0; u < 20; ++u) ev[u] = embT[(size_t)(c + u) * KP + k];
#pragma unroll
            for (int u = 0; u < 20; ++u) g = fmaf(ct[c + u], ev[u], g);
        }
        for (; c < a.E; ++c) g = fmaf(ct[c], embT[(size_t)c * KP + k], g);
        G[wave * KP + k] = g;
    }
    // Q[t][t']: wave t computes its row; lanes stride over c, fixed-order wave reduction
    {
        float q[4] = {0.f, 0.f, 0.f, 0.f};
        const float* ct = Ct + wave * a.E;
        for (int c = lane; c < a.E; c += 64) {
            const float v = ct[c];
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = fmaf(v, Ct[u * a.E + c], q[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float s = wave_sum(q[u]);
            if (lane == 0) Q[wave * 4 + u] = s;
        }
    }
}

__global__ __launch_bounds__(256) void fh_prep_kernel(const float* __restrict__ embed, float* __restrict__ ws, int E,
                                                      int K, int KP) {
    float* embT = ws;
    float* en = ws + (size_t)E * KP;
    float* ent = en + KP;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < E * KP; i += gridDim.x * 256) {
        const int k = i % KP, c = i / KP;
        embT[i] = (k < K) ? embed[(size_t)k * E + c] : 0.f;
    }
    if (blockIdx.x == 0) {
        // norms: thread k walks its row in ascending order (the order is part of the arithmetic contract with the oracle).  The
        // rows are staged through LDS in slices first: as a chain of dependent global loads the 300 steps took ~25 us.
        __shared__ float row[64][65];
        float s = 0.f;
        const int k = threadIdx.x;                 // class k (K <= 256 = the block)
        for (int g0 = 0; g0 < K; g0 += 64)         // 64 classes at a time through the LDS tile
            for (int c0 = 0; c0 < E; c0 += 64) {
                const int n = min(64, E - c0);
                __syncthreads();
                for (int i = threadIdx.x; i < 64 * 64; i += 256) {
                    const int kk = i >> 6, c = i & 63;
                    row[kk][c] = (g0 + kk < K && c < n) ? embed[(size_t)(g0 + kk) * E + c0 + c] : 0.f;
                }
                __syncthreads();
                if (k < K && (k >> 6) == (g0 >> 6))
                    for (int c = 0; c < n; ++c) s = fmaf(row[k & 63][c], row[k & 63][c], s);
            }
        if (k < KP) {
            const float nrm = sqrtf(s);
            en[k] = (nrm == 0.f) ? 1.f : nrm;
            ent[k] = nrm;
        }
    }
}

template <int KP, int S, bool GROUPED, bool MSE>
__global__ __launch_bounds__(256) void fh_cell_kernel(FhArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const FhLds L = fh_lds(a.E, KP, MSE);
    float* Ct = sm + L.Ct;
    float* G = sm + L.G;
    float* Q = sm + L.Q;
    float* Aw = sm + L.Aw;
    float* red = sm + L.red;
    double* dred = (double*)(sm + L.dred);
    float* Pk = sm + L.Pk;
    int* present = (int*)(sm + L.present);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const int b = blockIdx.x / cells, cell = blockIdx.x % cells;
    const int I = cell / cells_w, J = cell % cells_w;

    const float* embT = a.ws_f;
    const float* en = a.ws_f + (size_t)a.E * KP;
    const float* ent = en + KP;

    // ---- the four tap vectors (missing taps are zero) ----
    fh_load_taps(a, b, I, J, tid, Ct);
    for (int i = tid; i < 16 * KP; i += 256) Aw[i] = 0.f;
    if (MSE)
        for (int i = tid; i < KP; i += 256) present[i] = 0;
    __syncthreads();
    // MSE: a first pass over the labels marks the classes of this cell for the P_k pass (the pixel loop reads them again from L2)
    if (MSE && a.target) {
        for (int q = tid; q < S * S; q += 256) {
            const int y = S * I + q / S - a.crop, x = S * J + q % S - a.crop;
            if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
                const long l = a.target[((size_t)b * a.H + y) * a.W + x];
                if (l >= 0) present[l < a.K ? (int)l : 0] = 1;    // every writer stores the same value
            }
        }
    }
    fh_build_GQ<KP>(a, embT, Ct, lane, wave, G, Q);
    __syncthreads();
    if (MSE) {
        // P_k of the present classes, ascending k, dealt to the waves in turn
        int n = 0;
        for (int k = 0; k < a.K; ++k) {
            if (!present[k]) continue;
            if ((n++ & 3) != wave) continue;
            float p[10];
            fh_pk(a.embed + (size_t)k * a.E, a.E, lane, [&](int t, int c) { return Ct[t * a.E + c]; }, p);
            if (lane == 0) {
#pragma unroll
                for (int v = 0; v < 10; ++v) Pk[k * 10 + v] = p[v];
            }
        }
        __syncthreads();
    }

    // ---- pixels of this cell: Y in [S I, S I + S) x X in [S J, S J + S) ----
    float bm[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) bm[u] = 0.f;
    double cos_sum = 0.0, cnt = 0.0;
    float* myA = Aw + wave * 4 * KP;
    for (int q = tid; q < S * S; q += 256) {         // S = 32: a wave covers 2 rows of the cell; S = 8: wave 0 holds the whole cell
        const FhPx px = fh_pixel<KP, S, GROUPED, MSE>(a, b, I, J, q / S, q % S, true, G, Q, en, ent, Pk, bm, cos_sum, cnt);
        fh_scatter_A<KP>(px, a.K, lane, myA, [](int, bool) {});
    }
    // ---- block reductions (fixed order) ----
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const float r = wave_sum(bm[u]);
        if (lane == 0) red[wave * 16 + u] = r;
    }
    cos_sum = wave_sum_d(cos_sum); cnt = wave_sum_d(cnt);
    if (lane == 0) { dred[wave * 2] = cos_sum; dred[wave * 2 + 1] = cnt; }
    __syncthreads();
    float* wc = a.ws_f + ws_cell_off(a.E, KP) + (size_t)blockIdx.x * ws_cell_stride(KP);
    for (int i = tid; i < 4 * KP; i += 256) wc[i] = combine4(Aw[i], Aw[4 * KP + i], Aw[8 * KP + i], Aw[12 * KP + i]);
    if (tid < 16) wc[4 * KP + tid] = combine4(red[tid], red[16 + tid], red[32 + tid], red[48 + tid]);
    if (tid == 0) {
        a.part[(size_t)blockIdx.x * 2] = combine4(dred[0], dred[2], dred[4], dred[6]);
        a.part[(size_t)blockIdx.x * 2 + 1] = combine4(dred[1], dred[3], dred[5], dred[7]);
    }
}

// ---- small cells (stride 8): per-POSITION tables instead of per-cell dot products -----------------------------------------------
// With 8x8 cells a block per cell would spend its time re-deriving G and Q (each coarse vector is a tap of 4 cells).  Both only
// depend on coarse positions:  D[pos][k] = C_pos . e_k,  N[pos][n] = C_pos . C_nbr for nbr in {self, E, S, SE, SW}; a cell's
// G[t][k] / Q[t][u] are lookups.  Same chains as fh_cell_kernel (ascending fmaf for D; 64 strided partial chains + xor butterfly
// for N), so the two paths -- and the CPU restatement -- agree bit for bit.
template <int KP>
__global__ __launch_bounds__(256) void fh_tables_kernel(FhArgs a, float* __restrict__ D, float* __restrict__ N) {
    extern __shared__ __attribute__((aligned(16))) float sm[];            // [4 waves][E]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long npos = (long)a.B * a.h * a.w;
    const long pos = (long)blockIdx.x * 4 + wave;
    const bool ok = pos < npos;
    const long p = ok ? pos : 0;
    const int b = (int)(p / (a.h * a.w)), r = (int)(p % (a.h * a.w));
    const int i = r / a.w, j = r % a.w;
    const float* cv = a.coarse + (size_t)p * a.ldc + a.c0;
    float* Cs = sm + wave * a.E;
    for (int c = lane; c < a.E; c += 64) Cs[c] = cv[c];
    __syncthreads();
    const float* embT = a.ws_f;
    for (int k = lane; ok && k < KP; k += 64) {
        float g = 0.f;
        for (int c = 0; c < a.E; ++c) g = fmaf(Cs[c], embT[(size_t)c * KP + k], g);
        D[(size_t)pos * KP + k] = g;
    }
    const int di[5] = {0, 0, 1, 1, 1}, dj[5] = {0, 1, 0, 1, -1};
#pragma unroll
    for (int n = 0; n < 5; ++n) {
        const int ni = i + di[n], nj = j + dj[n];
        float q = 0.f;
        if (ni < a.h && nj >= 0 && nj < a.w) {
            const float* nv = a.coarse + (((size_t)b * a.h + ni) * a.w + nj) * a.ldc + a.c0;
            for (int c = lane; c < a.E; c += 64) q = fmaf(Cs[c], nv[c], q);
        }
        q = wave_sum(q);
        if (ok && lane == 0) N[(size_t)pos * 8 + n] = q;
    }
}

// G [4][KP] and Q [4][4] of a wave's cell looked up in the position tables (tp: the cell's four tap positions, -1 = outside the map)
template <int KP>
__device__ __forceinline__ void fh_lookup_GQ(const long (&tp)[4], const float* __restrict__ D, const float* __restrict__ N, int lane,
                                             float* G, float* Q) {
    for (int k = lane; k < KP; k += 64) {
#pragma unroll
        for (int t = 0; t < 4; ++t) G[t * KP + k] = (tp[t] >= 0) ? D[(size_t)tp[t] * KP + k] : 0.f;
    }
    if (lane < 16) {
        const int t = min(lane >> 2, lane & 3), u = max(lane >> 2, lane & 3);
        // (t, u) -> neighbour slot of the LOWER tap: self, E, S, SE | (1,2) SW, (1,3) S | (2,3) E
        const int slot = (t == u) ? 0 : (t == 0 ? u : (t == 1 ? (u == 2 ? 4 : 2) : 1));
        const long pt = (t == 0) ? tp[0] : (t == 1) ? tp[1] : (t == 2) ? tp[2] : tp[3];
        const long pu = (u == 0) ? tp[0] : (u == 1) ? tp[1] : (u == 2) ? tp[2] : tp[3];
        Q[lane] = (pt >= 0 && pu >= 0) ? N[(size_t)pt * 8 + slot] : 0.f;
    }
}

// one wave per cell (S * S <= 64 pixels), four cells per block; same per-pixel arithmetic and the same outputs as fh_cell_kernel
template <int KP, int S, bool GROUPED, bool MSE>
__global__ __launch_bounds__(256) void fh_cell_tab_kernel(FhArgs a, const float* __restrict__ D, const float* __restrict__ N) {
    static_assert(S * S <= 64, "one wave per cell");
    __shared__ float Gs[4][4 * KP];
    __shared__ float Qs[4][16];
    __shared__ float As[4][4 * KP];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const long ncell = (long)a.B * cells;
    const long cid = (long)blockIdx.x * 4 + wave;
    const bool ok = cid < ncell;
    const long cc = ok ? cid : 0;
    const int b = (int)(cc / cells), cell = (int)(cc % cells);
    const int I = cell / cells_w, J = cell % cells_w;
    const float* en = a.ws_f + (size_t)a.E * KP;
    const float* ent = en + KP;
    float* G = Gs[wave];
    float* Q = Qs[wave];
    float* myA = As[wave];
    long tp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) tp[t] = tap_pos(b, a.h, a.w, I, J, t);
    for (int i = lane; i < 4 * KP; i += 64) myA[i] = 0.f;
    fh_lookup_GQ<KP>(tp, D, N, lane, G, Q);
    __syncthreads();

    float bm[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) bm[u] = 0.f;
    double cos_sum = 0.0, cnt = 0.0;
    const FhPx px = fh_pixel<KP, S, GROUPED, MSE>(a, b, I, J, lane / S, lane % S, ok && lane < S * S, G, Q, en, ent, nullptr, bm, cos_sum, cnt);
    fh_scatter_A<KP>(px, a.K, lane, myA, [&](int kl, bool mine) {
        if (MSE) {
            // P_kl from the vectors (same chains as fh_cell_kernel), kept in registers; the loss term of the pixels that carry kl
            float p[10];
            fh_pk(a.embed + (size_t)kl * a.E, a.E, lane,
                  [&](int t, int c) { return (tp[t] >= 0) ? a.coarse[(size_t)tp[t] * a.ldc + a.c0 + c] : 0.f; }, p);
            if (mine) cos_sum += (double)mse_px(px.wt, p);
        }
    });
    float bs[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) bs[u] = wave_sum(bm[u]);
    cos_sum = wave_sum_d(cos_sum); cnt = wave_sum_d(cnt);
    __syncthreads();
    if (!ok) return;
    float* wc = a.ws_f + ws_cell_off(a.E, KP) + (size_t)cid * ws_cell_stride(KP);
    for (int i = lane; i < 4 * KP; i += 64) wc[i] = myA[i];
    if (lane == 0) {
#pragma unroll
        for (int u = 0; u < 16; ++u) wc[4 * KP + u] = bs[u];
        a.part[(size_t)cid * 2] = cos_sum;
        a.part[(size_t)cid * 2 + 1] = cnt;
    }
}

// ---- similarity cross-entropy (szn_fused_simce_head): softmax over the competing classes' cosines ------------------------------------
// term = logsumexp_{k in S} cos_k / T - cos_label / T over the classes S outside `excl`.  The cell algebra is the cosine head's (G, Q,
// fh_sim, fh_argmax: pred is that head's bit for bit); the per-pixel coefficients are dense in k:
//     A[t][k] = sum_px w_t (y_k - p_k) / (T |s| n_k),      Bm[t][u] = sum_px w_t w_u (cos_label - sum_k p_k cos_k) / (T |s|^2)
// so fh_gather_kernel<T, false> and the `mse` form of fh_finalize_kernel serve it unchanged.  A pixel walks the classes three times
// (max, sum of exps, coefficients) re-deriving cos_k from G each time (sce_cos: 4 broadcast LDS reads, 4 fmaf, 2 products), cheaper than
// holding K values per lane.  Dense A: 64 classes at a time, every lane writes its pixel's coefficients to row `lane` of a per-wave LDS tile
// [64][65] (the odd row stride keeps both the row-wise writes and the column-wise reads free of bank conflicts), then lane k walks
// the 64 pixels of column k in ascending order, one fmaf chain per tap: fixed order, no cross-lane traffic, no atomics.
struct SceArgs { ClassBits excl; float inv_t; };
constexpr int kSceRow = 65;                         // tile row stride in floats
constexpr int kSceWave = 64 * kSceRow + 64 * 4;     // per wave: tile [64][65] | the pixels' tap weights [64][4]

__device__ __forceinline__ bool sce_competes(const SceArgs& s, int k) { return !((class_word(s.excl, k >> 6) >> (k & 63)) & 1ull); }

// what one pixel hands to the dense-A pass (counted == false: all its coefficients are zero)
struct ScePx { float wt[4]; long lbl; bool counted; float rsn, m, rsum; };

// cos_k of the softmax passes: fh_sim's dot product times 1 / |s| (one division per pixel) and the hardware reciprocal of n_k (1 ulp),
// instead of a division per class and pass.  All three passes call this one function, so max_k z_k is the maximum of the very
// values the exponentials see.  (The prediction keeps fh_sim's division: its bits are the cosine head's.)
template <int KP>
__device__ __forceinline__ float sce_cos(const float (&wt)[4], const float* G, float rsn, const float* __restrict__ en, int k) {
    float d = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) d = fmaf(wt[t], G[t * KP + k], d);
    return d * (rsn * __builtin_amdgcn_rcpf(en[k]));
}

// Pixel (ty, tx) of cell (I, J) of image b: prediction (fh_pixel's), and for a counted pixel the softmax statistics, the loss term and
// the Bm update.  No target: nothing but the prediction.
template <int KP, int S, bool GROUPED>
__device__ __forceinline__ ScePx sce_pixel(const FhArgs& a, const SceArgs& s, int b, int I, int J, int ty, int tx, bool live,
                                           const float* G, const float* Q, const float* __restrict__ en, float (&bm)[16],
                                           double& term_sum, double& cnt) {
    ScePx px = {{0.f, 0.f, 0.f, 0.f}, -1, false, 0.f, 0.f, 0.f};
    const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;
    if (live && y >= 0 && y < a.H && x >= 0 && x < a.W) {
        cell_weights<S>(ty, tx, px.wt);
        const float (&wt)[4] = px.wt;
        const float ss = fh_ss(wt, Q);
        const float sn = sqrtf(ss);
        const size_t pix = ((size_t)b * a.H + y) * a.W + x;
        px.lbl = a.target ? a.target[pix] : -1;
        if (GROUPED || a.pred) a.pred[pix] = fh_argmax<KP, GROUPED>(a, wt, G, sn, en, pix, px.lbl);
        if (px.lbl >= 0 && px.lbl < a.K && !in_set(s.excl, px.lbl)) {
            const float rsn = 1.f / sn;
            float m = -INFINITY;
            for (int k = 0; k < a.K; ++k)
                if (sce_competes(s, k)) m = fmaxf(m, sce_cos<KP>(wt, G, rsn, en, k) * s.inv_t);
            float sum = 0.f, sc = 0.f;
            for (int k = 0; k < a.K; ++k)
                if (sce_competes(s, k)) {
                    const float c = sce_cos<KP>(wt, G, rsn, en, k);
                    const float e = expf(c * s.inv_t - m);
                    sum += e;
                    sc = fmaf(e, c, sc);
                }
            const float cl = sce_cos<KP>(wt, G, rsn, en, (int)px.lbl);
            term_sum += (double)((m - cl * s.inv_t) + logf(sum));
            cnt += 1.0;
            px.counted = true; px.rsn = rsn; px.m = m; px.rsum = 1.f / sum;
            const float bco = (cl - sc * px.rsum) * s.inv_t / ss;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < 4; ++u) bm[t * 4 + u] = fmaf(wt[t] * wt[u], bco, bm[t * 4 + u]);
        }
    }
    return px;
}

// The per-pixel coefficient of class k that sim_ce hands to the dense-A pass: (y_k - p_k) / (T |s| n_k), 0 for a pixel that does not
// count and a class that does not compete.
template <int KP>
struct SceCoef {
    const SceArgs& s; const ScePx& px; const float* G; const float* __restrict__ en; float aco;
    __device__ __forceinline__ SceCoef(const SceArgs& s_, const ScePx& px_, const float* G_, const float* __restrict__ en_)
        : s(s_), px(px_), G(G_), en(en_), aco(s_.inv_t * px_.rsn) {}
    __device__ __forceinline__ float operator()(int k) const {
        float c = 0.f;
        if (px.counted && sce_competes(s, k)) {
            const float p = expf(sce_cos<KP>(px.wt, G, px.rsn, en, k) * s.inv_t - px.m) * px.rsum;
            c = (((long)k == px.lbl ? 1.f : 0.f) - p) * (aco * __builtin_amdgcn_rcpf(en[k]));
        }
        return c;
    }
};

// A[t][k] += sum over the wave's 64 pixels of w_t coef(k), every k < K; coef(k) is this lane's pixel's coefficient of class k (SceCoef,
// RankCoef), wt its tap weights.  wl: this wave's kSceWave floats of LDS.
// Block-uniform control flow (the barriers order the tile writes before the column reads, and the reads before the next writes).
template <int KP, class Coef>
__device__ __forceinline__ void sce_dense_A(const FhArgs& a, const float (&wt)[4], const Coef& coef, int lane, float* wl, float* myA) {
    float* tile = wl;
    float* wpx = wl + 64 * kSceRow;
#pragma unroll
    for (int t = 0; t < 4; ++t) wpx[lane * 4 + t] = wt[t];
    for (int k0 = 0; k0 < a.K; k0 += 64) {
        const int nk = min(64, a.K - k0);
        for (int kk = 0; kk < nk; ++kk) tile[lane * kSceRow + kk] = coef(k0 + kk);
        __syncthreads();
        if (lane < nk) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int p = 0; p < 64; ++p) {
                const float c = tile[p * kSceRow + lane];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = fmaf(wpx[p * 4 + t], c, acc[t]);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) myA[t * KP + k0 + lane] += acc[t];
        }
        __syncthreads();
    }
}
template <int KP>
__device__ __forceinline__ SceCoef<KP> sce_coef(const SceArgs& s, const ScePx& px, const float* G, const float* __restrict__ en) {
    return SceCoef<KP>(s, px, G, en);
}

// ---- hinge ranking loss (szn_fused_rank_head, DeViSE): the pixel's own class must beat every other competing class by a margin ---------
// v_k = margin - cos_label + cos_k, k in S \ {label}.  Sum of hinges: term = sum_k max(0, v_k), c_k = 1[v_k > 0]; hardest negative:
// term = max(0, v_k*), k* = the lowest index of the largest v_k, c_k* = 1[v_k* > 0]; c_label = -sum_k c_k.  The gradient has sim_ce's
// shape with c_k in the place of (p_k - y_k) / T, so the cell kernels, the tile and everything downstream are sim_ce's:
//     A[t][k] = -sum_px w_t c_k / (|s| n_k),      Bm[t][u] = -sum_px w_t w_u sum_k c_k cos_k / |s|^2
// One walk over the classes per pixel (term, number of violators, sum of their cosines | the best negative); no exponential, no
// logarithm.  The dense-A pass re-derives 1[v_k > 0] from the same sce_cos and the same rank_v > 0 as that walk (hardest: from the
// stored k*), so A and Bm describe one sub-gradient.  v_k = 0 exactly: coefficient 0.
struct RankArgs { ClassBits excl; float margin; int hardest; };
// mcl = margin - cos_label; nv = -c_label (the number of violators, 0 | 1 for hardest); kstar: hardest only, -1 without a violator
struct RankPx { float wt[4]; long lbl; bool counted; float rsn, mcl, nv; int kstar; };

__device__ __forceinline__ bool sce_competes(const RankArgs& s, int k) { return !((class_word(s.excl, k >> 6) >> (k & 63)) & 1ull); }
__device__ __forceinline__ float rank_v(float mcl, float c) { return mcl + c; }

template <int KP, int S, bool GROUPED>
__device__ __forceinline__ RankPx sce_pixel(const FhArgs& a, const RankArgs& s, int b, int I, int J, int ty, int tx, bool live,
                                            const float* G, const float* Q, const float* __restrict__ en, float (&bm)[16],
                                            double& term_sum, double& cnt) {
    RankPx px = {{0.f, 0.f, 0.f, 0.f}, -1, false, 0.f, 0.f, 0.f, -1};
    const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;
    if (live && y >= 0 && y < a.H && x >= 0 && x < a.W) {
        cell_weights<S>(ty, tx, px.wt);
        const float (&wt)[4] = px.wt;
        const float ss = fh_ss(wt, Q);
        const float sn = sqrtf(ss);
        const size_t pix = ((size_t)b * a.H + y) * a.W + x;
        px.lbl = a.target ? a.target[pix] : -1;
        if (GROUPED || a.pred) a.pred[pix] = fh_argmax<KP, GROUPED>(a, wt, G, sn, en, pix, px.lbl);
        if (px.lbl >= 0 && px.lbl < a.K && !in_set(s.excl, px.lbl)) {
            const float rsn = 1.f / sn;
            const float cl = sce_cos<KP>(wt, G, rsn, en, (int)px.lbl);
            const float mcl = s.margin - cl;
            float term = 0.f, nv = 0.f, sc = 0.f;
            if (s.hardest) {
                float best = -INFINITY, cbest = 0.f;
                int kb = -1;
                for (int k = 0; k < a.K; ++k)
                    if ((long)k != px.lbl && sce_competes(s, k)) {
                        const float c = sce_cos<KP>(wt, G, rsn, en, k);
                        const float v = rank_v(mcl, c);
                        if (v > best) { best = v; cbest = c; kb = k; }      // strict: the lowest index on a tie
                    }
                if (best > 0.f) { term = best; nv = 1.f; sc = cbest; px.kstar = kb; }
            } else {
                for (int k = 0; k < a.K; ++k)
                    if ((long)k != px.lbl && sce_competes(s, k)) {
                        const float c = sce_cos<KP>(wt, G, rsn, en, k);
                        const float v = rank_v(mcl, c);
                        if (v > 0.f) { term += v; nv += 1.f; sc += c; }
                    }
            }
            term_sum += (double)term;
            cnt += 1.0;
            px.counted = true; px.rsn = rsn; px.mcl = mcl; px.nv = nv;
            const float bco = (nv * cl - sc) / ss;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < 4; ++u) bm[t * 4 + u] = fmaf(wt[t] * wt[u], bco, bm[t * 4 + u]);
        }
    }
    return px;
}

// -c_k / (|s| n_k): nv for the label, -1 for a violator (hardest: for k*), 0 elsewhere
template <int KP>
struct RankCoef {
    const RankArgs& s; const RankPx& px; const float* G; const float* __restrict__ en;
    __device__ __forceinline__ float operator()(int k) const {
        if (!px.counted || px.nv == 0.f) return 0.f;
        float c = 0.f;
        if ((long)k == px.lbl) c = px.nv;
        else if (s.hardest ? k == px.kstar : sce_competes(s, k) && rank_v(px.mcl, sce_cos<KP>(px.wt, G, px.rsn, en, k)) > 0.f) c = -1.f;
        return c == 0.f ? 0.f : c * (px.rsn * __builtin_amdgcn_rcpf(en[k]));
    }
};
template <int KP>
__device__ __forceinline__ RankCoef<KP> sce_coef(const RankArgs& s, const RankPx& px, const float* G, const float* __restrict__ en) {
    return RankCoef<KP>{s, px, G, en};
}

// ---- sim_ce with the unseen-bias term on hidden pixels (szn_fused_simce_bias_head, QFSL) ---------------------------------------------
// A labelled pixel (0 <= lbl < K, lbl outside `excl`) is sim_ce's pixel: the same passes, the same expressions, the same bits.  A hidden
// pixel (lbl == hidden) is known to carry some class of `unseen`: its softmax runs over all K classes, z_k = cos_k / T, and its term is
//     weight * -log sum_{u in U} p_u = weight * ((m - m_U) + log sum_k e^{z_k - m} - log sum_u e^{z_u - m_U})
// with m = max_k z_k and m_U = max_u z_u: each sum holds a term equal to 1, so neither logarithm sees 0 where P_U itself (e^{-200} at
// T = 0.01) is no float.  q_k = 1[k in U] e^{z_k - m_U} / sum_U for the same reason, never p_k / P_U.  The gradient has sim_ce's shape
// with q_k in the place of y_k:
//     A[t][k] += w_t weight (q_k - p_k) / (T |s| n_k),      Bm[t][u] += w_t w_u weight (sum_k q_k cos_k - sum_k p_k cos_k) / (T |s|^2)
// Both kinds count 1 in N_b; sums, finalize and gather are sim_ce's.  Per pixel: |q_k - p_k| summed over k is at most 2, so the
// pixel's d(score) is bounded by 2 weight / (T |s|), sim_ce's 2 / (T |s|) times weight.
struct BiasArgs { ClassBits excl, unseen; float inv_t, weight; long hidden; };
// kind: 0 the pixel does not count, 1 labelled (m, rsum over the competing classes; mu, rsumu unused), 2 hidden (m, rsum over all
// classes, mu, rsumu over `unseen`)
struct BiasPx { float wt[4]; long lbl; int kind; float rsn, m, rsum, mu, rsumu; };

__device__ __forceinline__ bool sce_competes(const BiasArgs& s, int k) { return !((class_word(s.excl, k >> 6) >> (k & 63)) & 1ull); }
__device__ __forceinline__ bool bias_unseen(const BiasArgs& s, int k) { return (class_word(s.unseen, k >> 6) >> (k & 63)) & 1ull; }

template <int KP, int S, bool GROUPED>
__device__ __forceinline__ BiasPx sce_pixel(const FhArgs& a, const BiasArgs& s, int b, int I, int J, int ty, int tx, bool live,
                                            const float* G, const float* Q, const float* __restrict__ en, float (&bm)[16],
                                            double& term_sum, double& cnt) {
    BiasPx px = {{0.f, 0.f, 0.f, 0.f}, -1, 0, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;
    if (live && y >= 0 && y < a.H && x >= 0 && x < a.W) {
        cell_weights<S>(ty, tx, px.wt);
        const float (&wt)[4] = px.wt;
        const float ss = fh_ss(wt, Q);
        const float sn = sqrtf(ss);
        const size_t pix = ((size_t)b * a.H + y) * a.W + x;
        px.lbl = a.target ? a.target[pix] : -1;
        if (GROUPED || a.pred) a.pred[pix] = fh_argmax<KP, GROUPED>(a, wt, G, sn, en, pix, px.lbl);
        const bool lab = px.lbl >= 0 && px.lbl < a.K && !in_set(s.excl, px.lbl);
        const bool hid = px.lbl == s.hidden;             // hidden < -1: never the -1 of a call without target
        if (lab || hid) {
            // one walk per pass for both kinds, so a wave that holds both does not pay for two: a labelled lane skips the classes of
            // `excl` and never enters the U branch, and what it computes is sim_ce's sequence of operations
            const float rsn = 1.f / sn;
            float m = -INFINITY, mu = -INFINITY;
            for (int k = 0; k < a.K; ++k)
                if (hid || sce_competes(s, k)) {
                    const float z = sce_cos<KP>(wt, G, rsn, en, k) * s.inv_t;
                    m = fmaxf(m, z);
                    if (hid && bias_unseen(s, k)) mu = fmaxf(mu, z);
                }
            float sum = 0.f, sc = 0.f, sumu = 0.f, scu = 0.f;
            for (int k = 0; k < a.K; ++k)
                if (hid || sce_competes(s, k)) {
                    const float c = sce_cos<KP>(wt, G, rsn, en, k);
                    const float z = c * s.inv_t;
                    const float e = expf(z - m);
                    sum += e;
                    sc = fmaf(e, c, sc);
                    if (hid && bias_unseen(s, k)) {
                        const float eu = expf(z - mu);
                        sumu += eu;
                        scu = fmaf(eu, c, scu);
                    }
                }
            cnt += 1.0;
            px.rsn = rsn; px.m = m; px.rsum = 1.f / sum;
            float bco;
            if (lab) {
                const float cl = sce_cos<KP>(wt, G, rsn, en, (int)px.lbl);
                term_sum += (double)((m - cl * s.inv_t) + logf(sum));
                px.kind = 1;
                bco = (cl - sc * px.rsum) * s.inv_t / ss;
            } else {
                term_sum += (double)(s.weight * ((m - mu) + (logf(sum) - logf(sumu))));
                px.kind = 2; px.mu = mu; px.rsumu = 1.f / sumu;
                bco = s.weight * (scu * px.rsumu - sc * px.rsum) * s.inv_t / ss;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < 4; ++u) bm[t * 4 + u] = fmaf(wt[t] * wt[u], bco, bm[t * 4 + u]);
        }
    }
    return px;
}

// labelled: SceCoef's (y_k - p_k) / (T |s| n_k) over the competing classes; hidden: weight (q_k - p_k) / (T |s| n_k) over all classes
template <int KP>
struct BiasCoef {
    const BiasArgs& s; const BiasPx& px; const float* G; const float* __restrict__ en; float aco;
    __device__ __forceinline__ BiasCoef(const BiasArgs& s_, const BiasPx& px_, const float* G_, const float* __restrict__ en_)
        : s(s_), px(px_), G(G_), en(en_), aco(s_.inv_t * px_.rsn * (px_.kind == 2 ? s_.weight : 1.f)) {}      // x 1: exact
    __device__ __forceinline__ float operator()(int k) const {
        float c = 0.f;
        const bool hid = px.kind == 2;
        if (px.kind != 0 && (hid || sce_competes(s, k))) {                  // one walk for both kinds, as in sce_pixel
            const float z = sce_cos<KP>(px.wt, G, px.rsn, en, k) * s.inv_t;
            const float p = expf(z - px.m) * px.rsum;
            float tk = (long)k == px.lbl ? 1.f : 0.f;                       // y_k; a hidden pixel's label is no class
            if (hid && bias_unseen(s, k)) tk = expf(z - px.mu) * px.rsumu;  // q_k
            c = (tk - p) * (aco * __builtin_amdgcn_rcpf(en[k]));
        }
        return c;
    }
};
template <int KP>
__device__ __forceinline__ BiasCoef<KP> sce_coef(const BiasArgs& s, const BiasPx& px, const float* G, const float* __restrict__ en) {
    return BiasCoef<KP>(s, px, G, en);
}

// dynamic LDS in floats: stride 32 fh_lds(E, KP, false) | 4 waves' tiles; stride 8 G [4][4 KP] | A [4][4 KP] | Q [4][16] | the tiles
__host__ __device__ inline size_t sce_lds_floats(int stride, int E, int KP) {
    return (stride == 8 ? (size_t)32 * KP + 64 : (size_t)fh_lds(E, KP, false).end) + 4 * kSceWave;
}

// LA: SceArgs (sim_ce) | RankArgs (rank) | BiasArgs (sim_ce with the bias term); sce_pixel and sce_coef are overloaded on it
template <int KP, bool GROUPED, class LA>
__global__ __launch_bounds__(256) void sce_cell_kernel(FhArgs a, LA s) {        // stride 32: one block per (image, cell)
    constexpr int S = 32;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const FhLds L = fh_lds(a.E, KP, false);
    float* Ct = sm + L.Ct;
    float* G = sm + L.G;
    float* Q = sm + L.Q;
    float* Aw = sm + L.Aw;
    float* red = sm + L.red;
    double* dred = (double*)(sm + L.dred);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* wl = sm + L.end + wave * kSceWave;
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const int b = blockIdx.x / cells, cell = blockIdx.x % cells;
    const int I = cell / cells_w, J = cell % cells_w;
    const float* embT = a.ws_f;
    const float* en = a.ws_f + (size_t)a.E * KP;

    fh_load_taps(a, b, I, J, tid, Ct);
    for (int i = tid; i < 16 * KP; i += 256) Aw[i] = 0.f;
    __syncthreads();
    fh_build_GQ<KP>(a, embT, Ct, lane, wave, G, Q);
    __syncthreads();

    float bm[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) bm[u] = 0.f;
    double term_sum = 0.0, cnt = 0.0;
    float* myA = Aw + wave * 4 * KP;
    for (int q = tid; q < S * S; q += 256) {         // four rounds for every thread: the barriers of sce_dense_A are block-uniform
        const auto px = sce_pixel<KP, S, GROUPED>(a, s, b, I, J, q / S, q % S, true, G, Q, en, bm, term_sum, cnt);
        if (a.target) sce_dense_A<KP>(a, px.wt, sce_coef<KP>(s, px, G, en), lane, wl, myA);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const float r = wave_sum(bm[u]);
        if (lane == 0) red[wave * 16 + u] = r;
    }
    term_sum = wave_sum_d(term_sum); cnt = wave_sum_d(cnt);
    if (lane == 0) { dred[wave * 2] = term_sum; dred[wave * 2 + 1] = cnt; }
    __syncthreads();
    float* wc = a.ws_f + ws_cell_off(a.E, KP) + (size_t)blockIdx.x * ws_cell_stride(KP);
    for (int i = tid; i < 4 * KP; i += 256) wc[i] = combine4(Aw[i], Aw[4 * KP + i], Aw[8 * KP + i], Aw[12 * KP + i]);
    if (tid < 16) wc[4 * KP + tid] = combine4(red[tid], red[16 + tid], red[32 + tid], red[48 + tid]);
    if (tid == 0) {
        a.part[(size_t)blockIdx.x * 2] = combine4(dred[0], dred[2], dred[4], dred[6]);
        a.part[(size_t)blockIdx.x * 2 + 1] = combine4(dred[1], dred[3], dred[5], dred[7]);
    }
}

template <int KP, bool GROUPED, class LA>
__global__ __launch_bounds__(256) void sce_cell_tab_kernel(FhArgs a, LA s, const float* __restrict__ D,
                                                           const float* __restrict__ N) {      // stride 8: one wave per cell
    constexpr int S = 8;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* G = sm + wave * 4 * KP;
    float* myA = sm + 16 * KP + wave * 4 * KP;
    float* Q = sm + 32 * KP + wave * 16;
    float* wl = sm + 32 * KP + 64 + wave * kSceWave;
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const long ncell = (long)a.B * cells;
    const long cid = (long)blockIdx.x * 4 + wave;
    const bool ok = cid < ncell;
    const long cc = ok ? cid : 0;
    const int b = (int)(cc / cells), cell = (int)(cc % cells);
    const int I = cell / cells_w, J = cell % cells_w;
    const float* en = a.ws_f + (size_t)a.E * KP;
    long tp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) tp[t] = tap_pos(b, a.h, a.w, I, J, t);
    for (int i = lane; i < 4 * KP; i += 64) myA[i] = 0.f;
    fh_lookup_GQ<KP>(tp, D, N, lane, G, Q);
    __syncthreads();

    float bm[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) bm[u] = 0.f;
    double term_sum = 0.0, cnt = 0.0;
    const auto px = sce_pixel<KP, S, GROUPED>(a, s, b, I, J, lane / S, lane % S, ok && lane < S * S, G, Q, en, bm, term_sum, cnt);
    if (a.target) sce_dense_A<KP>(a, px.wt, sce_coef<KP>(s, px, G, en), lane, wl, myA);
    float bs[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) bs[u] = wave_sum(bm[u]);
    term_sum = wave_sum_d(term_sum); cnt = wave_sum_d(cnt);
    __syncthreads();
    if (!ok) return;
    float* wc = a.ws_f + ws_cell_off(a.E, KP) + (size_t)cid * ws_cell_stride(KP);
    for (int i = lane; i < 4 * KP; i += 64) wc[i] = myA[i];
    if (lane == 0) {
#pragma unroll
        for (int u = 0; u < 16; ++u) wc[4 * KP + u] = bs[u];
        a.part[(size_t)cid * 2] = term_sum;
        a.part[(size_t)cid * 2 + 1] = cnt;
    }
}

// loss = mean_b (N_b - S_b)/N_b (cosine) | mean_b S_b / N_b (mse); stats[b] = {S_b, N_b}.  One block per image sums its cells (fixed order: 256 strided double
// chains, wave butterflies, then the four wave totals), a single wave combines the images.
__global__ __launch_bounds__(256) void fh_image_sums_kernel(const double* __restrict__ part, int cells, float* __restrict__ stats,
                                                            double* __restrict__ sums) {
    __shared__ double red[4][2];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s = 0.0, n = 0.0;
    for (int k = threadIdx.x; k < cells; k += 256) { s += part[((size_t)b * cells + k) * 2]; n += part[((size_t)b * cells + k) * 2 + 1]; }
    s = wave_sum_d(s); n = wave_sum_d(n);
    if (lane == 0) { red[wave][0] = s; red[wave][1] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double st = combine4(red[0][0], red[1][0], red[2][0], red[3][0]), nt = combine4(red[0][1], red[1][1], red[2][1], red[3][1]);
        sums[2 * b] = st; sums[2 * b + 1] = nt;
        stats[2 * b] = (float)st; stats[2 * b + 1] = (float)nt;
    }
}

__global__ void fh_finalize_kernel(const double* __restrict__ sums, int B, int mse, float* __restrict__ loss) {
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int b = 0; b < B; ++b) acc += mse ? sums[2 * b] / sums[2 * b + 1] : (sums[2 * b + 1] - sums[2 * b]) / sums[2 * b + 1];
        loss[0] = (float)(acc / B);
    }
}

template <typename T, bool MSE>
__global__ __launch_bounds__(256) void fh_gather_kernel(const float* __restrict__ coarse, const float* __restrict__ embed,
                                                        const float* __restrict__ ws, const float* __restrict__ stats,
                                                        T* __restrict__ dcoarse, int B, int h, int w, int E, int ldc,
                                                        int c0, int K, int KP) {
    __shared__ float Al[4][256];     // A of the 4 cells (KP <= 256), row = the tap index this position has in that cell
    __shared__ float Bl[4][4];       // matching rows of Bm
    const int pos = blockIdx.x;
    const int b = pos / (h * w), r = pos % (h * w);
    const int i = r / w, j = r % w;
    const int cells_w = w + 1, cells = (h + 1) * cells_w;
    const float* cellbase = ws + ws_cell_off(E, KP);
    // this position is tap u of cell (tap_cell_I(i, u), tap_cell_J(j, u)), u = 0..3
    for (int idx = threadIdx.x; idx < 4 * KP + 16; idx += 256) {
        if (idx < 4 * KP) {
            const int u = idx / KP, k = idx % KP;
            const int I = tap_cell_I(i, u), J = tap_cell_J(j, u);
            const float* wc = cellbase + ((size_t)b * cells + I * cells_w + J) * ws_cell_stride(KP);
            Al[u][k] = wc[u * KP + k];
        } else {
            const int q = idx - 4 * KP, u = q >> 2, t2 = q & 3;
            const int I = tap_cell_I(i, u), J = tap_cell_J(j, u);
            const float* wc = cellbase + ((size_t)b * cells + I * cells_w + J) * ws_cell_stride(KP);
            Bl[u][t2] = wc[4 * KP + u * 4 + t2];
        }
    }
    __syncthreads();
    // the class term is linear in A: sum the four cells' rows first, one pass over the K embeddings instead of four
    Al[0][threadIdx.x] = (threadIdx.x < KP) ? combine4(Al[0][threadIdx.x], Al[1][threadIdx.x], Al[2][threadIdx.x], Al[3][threadIdx.x]) : 0.f;
    __syncthreads();
    const float scale = (MSE ? 2.f : 1.f) / ((float)B * stats[2 * b + 1]);
    for (int c = threadIdx.x; c < E; c += 256) {
        float acc = 0.f;
        for (int k = 0; k < K; ++k) acc = fmaf(-Al[0][k], embed[(size_t)k * E + c], acc);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float bu = 0.f;
            const int I = tap_cell_I(i, u), J = tap_cell_J(j, u);
#pragma unroll
            for (int t2 = 0; t2 < 4; ++t2) {
                const int ci = tap_i(I, t2), cj = tap_j(J, t2);
                if (ci >= 0 && ci < h && cj >= 0 && cj < w)
                    bu = fmaf(Bl[u][t2], coarse[(((size_t)b * h + ci) * w + cj) * ldc + c0 + c], bu);
            }
            acc += bu;
        }
        float v = acc * scale;
        // MSE: the 16-bit outputs are the rounding of the fp32 result.  Left alone, the compiler merges this product and the half
        // conversion into one v_fma_mixlo_f16 (a single rounding) despite -ffp-contract=off; the cosine instantiations keep that
        // form, their bits are pinned.
        if (MSE) asm volatile("" : "+v"(v));
        elem<T>::st(dcoarse + ((size_t)pos) * ldc + c0 + c, v);
    }
}

// ---- calibrated stacking (szn_calib_head): the cells' G and Q as above, two running bests per pixel, crossing tables ------------
// A pixel is (t, a, b, bin): target, best seen class, best unseen class, first gamma at which it takes b (n: never; include/szn.h).
// XA [K][K][n + 1] counts (t, a, bin), XB (t, b, bin), both int64, zeroed by the call.  Integer atomics: the result does not depend on
// their order.  The gammas travel as kernel arguments; the per-pixel search is a wave-uniform loop over them (scalar loads).
// CalArgs, calib_count and calib_hist_kernel: szn_calib.h (szn_conse_head.hip feeds the same tables).

// Pixel (ty, tx) of cell (I, J) of image b: the prediction at gammas[pred_index] (where wanted) and the pixel's key
// t | a << 8 | b << 16 | bin << 24, or -1 where it is not counted (no histogram, outside the image, label outside [0, K))
// HUB: szn_hub_head's hubness-corrected similarities (fh_two_best), T = the image's staged rows in LDS; nothing else differs
template <int KP, int S, bool HUB = false>
__device__ __forceinline__ int calib_pixel(const FhArgs& a, const CalArgs& c, int b, int I, int J, int ty, int tx, bool live,
                                           const float* G, const float* Q, const float* __restrict__ en, const float4* T = nullptr) {
    const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;
    if (!(live && y >= 0 && y < a.H && x >= 0 && x < a.W)) return -1;
    float wt[4];
    cell_weights<S>(ty, tx, wt);
    const float sn = sqrtf(fh_ss(wt, Q));
    FhTwoBest r = fh_two_best<KP, HUB>(a, wt, G, sn, en, T);
    const float m = r.va - r.vb;
    int bin = 0;
    if (m != m) { r.ia = 0; r.ib = 0; bin = c.n; }        // NaN: class 0 at every gamma
    else
        for (int g = 0; g < c.n; ++g) bin += (m > c.gamma[g] || (m == c.gamma[g] && r.ia < r.ib)) ? 1 : 0;   // ascending: a prefix
    const size_t pix = ((size_t)b * a.H + y) * a.W + x;
    if (c.pred) c.pred[pix] = bin > c.pred_index ? r.ia : r.ib;
    if (!c.XA) return -1;
    const long t = a.target[pix];
    if (t < 0 || t >= a.K) return -1;
    return (int)t | r.ia << 8 | r.ib << 16 | bin << 24;
}

// ---- seen-mask threshold sweep (szn_seen_sweep_head): the calibrated head's cells, tables and crossing scheme with another switch ------
// The thresholds travel in CalArgs::gamma.  A pixel takes the seen group at g iff margin[pix] > tau[g]; a is the grouped head's answer in
// the seen group, b in the unseen group (fh_group_bests), bin = the first g at which the comparison fails (a NaN margin: 0).
template <int KP, int S>
__device__ __forceinline__ int sweep_pixel(const FhArgs& a, const CalArgs& c, const float* __restrict__ margin, int b, int I, int J,
                                           int ty, int tx, bool live, const float* G, const float* Q, const float* __restrict__ en) {
    const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;
    if (!(live && y >= 0 && y < a.H && x >= 0 && x < a.W)) return -1;
    float wt[4];
    cell_weights<S>(ty, tx, wt);
    const float sn = sqrtf(fh_ss(wt, Q));
    const FhGroupBest r = fh_group_bests<KP>(a, wt, G, sn, en);
    const size_t pix = ((size_t)b * a.H + y) * a.W + x;
    const float m = margin[pix];
    int bin = 0;
    for (int g = 0; g < c.n; ++g) bin += (m > c.gamma[g]) ? 1 : 0;        // ascending: a prefix
    if (c.pred) c.pred[pix] = bin > c.pred_index ? r.ia : r.ib;
    if (!c.XA) return -1;
    const long t = a.target[pix];
    if (t < 0 || t >= a.K) return -1;
    return (int)t | r.ia << 8 | r.ib << 16 | bin << 24;
}

// ---- soft seen/unseen gating (szn_soft_gate_head): the sweep's cells, tables and crossing scheme with a per-pixel adaptive switch --------
// p(k | x) = p(group(k) | x) p(k | group(k), x) with p(seen) = sigmoid(margin - tau) and a softmax over the cosines at temperature T
// inside each group collapses to: the pixel takes a iff e = margin - weight * (l_S - l_U) > tau, l_G = -log P_G(best of G) (include/szn.h).
// a, b are the TRUE in-group argmaxes (fh_two_best's rule), not fh_group_bests' zeroed-row answers.
struct GateArgs {
    const float* margin;         // (B,H,W)
    float* eff;                  // (B,H,W) or null: e per pixel
    float inv_t, weight;
};

// One trip through the classes: fh_two_best's two running bests, and next to each the sum of exp((sim - best) / T) over its group,
// rescaled when the best moves (an online log-sum-exp).  One expf per class: its argument is -|sim - best| / T <= 0 either way -- the
// factor that rescales the old sum when sim takes over, the new term when it does not -- so nothing overflows, and the class that holds
// the maximum contributes exactly 1: sum >= 1, a group of one class gives exactly 1 and logf(1) = 0.  The group bit is wave-uniform as in
// fh_two_best: scalar selects.  A NaN similarity (zero-norm pixel) makes both sums NaN.
struct FhGateBest { int ia, ib; float ls, lu; };
template <int KP>
__device__ __forceinline__ FhGateBest fh_gate_bests(const FhArgs& a, const float (&wt)[4], const float* G, float sn,
                                                    const float* __restrict__ en, float inv_t) {
    int ia = -1, ib = -1;
    float va = 0.f, vb = 0.f, sa = 0.f, sb = 0.f;
    for (int k = 0; k < a.K; ++k) {
        const bool u = (bool)((class_word(a.unseen, k >> 6) >> (k & 63)) & 1ull);
        const float sim = fh_sim<KP>(wt, G, sn, en, k);
        const bool first = u ? ib < 0 : ia < 0;
        const float v = first ? sim : (u ? vb : va), s = u ? sb : sa;
        const bool take = first || sim > v;
        const float d = sim - v;                                  // the group's first class: 0, or NaN for a NaN similarity
        const float ex = expf((take ? -d : d) * inv_t);
        const float s2 = first ? 1.f + d : (take ? fmaf(s, ex, 1.f) : s + ex);
        if (u) { sb = s2; if (take) { vb = sim; ib = k; } }
        else { sa = s2; if (take) { va = sim; ia = k; } }
    }
    return {ia, ib, logf(sa), logf(sb)};
}

template <int KP, int S>
__device__ __forceinline__ int gate_pixel(const FhArgs& a, const CalArgs& c, const GateArgs& g, int b, int I, int J,
                                          int ty, int tx, bool live, const float* G, const float* Q, const float* __restrict__ en) {
    const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;
    if (!(live && y >= 0 && y < a.H && x >= 0 && x < a.W)) return -1;
    float wt[4];
    cell_weights<S>(ty, tx, wt);
    const float sn = sqrtf(fh_ss(wt, Q));
    FhGateBest r = fh_gate_bests<KP>(a, wt, G, sn, en, g.inv_t);
    const size_t pix = ((size_t)b * a.H + y) * a.W + x;
    const float D = r.ls - r.lu;
    const float e = fmaf(-g.weight, D, g.margin[pix]);
    int bin = 0;
    if (D != D) { r.ia = 0; r.ib = 0; bin = c.n; }        // NaN (a zero-norm pixel): class 0 at every tau, calib_pixel's rule
    else
        for (int t = 0; t < c.n; ++t) bin += (e > c.gamma[t]) ? 1 : 0;     // ascending: a prefix; a NaN margin: the unseen group
    if (g.eff) g.eff[pix] = e;
    if (c.pred) c.pred[pix] = bin > c.pred_index ? r.ia : r.ib;
    if (!c.XA) return -1;
    const long t = a.target[pix];
    if (t < 0 || t >= a.K) return -1;
    return (int)t | r.ia << 8 | r.ib << 16 | bin << 24;
}

// The two walks over the pixels that the calibrated head and the threshold sweep share: px(b, I, J, ty, tx, live, G, Q, en) is the head's
// per-pixel body (calib_pixel, sweep_pixel, gate_pixel) and returns the pixel's key.  Stride 32: one block per (image, cell), G and Q built in `sm`.
template <int KP, typename Px>
__device__ __forceinline__ void calib_cell_walk(const FhArgs& a, const CalArgs& c, float* sm, Px px) {
    constexpr int S = 32;
    const FhLds L = fh_lds(a.E, KP, false);
    float* Ct = sm + L.Ct;
    float* G = sm + L.G;
    float* Q = sm + L.Q;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const int b = blockIdx.x / cells, cell = blockIdx.x % cells;
    const int I = cell / cells_w, J = cell % cells_w;
    const float* embT = a.ws_f;
    const float* en = a.ws_f + (size_t)a.E * KP;
    fh_load_taps(a, b, I, J, tid, Ct);
    __syncthreads();
    fh_build_GQ<KP>(a, embT, Ct, lane, wave, G, Q);
    __syncthreads();
    for (int q = tid; q < S * S; q += 256) calib_count(a, c, px(b, I, J, q / S, q % S, true, G, Q, en), lane);
}

// Stride 8: one wave per cell, G and Q looked up from the position tables into the wave's rows of Gs [4][4 KP] and Qs [4][16] (LDS)
template <int KP, typename Px>
__device__ __forceinline__ void calib_cell_tab_walk(const FhArgs& a, const CalArgs& c, const float* __restrict__ D,
                                                    const float* __restrict__ N, float* Gs, float* Qs, Px px) {
    constexpr int S = 8;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const long ncell = (long)a.B * cells;
    const long cid = (long)blockIdx.x * 4 + wave;
    const bool ok = cid < ncell;
    const long cc = ok ? cid : 0;
    const int b = (int)(cc / cells), cell = (int)(cc % cells);
    const int I = cell / cells_w, J = cell % cells_w;
    const float* en = a.ws_f + (size_t)a.E * KP;
    float* G = Gs + wave * 4 * KP;
    float* Q = Qs + wave * 16;
    long tp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) tp[t] = tap_pos(b, a.h, a.w, I, J, t);
    fh_lookup_GQ<KP>(tp, D, N, lane, G, Q);
    __syncthreads();
    calib_count(a, c, px(b, I, J, lane / S, lane % S, ok && lane < S * S, G, Q, en), lane);
}

template <int KP>
__global__ __launch_bounds__(256) void calib_cell_kernel(FhArgs a, CalArgs c) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    calib_cell_walk<KP>(a, c, sm, [&](int b, int I, int J, int ty, int tx, bool live, const float* G, const float* Q, const float* en) {
        return calib_pixel<KP, 32>(a, c, b, I, J, ty, tx, live, G, Q, en);
    });
}

template <int KP>
__global__ __launch_bounds__(256) void calib_cell_tab_kernel(FhArgs a, CalArgs c, const float* __restrict__ D,
                                                             const float* __restrict__ N) {
    __shared__ float Gs[4 * 4 * KP];
    __shared__ float Qs[4 * 16];
    calib_cell_tab_walk<KP>(a, c, D, N, Gs, Qs, [&](int b, int I, int J, int ty, int tx, bool live, const float* G, const float* Q, const float* en) {
        return calib_pixel<KP, 8>(a, c, b, I, J, ty, tx, live, G, Q, en);
    });
}

template <int KP>
__global__ __launch_bounds__(256) void sweep_cell_kernel(FhArgs a, CalArgs c, const float* __restrict__ margin) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    calib_cell_walk<KP>(a, c, sm, [&](int b, int I, int J, int ty, int tx, bool live, const float* G, const float* Q, const float* en) {
        return sweep_pixel<KP, 32>(a, c, margin, b, I, J, ty, tx, live, G, Q, en);
    });
}

template <int KP>
__global__ __launch_bounds__(256) void sweep_cell_tab_kernel(FhArgs a, CalArgs c, const float* __restrict__ margin,
                                                             const float* __restrict__ D, const float* __restrict__ N) {
    __shared__ float Gs[4 * 4 * KP];
    __shared__ float Qs[4 * 16];
    calib_cell_tab_walk<KP>(a, c, D, N, Gs, Qs, [&](int b, int I, int J, int ty, int tx, bool live, const float* G, const float* Q, const float* en) {
        return sweep_pixel<KP, 8>(a, c, margin, b, I, J, ty, tx, live, G, Q, en);
    });
}

template <int KP>
__global__ __launch_bounds__(256) void gate_cell_kernel(FhArgs a, CalArgs c, GateArgs g) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    calib_cell_walk<KP>(a, c, sm, [&](int b, int I, int J, int ty, int tx, bool live, const float* G, const float* Q, const float* en) {
        return gate_pixel<KP, 32>(a, c, g, b, I, J, ty, tx, live, G, Q, en);
    });
}

template <int KP>
__global__ __launch_bounds__(256) void gate_cell_tab_kernel(FhArgs a, CalArgs c, GateArgs g, const float* __restrict__ D,
                                                            const float* __restrict__ N) {
    __shared__ float Gs[4 * 4 * KP];
    __shared__ float Qs[4 * 16];
    calib_cell_tab_walk<KP>(a, c, D, N, Gs, Qs, [&](int b, int I, int J, int ty, int tx, bool live, const float* G, const float* Q, const float* en) {
        return gate_pixel<KP, 8>(a, c, g, b, I, J, ty, tx, live, G, Q, en);
    });
}

// ---- hubness correction (szn_hub_stats, szn_hub_head; include/szn.h) --------------------------------------------------------------
// szn_hub_head's pixel kernels: the calibrated head's with calib_pixel<HUB>.  hub_stage: (en[k], scale, shift, 0) of image b's classes
// i0, i0 + step, ... into T [K] (LDS); the walks synchronise before the first pixel reads it
template <int KP>
__device__ __forceinline__ void hub_stage(const FhArgs& a, const float* __restrict__ table, int b, int i0, int step, float4* T) {
    const float* en = a.ws_f + (size_t)a.E * KP;
    const float* tb = table + (size_t)b * a.K * 2;
    for (int k = i0; k < a.K; k += step) T[k] = make_float4(en[k], tb[2 * k], tb[2 * k + 1], 0.f);
}

template <int KP>
__global__ __launch_bounds__(256) void hub_cell_kernel(FhArgs a, CalArgs c, const float* __restrict__ table) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float4* T = (float4*)(sm + fh_lds(a.E, KP, false).Q + 16);            // behind Ct | G | Q: 16 (E + KP + 4) bytes in, 16-byte aligned
    hub_stage<KP>(a, table, blockIdx.x / ((a.h + 1) * (a.w + 1)), threadIdx.x, 256, T);
    calib_cell_walk<KP>(a, c, sm, [&](int b, int I, int J, int ty, int tx, bool live, const float* G, const float* Q, const float* en) {
        return calib_pixel<KP, 32, true>(a, c, b, I, J, ty, tx, live, G, Q, en, T);
    });
}

template <int KP>
__global__ __launch_bounds__(256) void hub_cell_tab_kernel(FhArgs a, CalArgs c, const float* __restrict__ table,
                                                           const float* __restrict__ D, const float* __restrict__ N) {
    __shared__ float Gs[4 * 4 * KP];
    __shared__ float Qs[4 * 16];
    __shared__ float4 Ts[4 * KP];                                         // one image's rows per wave (calib_cell_tab_walk's cell of the wave)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long cells = (long)(a.h + 1) * (a.w + 1), cid = (long)blockIdx.x * 4 + wave;
    float4* T = Ts + wave * KP;
    hub_stage<KP>(a, table, cid < a.B * cells ? (int)(cid / cells) : 0, threadIdx.x & 63, 64, T);
    calib_cell_tab_walk<KP>(a, c, D, N, Gs, Qs, [&](int b, int I, int J, int ty, int tx, bool live, const float* G, const float* Q, const float* en) {
        return calib_pixel<KP, 8, true>(a, c, b, I, J, ty, tx, live, G, Q, en, T);
    });
}

// szn_hub_stats, pass 1: S[b][k] = (sum q, sum q^2) over the counted pixels of image b, q = the similarity in units of 2^-20, and n[b] = their
// number, all int64 and zeroed by the call.  Integers: any order of accumulation gives the same bits.  Classes outermost, eight at a time, so
// a thread holds 24 partial sums, not 2 K: each thread adds its own pixels of the cell for the eight classes, the wave reduces them
// (wave_sum8), one LDS slot per wave, class and moment, and after the loop one 64-bit integer atomic add per block (stride 8: per image
// present in the block), class and moment.  Inside a wave everything fits 32 bits: |q| <= 2^21 and at most 256 pixels per wave give
// |sum q| <= 2^29, and q^2 <= 2^42 travels as its low 20 bits (sum < 2^28) and the rest (sum <= 2^30), put together in 64 bits at the slot.
// SZN_HUB_NO_ACCUM (tools/bench_hub.py builds a second library with it): the walk and the similarities alone, for timing what the
// quantisation, the reductions and the atomics cost; the sums stay zero.
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// The wave's totals of v[0..7] in 10 exchanges instead of 48: three halving steps hand each lane the values its partner keeps (lanes 32, 16,
// 8 apart), three plain steps finish the one value left.  Afterwards every lane holds the total of v[hub_slot(lane)].
__device__ __forceinline__ int wave_sum8(const int (&v)[8], int lane) {
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
    int x[4], y[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = (h5 ? v[4 + i] : v[i]) + __shfl_xor(h5 ? v[i] : v[4 + i], 32, 64);
#pragma unroll
    for (int i = 0; i < 2; ++i) y[i] = (h4 ? x[2 + i] : x[i]) + __shfl_xor(h4 ? x[i] : x[2 + i], 16, 64);
    int z = (h3 ? y[1] : y[0]) + __shfl_xor(h3 ? y[0] : y[1], 8, 64);
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
    return z;
}
__device__ __forceinline__ int hub_slot(int lane) { return ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1); }
// eight classes' partial sums of a lane (s1 = sum q, lo / hi = sum of the low 20 bits / the rest of q^2) -> the wave's totals into the LDS
// slots red [KP][2] of the wave, classes k0 .. k0 + 7 below K
__device__ __forceinline__ void hub_reduce8(const int (&s1)[8], const int (&lo)[8], const int (&hi)[8], int k0, int K, int lane,
                                            long long* red) {
    const int t1 = wave_sum8(s1, lane), tl = wave_sum8(lo, lane), th = wave_sum8(hi, lane);
    const int k = k0 + hub_slot(lane);
    if ((lane & 7) == 0 && k < K) {
        red[k * 2] = t1;
        red[k * 2 + 1] = ((long long)th << 20) + tl;
    }
}
__device__ __forceinline__ void hub_add(long long q, int& s1, int& lo, int& hi) {
    const unsigned long long q2 = (unsigned long long)(q * q);
    s1 += (int)q;
    lo += (int)(q2 & 0xfffffull);
    hi += (int)(q2 >> 20);
}
__device__ __forceinline__ long long hub_q(float sim) {
    const float f = fminf(fmaxf(rintf(sim * 1048576.f), -2097152.f), 2097152.f);      // whole numbers: the clamp commutes with the conversion
    return (long long)f;
}
// Pixel (ty, tx) of cell (I, J) of image b: does it count (inside H x W, not padding, a finite norm > 0)?  Its weights and norm.
template <int S>
__device__ __forceinline__ bool hub_counted(const FhArgs& a, int b, int I, int J, int ty, int tx, bool live, const float* Q,
                                            float (&wt)[4], float& sn) {
    const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;
    cell_weights<S>(ty, tx, wt);
    sn = sqrtf(fh_ss(wt, Q));
    if (!(live && y >= 0 && y < a.H && x >= 0 && x < a.W)) return false;
    if (a.target && a.target[((size_t)b * a.H + y) * a.W + x] == SZN_PAD_LABEL) return false;
    return sn > 0.f && sn < INFINITY;
}

template <int KP>
__global__ __launch_bounds__(256) void hub_stats_cell_kernel(FhArgs a, unsigned long long* __restrict__ Ssum,
                                                             unsigned long long* __restrict__ Ncnt) {    // stride 32: one block per (image, cell)
    constexpr int S = 32;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const FhLds L = fh_lds(a.E, KP, false);
    float* Ct = sm + L.Ct;
    float* G = sm + L.G;
    float* Q = sm + L.Q;
    long long* red = (long long*)(sm + L.Q + 16);            // [4 waves][KP][2], then [4] counts (L.Q + 16 is even: 8-byte aligned)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const int b = blockIdx.x / cells, cell = blockIdx.x % cells;
    const int I = cell / cells_w, J = cell % cells_w;
    const float* embT = a.ws_f;
    const float* en = a.ws_f + (size_t)a.E * KP;
    fh_load_taps(a, b, I, J, tid, Ct);
    __syncthreads();
    fh_build_GQ<KP>(a, embT, Ct, lane, wave, G, Q);
    __syncthreads();
    float wt[4][4], sn[4];
    bool cnt[4];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = tid + 256 * j;
        cnt[j] = hub_counted<S>(a, b, I, J, q / S, q % S, true, Q, wt[j], sn[j]);
        mine += cnt[j] ? 1 : 0;
    }
#ifdef SZN_HUB_NO_ACCUM
    float sink = 0.f;
    for (int k = 0; k < a.K; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) sink = fmaxf(sink, cnt[j] ? fh_sim<KP>(wt[j], G, sn[j], en, k) : 0.f);
    if (sink == 123456.f) Ncnt[b] = (unsigned long long)mine;      // never true (|sim| <= 1): keeps the similarities alive
#else
    for (int k0 = 0; k0 < a.K; k0 += 8) {
        int s1[8], lo[8], hi[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            s1[c] = lo[c] = hi[c] = 0;
            if (k0 + c < a.K)                                      // uniform
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (cnt[j]) hub_add(hub_q(fh_sim<KP>(wt[j], G, sn[j], en, k0 + c)), s1[c], lo[c], hi[c]);
        }
        hub_reduce8(s1, lo, hi, k0, a.K, lane, red + (size_t)wave * KP * 2);
    }
    const long long nw = wave_sum_ll((long long)mine);
    if (lane == 0) red[4 * KP * 2 + wave] = nw;
    __syncthreads();
    for (int i = tid; i < 2 * a.K; i += 256) {
        long long s = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) s += red[v * KP * 2 + i];
        if (s) atomicAdd(Ssum + (size_t)b * a.K * 2 + i, (unsigned long long)s);
    }
    if (tid == 0) {
        const long long n = red[4 * KP * 2] + red[4 * KP * 2 + 1] + red[4 * KP * 2 + 2] + red[4 * KP * 2 + 3];
        if (n) atomicAdd(Ncnt + b, (unsigned long long)n);
    }
#endif
}

// Stride 8: one wave per cell, one pixel per lane; the four cells of a block lie in at most two images (an image has >= 4 cells)
template <int KP>
__global__ __launch_bounds__(256) void hub_stats_cell_tab_kernel(FhArgs a, unsigned long long* __restrict__ Ssum,
                                                                 unsigned long long* __restrict__ Ncnt, const float* __restrict__ D,
                                                                 const float* __restrict__ N) {
    constexpr int S = 8;
    __shared__ float Gs[4 * 4 * KP];
    __shared__ float Qs[4 * 16];
    __shared__ long long red[4 * KP * 2];
    __shared__ long long redn[4];
    __shared__ int bw[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const long ncell = (long)a.B * cells;
    const long cid = (long)blockIdx.x * 4 + wave;
    const bool ok = cid < ncell;
    const long cc = ok ? cid : 0;
    const int b = (int)(cc / cells), cell = (int)(cc % cells);
    const int I = cell / cells_w, J = cell % cells_w;
    const float* en = a.ws_f + (size_t)a.E * KP;
    float* G = Gs + wave * 4 * KP;
    float* Q = Qs + wave * 16;
    long tp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) tp[t] = tap_pos(b, a.h, a.w, I, J, t);
    fh_lookup_GQ<KP>(tp, D, N, lane, G, Q);
    __syncthreads();
    float wt[4], sn;
    const bool cnt = hub_counted<S>(a, b, I, J, lane / S, lane % S, ok, Q, wt, sn);
#ifdef SZN_HUB_NO_ACCUM
    float sink = 0.f;
    for (int k = 0; k < a.K; ++k) sink = fmaxf(sink, cnt ? fh_sim<KP>(wt, G, sn, en, k) : 0.f);
    if (sink == 123456.f) Ncnt[b] = 1ull;                           // never true (|sim| <= 1): keeps the similarities alive
#else
    for (int k0 = 0; k0 < a.K; k0 += 8) {
        int s1[8], lo[8], hi[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            s1[c] = lo[c] = hi[c] = 0;
            if (k0 + c < a.K && cnt) hub_add(hub_q(fh_sim<KP>(wt, G, sn, en, k0 + c)), s1[c], lo[c], hi[c]);
        }
        hub_reduce8(s1, lo, hi, k0, a.K, lane, red + (size_t)wave * KP * 2);
    }
    const long long nw = wave_sum_ll(cnt ? 1ll : 0ll);
    if (lane == 0) { redn[wave] = nw; bw[wave] = ok ? b : -1; }
    __syncthreads();
    const int b0 = bw[0];                                           // wave 0's cell always exists
    for (int i = tid; i < 2 * a.K; i += 256) {
        long long s0 = 0, s1 = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const long long r = red[v * KP * 2 + i];
            if (bw[v] == b0) s0 += r;
            else if (bw[v] >= 0) s1 += r;
        }
        if (s0) atomicAdd(Ssum + (size_t)b0 * a.K * 2 + i, (unsigned long long)s0);
        if (s1) atomicAdd(Ssum + (size_t)(b0 + 1) * a.K * 2 + i, (unsigned long long)s1);
    }
    if (tid == 0) {
        long long n0 = 0, n1 = 0;
        for (int v = 0; v < 4; ++v) {
            if (bw[v] == b0) n0 += redn[v];
            else if (bw[v] >= 0) n1 += redn[v];
        }
        if (n0) atomicAdd(Ncnt + b0, (unsigned long long)n0);
        if (n1) atomicAdd(Ncnt + b0 + 1, (unsigned long long)n1);
    }
#endif
}

// szn_hub_stats, pass 2: one thread per (image, class), double arithmetic: the moments and the (scale, shift) row of the mode
__global__ __launch_bounds__(256) void hub_table_kernel(const long long* __restrict__ Ssum, const long long* __restrict__ Ncnt, int B, int K,
                                                        int mode, double beta, double min_sd, float* __restrict__ table,
                                                        int64_t* __restrict__ sums, int64_t* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * K) return;
    const int b = i / K;
    const long long n = Ncnt[b], s1 = Ssum[2 * (size_t)i], s2 = Ssum[2 * (size_t)i + 1];
    float scale = 1.f, shift = 0.f;
    if (n > 0) {
        const double mean = (double)s1 / ((double)n * 1048576.0);
        const double ex2 = (double)s2 / ((double)n * 1099511627776.0);
        const double sd = sqrt(fmax(ex2 - mean * mean, 0.0));
        if (mode == 0) shift = (float)(beta * mean);
        else {
            const double f = fmax(sd, min_sd);
            scale = (float)(1.0 / f);
            shift = (float)(beta * mean / f);
        }
    }
    table[2 * (size_t)i] = scale;
    table[2 * (size_t)i + 1] = shift;
    if (sums) { sums[2 * (size_t)i] = s1; sums[2 * (size_t)i + 1] = s2; }
    if (counts && i % K == 0) counts[b] = n;
}

// workspace of szn_hub_stats: the fused head's | S [B][K][2] int64 | n [B] int64
struct HubWorkspace { size_t S, n, bytes; };       // byte offsets
inline HubWorkspace hub_workspace(int B, int h, int w, int E, int K) {
    HubWorkspace L;
    L.S = align256(fh_workspace(B, h, w, E, kp_of(K)).bytes);
    L.n = L.S + (size_t)B * K * 2 * sizeof(long long);
    L.bytes = L.n + (size_t)B * sizeof(long long);
    return L;
}

template <int KP>
void hub_stats_launch(int stride, const FhArgs& a, unsigned long long* S, unsigned long long* n, float* tabD, float* tabN, hipStream_t st) {
    const int cells = (a.h + 1) * (a.w + 1);
    if (stride == 8) {
        hipLaunchKernelGGL(fh_tables_kernel<KP>, dim3((unsigned)(((long)a.B * a.h * a.w + 3) / 4)), dim3(256),
                           (size_t)4 * a.E * sizeof(float), st, a, tabD, tabN);
        hipLaunchKernelGGL(hub_stats_cell_tab_kernel<KP>, dim3((unsigned)(((long)a.B * cells + 3) / 4)), dim3(256), 0, st, a, S, n,
                           (const float*)tabD, (const float*)tabN);
    } else {
        const size_t lds = (size_t)(fh_lds(a.E, KP, false).Q + 16) * sizeof(float) + ((size_t)4 * KP * 2 + 4) * sizeof(long long);
        auto kern = hub_stats_cell_kernel<KP>;
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(a.B * cells), dim3(256), lds, st, a, S, n);
    }
}

// hub: szn_hub_head's pixel kernels; else gate: szn_soft_gate_head's; else margin == nullptr: szn_calib_head's; else szn_seen_sweep_head's -- same
// grids and LDS.
// tabled: the stride-8 position tables are in the workspace already (szn_seen_sweep_head_tabled, szn_soft_gate_head_tabled)
template <int KP>
void calib_launch(int stride, const FhArgs& a, const CalArgs& c, const float* margin, const GateArgs* gate, bool tabled, float* tabD,
                  float* tabN, hipStream_t st, const float* hub = nullptr) {
    const int cells = (a.h + 1) * (a.w + 1);
    if (stride == 8) {
        const dim3 grid((unsigned)(((long)a.B * cells + 3) / 4));
        if (!tabled) hipLaunchKernelGGL(fh_tables_kernel<KP>, dim3((unsigned)(((long)a.B * a.h * a.w + 3) / 4)), dim3(256),
                                        (size_t)4 * a.E * sizeof(float), st, a, tabD, tabN);
        if (hub) hipLaunchKernelGGL(hub_cell_tab_kernel<KP>, grid, dim3(256), 0, st, a, c, hub, (const float*)tabD, (const float*)tabN);
        else if (gate) hipLaunchKernelGGL(gate_cell_tab_kernel<KP>, grid, dim3(256), 0, st, a, c, *gate, (const float*)tabD, (const float*)tabN);
        else if (margin) hipLaunchKernelGGL(sweep_cell_tab_kernel<KP>, grid, dim3(256), 0, st, a, c, margin, (const float*)tabD, (const float*)tabN);
        else hipLaunchKernelGGL(calib_cell_tab_kernel<KP>, grid, dim3(256), 0, st, a, c, (const float*)tabD, (const float*)tabN);
    } else {
        const size_t lds = (size_t)(fh_lds(a.E, KP, false).Q + 16) * sizeof(float);       // Ct | G | Q
        if (hub) {
            auto kern = hub_cell_kernel<KP>;
            const size_t hlds = lds + (size_t)KP * sizeof(float4);                      // + the staged table rows
            if (hlds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hlds);
            hipLaunchKernelGGL(kern, dim3(a.B * cells), dim3(256), hlds, st, a, c, hub);
        } else if (gate) {
            auto kern = gate_cell_kernel<KP>;
            if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, dim3(a.B * cells), dim3(256), lds, st, a, c, *gate);
        } else if (margin) {
            auto kern = sweep_cell_kernel<KP>;
            if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, dim3(a.B * cells), dim3(256), lds, st, a, c, margin);
        } else {
            auto kern = calib_cell_kernel<KP>;
            if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, dim3(a.B * cells), dim3(256), lds, st, a, c);
        }
    }
}

// workspace of szn_calib_head: the fused head's (embedding tables at its head, the stride-8 position tables) | XA | XB
struct CalWorkspace { size_t XA, XB, bytes; };       // byte offsets
inline CalWorkspace calib_workspace(int B, int h, int w, int E, int K, int n) {
    CalWorkspace L;
    const size_t tab = (size_t)K * K * (n + 1) * sizeof(unsigned long long);
    L.XA = align256(fh_workspace(B, h, w, E, kp_of(K)).bytes);
    L.XB = L.XA + tab;
    L.bytes = L.XB + tab;
    return L;
}

// what szn_calib_head and its workspace query refuse about sizes; 0 = fine
const char* calib_bad_geometry(int stride, int B, int h, int w, int E, int K, int n_gammas) {
    if (stride != 32 && stride != 8) return "stride must be 8 or 32";
    if (n_gammas < 1 || n_gammas > SZN_CALIB_MAX_GAMMAS) return "n_gammas outside [1, SZN_CALIB_MAX_GAMMAS]";
    if (B <= 0 || h <= 0 || w <= 0 || E <= 0 || K <= 0) return "a size that is not positive";
    if (K > SZN_MAX_CLASSES) return "K above SZN_MAX_CLASSES";
    return nullptr;
}

// ---- self-training pseudo labels (szn_pseudo_head): the calibrated head's per-pixel quantities, a per-class confidence histogram,
// an on-device threshold search, a relabel pass ------------------------------------------------------------------------------------------
// Pass 1 (pseudo_cell_kernel / pseudo_cell_tab_kernel: calib_cell_kernel / calib_cell_tab_kernel with another per-pixel body) looks at
// the pixels whose target is cand_label only -- every other pixel skips the trip through the classes -- and leaves per pixel a record
// {class or -1, confidence bits} in the workspace (8 B); candidates add 1 to QH[class][bin], equal keys of a wave combined first
// (calib_count's scheme, one 64-bit integer atomic add per distinct key).  Pass 2 (pseudo_thr_kernel): one block per class, a suffix
// scan over the 1024 bins.  Pass 3 (pseudo_relabel_kernel): elementwise over the records.  Integers throughout: bit-reproducible.
struct PseudoArgs {
    float gamma, conf_floor;
    long cand_label;
    unsigned long long* QH;      // [K][SZN_PSEUDO_BINS], zeroed by the call
    int2* rec;                   // [B][H][W]: x = the candidate's class or -1, y = the bits of its confidence (NaN: none)
};

// bin of a confidence: clamp(floor(c * 512 + 512), 0, 1023); c * 512 is exact, so the fma is the two-step form's bits
__device__ __forceinline__ int pseudo_bin(float c) {
    return (int)fminf(fmaxf(floorf(fmaf(c, 512.f, 512.f)), 0.f), (float)(SZN_PSEUDO_BINS - 1));
}

// Pixel (ty, tx) of cell (I, J) of image b: its record, and its key class << 10 | bin, or -1 where it is no candidate
template <int KP, int S>
__device__ __forceinline__ int pseudo_pixel(const FhArgs& a, const PseudoArgs& p, int b, int I, int J, int ty, int tx, bool live,
                                            const float* G, const float* Q, const float* __restrict__ en) {
    const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;
    if (!(live && y >= 0 && y < a.H && x >= 0 && x < a.W)) return -1;
    const size_t pix = ((size_t)b * a.H + y) * a.W + x;
    int cls = -1;
    float conf = __int_as_float(0x7fc00000);
    if (a.target[pix] == p.cand_label) {
        float wt[4];
        cell_weights<S>(ty, tx, wt);
        const float sn = sqrtf(fh_ss(wt, Q));
        const FhTwoBest r = fh_two_best<KP>(a, wt, G, sn, en);
        const float m = r.va - r.vb;
        const bool takes_a = m > p.gamma || (m == p.gamma && r.ia < r.ib);         // szn_calib_head's rule at this gamma
        if (m == m && !takes_a && (p.conf_floor <= -2.f || r.vb >= p.conf_floor)) { cls = r.ib; conf = r.vb; }
    }
    p.rec[pix] = make_int2(cls, __float_as_int(conf));
    return cls < 0 ? -1 : (cls << 10 | pseudo_bin(conf));
}

// the keys of a wave, equal ones combined: one atomic add of the popcount per distinct key (the key is the index into QH)
__device__ __forceinline__ void pseudo_count(const PseudoArgs& p, int key, int lane) {
    static_assert(SZN_PSEUDO_BINS == 1 << 10, "the key packs the bin into 10 bits");
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const int k0 = __shfl(key, src, 64);
        const unsigned long long same = __ballot(key == k0);
        if (lane == src) atomicAdd(p.QH + k0, (unsigned long long)__popcll(same));
        todo &= ~same;
    }
}

template <int KP>
__global__ __launch_bounds__(256) void pseudo_cell_kernel(FhArgs a, PseudoArgs p) {      // stride 32: one block per (image, cell)
    constexpr int S = 32;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const FhLds L = fh_lds(a.E, KP, false);
    float* Ct = sm + L.Ct;
    float* G = sm + L.G;
    float* Q = sm + L.Q;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const int b = blockIdx.x / cells, cell = blockIdx.x % cells;
    const int I = cell / cells_w, J = cell % cells_w;
    const float* embT = a.ws_f;
    const float* en = a.ws_f + (size_t)a.E * KP;
    fh_load_taps(a, b, I, J, tid, Ct);
    __syncthreads();
    fh_build_GQ<KP>(a, embT, Ct, lane, wave, G, Q);
    __syncthreads();
    for (int q = tid; q < S * S; q += 256)
        pseudo_count(p, pseudo_pixel<KP, S>(a, p, b, I, J, q / S, q % S, true, G, Q, en), lane);
}

template <int KP>
__global__ __launch_bounds__(256) void pseudo_cell_tab_kernel(FhArgs a, PseudoArgs p, const float* __restrict__ D,
                                                              const float* __restrict__ N) {      // stride 8: one wave per cell
    constexpr int S = 8;
    __shared__ float Gs[4][4 * KP];
    __shared__ float Qs[4][16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const long ncell = (long)a.B * cells;
    const long cid = (long)blockIdx.x * 4 + wave;
    const bool ok = cid < ncell;
    const long cc = ok ? cid : 0;
    const int b = (int)(cc / cells), cell = (int)(cc % cells);
    const int I = cell / cells_w, J = cell % cells_w;
    const float* en = a.ws_f + (size_t)a.E * KP;
    long tp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) tp[t] = tap_pos(b, a.h, a.w, I, J, t);
    fh_lookup_GQ<KP>(tp, D, N, lane, Gs[wave], Qs[wave]);
    __syncthreads();
    pseudo_count(p, pseudo_pixel<KP, S>(a, p, b, I, J, lane / S, lane % S, ok && lane < S * S, Gs[wave], Qs[wave], en), lane);
}

// Class k = blockIdx.x: n = sum_q QH[k][q], keep = ceil(n * keep_permille / 1000), thr = the largest bin t whose suffix sum
// sum_{q >= t} QH[k][q] reaches keep (SZN_PSEUDO_BINS when n == 0), counts = {n, that suffix sum}.  Thread t owns bins 4 t .. 4 t + 3;
// an inclusive suffix scan of the 256 partial sums in LDS, then every thread tests its own four bins: the suffix sums fall with t
// from n >= keep to 0 < keep, so exactly one bin has its own sum at or above keep and its successor's below.
__global__ __launch_bounds__(256) void pseudo_thr_kernel(const unsigned long long* __restrict__ QH, int keep_permille,
                                                         int32_t* __restrict__ thr_ws, int64_t* __restrict__ qhist,
                                                         int32_t* __restrict__ thr, int64_t* __restrict__ counts) {
    static_assert(SZN_PSEUDO_BINS == 4 * 256, "four bins per thread");
    __shared__ unsigned long long suf[257];
    const int k = blockIdx.x, t = threadIdx.x;
    const unsigned long long* row = QH + (size_t)k * SZN_PSEUDO_BINS;
    unsigned long long v[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = row[4 * t + i];
        s += v[i];
        if (qhist) qhist[(size_t)k * SZN_PSEUDO_BINS + 4 * t + i] = (int64_t)v[i];
    }
    suf[t] = s;
    if (t == 0) suf[256] = 0;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const unsigned long long add = (t + d < 256) ? suf[t + d] : 0;
        __syncthreads();
        suf[t] += add;
        __syncthreads();
    }
    const unsigned long long n = suf[0];
    const unsigned long long keep = (n * (unsigned long long)keep_permille + 999) / 1000;
    if (n == 0) {
        if (t == 0) {
            thr_ws[k] = SZN_PSEUDO_BINS;
            if (thr) thr[k] = SZN_PSEUDO_BINS;
            if (counts) { counts[2 * k] = 0; counts[2 * k + 1] = 0; }
        }
        return;
    }
    unsigned long long above = suf[t + 1];              // the suffix sum from the first bin of the next thread on
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        const unsigned long long next = above;
        above += v[i];                                   // the suffix sum from bin 4 t + i on
        if (above >= keep && next < keep) {
            thr_ws[k] = 4 * t + i;
            if (thr) thr[k] = 4 * t + i;
            if (counts) { counts[2 * k] = (int64_t)n; counts[2 * k + 1] = (int64_t)above; }
        }
    }
}

// target_out = the candidate's class where its bin reaches its class's threshold, else the target verbatim; the inspection copies
__global__ __launch_bounds__(256) void pseudo_relabel_kernel(const int64_t* __restrict__ target, const int2* __restrict__ rec,
                                                             const int32_t* __restrict__ thr_ws, long n,
                                                             int64_t* __restrict__ target_out, int64_t* __restrict__ cand,
                                                             float* __restrict__ conf) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int2 r = rec[i];
    const float c = __int_as_float(r.y);
    int64_t lbl = target[i];
    if (r.x >= 0 && pseudo_bin(c) >= thr_ws[r.x]) lbl = r.x;
    target_out[i] = lbl;
    if (cand) cand[i] = r.x;
    if (conf) conf[i] = c;
}

template <int KP>
void pseudo_launch(int stride, const FhArgs& a, const PseudoArgs& p, float* tabD, float* tabN, hipStream_t st) {
    const int cells = (a.h + 1) * (a.w + 1);
    if (stride == 8) {
        hipLaunchKernelGGL(fh_tables_kernel<KP>, dim3((unsigned)(((long)a.B * a.h * a.w + 3) / 4)), dim3(256),
                           (size_t)4 * a.E * sizeof(float), st, a, tabD, tabN);
        hipLaunchKernelGGL(pseudo_cell_tab_kernel<KP>, dim3((unsigned)(((long)a.B * cells + 3) / 4)), dim3(256), 0, st, a, p,
                           (const float*)tabD, (const float*)tabN);
    } else {
        const size_t lds = (size_t)(fh_lds(a.E, KP, false).Q + 16) * sizeof(float);       // Ct | G | Q
        auto kern = pseudo_cell_kernel<KP>;
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(a.B * cells), dim3(256), lds, st, a, p);
    }
}

// workspace of szn_pseudo_head: the fused head's (embedding tables at its head, the stride-8 position tables) | QH | thr | rec
struct PseudoWorkspace { size_t QH, thr, rec, bytes; };       // byte offsets
inline PseudoWorkspace pseudo_workspace(int B, int h, int w, int E, int K, int H, int W) {
    PseudoWorkspace L;
    L.QH = align256(fh_workspace(B, h, w, E, kp_of(K)).bytes);
    L.thr = L.QH + (size_t)K * SZN_PSEUDO_BINS * sizeof(unsigned long long);
    L.rec = align256(L.thr + (size_t)K * sizeof(int32_t));
    L.bytes = L.rec + (size_t)B * H * W * sizeof(int2);
    return L;
}

// what every head of this family refuses about channels, the crop window and the workspace alignment (szn_ohem_head shares this much)
int calib_check_window(const char* who, int stride, int h, int w, int E, int ldc, int c0, int H, int W, int crop, const void* workspace) {
    if (c0 < 0 || ldc < c0 + E || H <= 0 || W <= 0 || crop < 0) SZN_FAIL(SZN_ERR_ARG, "%s: bad argument", who);
    if (H + crop > stride * h + stride || W + crop > stride * w + stride)
        SZN_FAIL(SZN_ERR_ARG, "%s: crop window exceeds the deconv output", who);
    if (((uintptr_t)workspace) & 15) SZN_FAIL(SZN_ERR_ARG, "%s: workspace must be 16-B aligned", who);
    return SZN_OK;
}
// what szn_calib_head and szn_pseudo_head refuse about the arguments they share (after calib_bad_geometry); SZN_OK = fine
int calib_check_shared(const char* who, int stride, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                       const ClassBits& ubits, const void* workspace) {
    if (int rc = calib_check_window(who, stride, h, w, E, ldc, c0, H, W, crop, workspace)) return rc;
    if (!class_bits_any(ubits)) SZN_FAIL(SZN_ERR_ARG, "%s: the unseen set is empty", who);
    if (!class_bits_fit(ubits, K)) SZN_FAIL(SZN_ERR_ARG, "%s: the unseen set names a class >= K = %d", who, K);
    int n_unseen = 0;
    for (int i = 0; i < 4; ++i) n_unseen += __builtin_popcountll(ubits.w[i]);
    if (n_unseen >= K) SZN_FAIL(SZN_ERR_ARG, "%s: every class below K = %d is unseen (both groups must be non-empty)", who, K);
    if (fh_lds(E, kp_of(K), false).bytes() > 150 * 1024) SZN_FAIL(SZN_ERR_UNSUPPORTED, "%s: E=%d too large for LDS", who, E);
    return SZN_OK;
}

// ---- hard-pixel mining (szn_ohem_head): the own-class cosine of every labelled pixel, a per-image histogram, an on-device cut, a
// relabel pass ----------------------------------------------------------------------------------------------------------------------
// Pass 1 (ohem_cell_kernel / ohem_cell_tab_kernel: the pseudo cell kernels with another per-pixel body) evaluates the pixels whose label
// is a class outside `skip` -- one class per pixel, fh_pixel's cosine term -- and leaves the cosine's bits per pixel in the workspace
// (4 B; NaN: not evaluated, or a zero norm: both keep their label).  This pass sees every labelled pixel and a wave's cosines fall into
// dozens of bins, so combining equal keys per wave would still issue about one global atomic per pixel: the bins are counted in LDS first
// (stride 32: the block is one cell of one image, one table; stride 8: the block's four cells touch at most two images, one table each)
// and every non-empty LDS bin becomes one 64-bit integer atomic add on QH[image][bin].  Pass 2 (ohem_cut_kernel): one block per image, a
// prefix scan over the 1024 bins.  Pass 3 (ohem_relabel_kernel): elementwise over the records.  Integers throughout: bit-reproducible.
static_assert(SZN_OHEM_BINS == SZN_PSEUDO_BINS, "pseudo_bin is the bin of both heads");
struct OhemArgs {
    ClassBits skip;              // labels the head ignores (sim_ce's exclude set): not evaluated, passed through
    unsigned long long* QH;      // [B][SZN_OHEM_BINS], zeroed by the call
    float* rec;                  // [B][H][W]: the pixel's own-class cosine, NaN where it was not evaluated
};

// Pixel (ty, tx) of cell (I, J) of image b: its record, and its bin, or -1 where it is not evaluated
template <int KP, int S>
__device__ __forceinline__ int ohem_pixel(const FhArgs& a, const OhemArgs& p, int b, int I, int J, int ty, int tx, bool live,
                                          const float* G, const float* Q, const float* __restrict__ ent) {
    const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;
    if (!(live && y >= 0 && y < a.H && x >= 0 && x < a.W)) return -1;
    const size_t pix = ((size_t)b * a.H + y) * a.W + x;
    const long lbl = a.target[pix];
    int q = -1;
    float c = __int_as_float(0x7fc00000);
    if (lbl >= 0 && lbl < a.K && !in_set(p.skip, lbl)) {
        float wt[4];
        cell_weights<S>(ty, tx, wt);
        const float sn = sqrtf(fh_ss(wt, Q));
        const int kl = (int)lbl;
        float d = 0.f;                                                     // fh_pixel's cosine term, operation for operation
#pragma unroll
        for (int t = 0; t < 4; ++t) d = fmaf(wt[t], G[t * KP + kl], d);
        c = d / (sn * ent[kl]);
        q = (c == c) ? pseudo_bin(c) : 0;
    }
    p.rec[pix] = c;
    return q;
}

template <int KP>
__global__ __launch_bounds__(256) void ohem_cell_kernel(FhArgs a, OhemArgs p) {      // stride 32: one block per (image, cell)
    constexpr int S = 32;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const FhLds L = fh_lds(a.E, KP, false);
    float* Ct = sm + L.Ct;
    float* G = sm + L.G;
    float* Q = sm + L.Q;
    unsigned int* hist = (unsigned int*)(sm + L.Aw);                      // [SZN_OHEM_BINS], behind Ct | G | Q
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const int b = blockIdx.x / cells, cell = blockIdx.x % cells;
    const int I = cell / cells_w, J = cell % cells_w;
    const float* embT = a.ws_f;
    const float* ent = a.ws_f + (size_t)a.E * KP + KP;
    for (int i = tid; i < SZN_OHEM_BINS; i += 256) hist[i] = 0u;
    fh_load_taps(a, b, I, J, tid, Ct);
    __syncthreads();
    fh_build_GQ<KP>(a, embT, Ct, lane, wave, G, Q);
    __syncthreads();
    for (int q = tid; q < S * S; q += 256) {
        const int bin = ohem_pixel<KP, S>(a, p, b, I, J, q / S, q % S, true, G, Q, ent);
        if (bin >= 0) atomicAdd(hist + bin, 1u);
    }
    __syncthreads();
    for (int i = tid; i < SZN_OHEM_BINS; i += 256) {
        const unsigned int v = hist[i];
        if (v) atomicAdd(p.QH + (size_t)b * SZN_OHEM_BINS + i, (unsigned long long)v);
    }
}

template <int KP>
__global__ __launch_bounds__(256) void ohem_cell_tab_kernel(FhArgs a, OhemArgs p, const float* __restrict__ D,
                                                            const float* __restrict__ N) {      // stride 8: one wave per cell
    constexpr int S = 8;
    __shared__ float Gs[4][4 * KP];
    __shared__ float Qs[4][16];
    __shared__ unsigned int hist[2][SZN_OHEM_BINS];       // the image of the block's first cell, and the next one
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;          // >= 4: four consecutive cells touch at most two images
    const long ncell = (long)a.B * cells;
    const long cid = (long)blockIdx.x * 4 + wave;
    const bool ok = cid < ncell;
    const long cc = ok ? cid : 0;
    const int b = (int)(cc / cells), cell = (int)(cc % cells);
    const int b0 = (int)(((long)blockIdx.x * 4) / cells);
    const int I = cell / cells_w, J = cell % cells_w;
    const float* ent = a.ws_f + (size_t)a.E * KP + KP;
    long tp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) tp[t] = tap_pos(b, a.h, a.w, I, J, t);
    for (int i = threadIdx.x; i < 2 * SZN_OHEM_BINS; i += 256) (&hist[0][0])[i] = 0u;
    fh_lookup_GQ<KP>(tp, D, N, lane, Gs[wave], Qs[wave]);
    __syncthreads();
    const int bin = ohem_pixel<KP, S>(a, p, b, I, J, lane / S, lane % S, ok && lane < S * S, Gs[wave], Qs[wave], ent);
    if (bin >= 0) atomicAdd(&hist[b - b0][bin], 1u);                   // bin >= 0 only where ok: b is b0 or b0 + 1
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * SZN_OHEM_BINS; i += 256) {
        const unsigned int v = (&hist[0][0])[i];
        if (v) atomicAdd(p.QH + (size_t)b0 * SZN_OHEM_BINS + i, (unsigned long long)v);      // v > 0 in the second table: b0 + 1 < B
    }
}

// Image b = blockIdx.x: n = sum_q QH[b][q], keep = ceil(n * keep_permille / 1000), tmin = the smallest t in [1, 1024] whose prefix sum
// P(t) = sum_{q < t} QH[b][q] reaches keep, cut = max(tmin, tbin) (0 when n == 0), counts = {n, P(cut)}.  Thread t owns bins
// 4 t .. 4 t + 3; an inclusive prefix scan of the 256 partial sums in LDS, then every thread tests its own four bins: P rises with t
// from P(0) = 0 < keep to P(1024) = n >= keep, so exactly one t has P(t) >= keep and P(t - 1) < keep.
__global__ __launch_bounds__(256) void ohem_cut_kernel(const unsigned long long* __restrict__ QH, int keep_permille, float thresh,
                                                       int32_t* __restrict__ cut_ws, int64_t* __restrict__ qhist,
                                                       int32_t* __restrict__ cut, int64_t* __restrict__ counts) {
    static_assert(SZN_OHEM_BINS == 4 * 256, "four bins per thread");
    __shared__ unsigned long long pre[257];
    __shared__ int s_tmin;
    const int b = blockIdx.x, t = threadIdx.x;
    const unsigned long long* row = QH + (size_t)b * SZN_OHEM_BINS;
    unsigned long long v[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = row[4 * t + i];
        s += v[i];
        if (qhist) qhist[(size_t)b * SZN_OHEM_BINS + 4 * t + i] = (int64_t)v[i];
    }
    pre[t + 1] = s;
    if (t == 0) pre[0] = 0;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const unsigned long long add = (t + 1 > d) ? pre[t + 1 - d] : 0;
        __syncthreads();
        pre[t + 1] += add;
        __syncthreads();
    }
    const unsigned long long n = pre[256];
    if (n == 0) {
        if (t == 0) {
            cut_ws[b] = 0;
            if (cut) cut[b] = 0;
            if (counts) { counts[2 * b] = 0; counts[2 * b + 1] = 0; }
        }
        return;
    }
    const unsigned long long keep = (n * (unsigned long long)keep_permille + 999) / 1000;
    unsigned long long below = pre[t];                  // P(4 t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned long long prev = below;
        below += v[i];                                   // P(4 t + i + 1)
        if (below >= keep && prev < keep) s_tmin = 4 * t + i + 1;
    }
    __syncthreads();
    // thresh rounded down to a bin edge; thresh * 512 is exact, so the fma is the two-step form's bits
    const int tbin = (int)fminf(fmaxf(floorf(fmaf(thresh, 512.f, 512.f)), 0.f), (float)SZN_OHEM_BINS);
    const int c = max(s_tmin, tbin);                     // in [1, 1024]
    if (t == (c - 1) >> 2) {
        unsigned long long kept = pre[t];
        for (int i = 0; i <= ((c - 1) & 3); ++i) kept += v[i];
        cut_ws[b] = c;
        if (cut) cut[b] = c;
        if (counts) { counts[2 * b] = (int64_t)n; counts[2 * b + 1] = (int64_t)kept; }
    }
}

// target_out = drop_label where the pixel was evaluated and its bin reaches its image's cut, else the target verbatim; conf = the record.
// Four pixels per thread; VEC (every pointer 16-byte aligned, H * W >= 4): 16-byte accesses on all whole groups of four.
__device__ __forceinline__ int64_t ohem_relabel_one(int64_t lbl, float c, int cut, int64_t drop_label) {
    return (c == c && pseudo_bin(c) >= cut) ? drop_label : lbl;
}
template <bool VEC>
__global__ __launch_bounds__(256) void ohem_relabel_kernel(const int64_t* __restrict__ target, const float* __restrict__ rec,
                                                           const int32_t* __restrict__ cut_ws, long n, long hw, int64_t drop_label,
                                                           int64_t* __restrict__ target_out, float* __restrict__ conf) {
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    if (VEC && i0 + 4 <= n) {
        const float4 c = *(const float4*)(rec + i0);
        const longlong2 l0 = *(const longlong2*)(target + i0), l1 = *(const longlong2*)(target + i0 + 2);
        const long ba = i0 / hw, next = (ba + 1) * hw;       // hw >= 4 (host): the four pixels belong to image ba or ba + 1
        const int ca = cut_ws[ba], cb = (i0 + 3 >= next) ? cut_ws[ba + 1] : ca;
        longlong2 o0, o1;
        o0.x = ohem_relabel_one(l0.x, c.x, ca, drop_label);
        o0.y = ohem_relabel_one(l0.y, c.y, i0 + 1 >= next ? cb : ca, drop_label);
        o1.x = ohem_relabel_one(l1.x, c.z, i0 + 2 >= next ? cb : ca, drop_label);
        o1.y = ohem_relabel_one(l1.y, c.w, cb, drop_label);
        *(longlong2*)(target_out + i0) = o0;
        *(longlong2*)(target_out + i0 + 2) = o1;
        if (conf) *(float4*)(conf + i0) = c;
        return;
    }
    for (long i = i0; i < n && i < i0 + 4; ++i) {
        const float c = rec[i];
        target_out[i] = ohem_relabel_one(target[i], c, cut_ws[i / hw], drop_label);
        if (conf) conf[i] = c;
    }
}

template <int KP>
void ohem_launch(int stride, const FhArgs& a, const OhemArgs& p, float* tabD, float* tabN, hipStream_t st) {
    const int cells = (a.h + 1) * (a.w + 1);
    if (stride == 8) {
        hipLaunchKernelGGL(fh_tables_kernel<KP>, dim3((unsigned)(((long)a.B * a.h * a.w + 3) / 4)), dim3(256),
                           (size_t)4 * a.E * sizeof(float), st, a, tabD, tabN);
        hipLaunchKernelGGL(ohem_cell_tab_kernel<KP>, dim3((unsigned)(((long)a.B * cells + 3) / 4)), dim3(256), 0, st, a, p,
                           (const float*)tabD, (const float*)tabN);
    } else {
        const size_t lds = (size_t)(fh_lds(a.E, KP, false).Aw + SZN_OHEM_BINS) * sizeof(float);       // Ct | G | Q | hist
        auto kern = ohem_cell_kernel<KP>;
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(a.B * cells), dim3(256), lds, st, a, p);
    }
}

// workspace of szn_ohem_head: the fused head's (embedding tables at its head, the stride-8 position tables) | QH | cut | rec
struct OhemWorkspace { size_t QH, cut, rec, bytes; };       // byte offsets
inline OhemWorkspace ohem_workspace(int B, int h, int w, int E, int K, int H, int W) {
    OhemWorkspace L;
    L.QH = align256(fh_workspace(B, h, w, E, kp_of(K)).bytes);
    L.cut = L.QH + (size_t)B * SZN_OHEM_BINS * sizeof(unsigned long long);
    L.rec = align256(L.cut + (size_t)B * sizeof(int32_t));
    L.bytes = L.rec + (size_t)B * H * W * sizeof(float);
    return L;
}

// the cell pass: stride 32 a block per cell; stride 8 the position tables, then a wave per cell
template <int KP, bool GROUPED, bool MSE>
void fh_launch(int stride, const FhArgs& a, float* tabD, float* tabN, hipStream_t st) {
    const int cells = (a.h + 1) * (a.w + 1);
    if (stride == 8) {
        hipLaunchKernelGGL(fh_tables_kernel<KP>, dim3((unsigned)(((long)a.B * a.h * a.w + 3) / 4)), dim3(256),
                           (size_t)4 * a.E * sizeof(float), st, a, tabD, tabN);
        hipLaunchKernelGGL((fh_cell_tab_kernel<KP, 8, GROUPED, MSE>), dim3((unsigned)(((long)a.B * cells + 3) / 4)), dim3(256), 0, st, a,
                           (const float*)tabD, (const float*)tabN);
    } else {
        const size_t lds = fh_lds(a.E, KP, MSE).bytes();
        auto kern = fh_cell_kernel<KP, 32, GROUPED, MSE>;
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(a.B * cells), dim3(256), lds, st, a);
    }
}
template <int KP>
void fh_launch_kp(bool grouped, bool mse, int stride, const FhArgs& a, float* tabD, float* tabN, hipStream_t st) {
    if (grouped) mse ? fh_launch<KP, true, true>(stride, a, tabD, tabN, st) : fh_launch<KP, true, false>(stride, a, tabD, tabN, st);
    else mse ? fh_launch<KP, false, true>(stride, a, tabD, tabN, st) : fh_launch<KP, false, false>(stride, a, tabD, tabN, st);
}

// the similarity cross-entropy and ranking cell pass: the same two shapes; the LDS is dynamic at both strides (the tiles take it past 48 KB)
template <int KP, bool GROUPED, class LA>
void sce_launch(int stride, const FhArgs& a, const LA& s, float* tabD, float* tabN, hipStream_t st) {
    const int cells = (a.h + 1) * (a.w + 1);
    const size_t lds = sce_lds_floats(stride, a.E, KP) * sizeof(float);
    if (stride == 8) {
        hipLaunchKernelGGL(fh_tables_kernel<KP>, dim3((unsigned)(((long)a.B * a.h * a.w + 3) / 4)), dim3(256),
                           (size_t)4 * a.E * sizeof(float), st, a, tabD, tabN);
        auto kern = sce_cell_tab_kernel<KP, GROUPED, LA>;
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3((unsigned)(((long)a.B * cells + 3) / 4)), dim3(256), lds, st, a, s, (const float*)tabD,
                           (const float*)tabN);
    } else {
        auto kern = sce_cell_kernel<KP, GROUPED, LA>;
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(a.B * cells), dim3(256), lds, st, a, s);
    }
}
template <int KP, class LA>
void sce_launch_kp(bool grouped, int stride, const FhArgs& a, const LA& s, float* tabD, float* tabN, hipStream_t st) {
    grouped ? sce_launch<KP, true>(stride, a, s, tabD, tabN, st) : sce_launch<KP, false>(stride, a, s, tabD, tabN, st);
}
template <class LA>
void sce_launch_k(int KP, bool grouped, int stride, const FhArgs& a, const LA& s, float* tabD, float* tabN, hipStream_t st) {
    switch (KP) {
        case 24: sce_launch_kp<24>(grouped, stride, a, s, tabD, tabN, st); break;
        case 40: sce_launch_kp<40>(grouped, stride, a, s, tabD, tabN, st); break;
        case 64: sce_launch_kp<64>(grouped, stride, a, s, tabD, tabN, st); break;
        case 128: sce_launch_kp<128>(grouped, stride, a, s, tabD, tabN, st); break;
        case 192: sce_launch_kp<192>(grouped, stride, a, s, tabD, tabN, st); break;
        default: sce_launch_kp<256>(grouped, stride, a, s, tabD, tabN, st); break;
    }
}

template <typename T, bool MSE>
void fh_launch_gather(const FhArgs& a, const float* stats, void* dcoarse, hipStream_t st) {
    hipLaunchKernelGGL((fh_gather_kernel<T, MSE>), dim3(a.B * a.h * a.w), dim3(256), 0, st, a.coarse, a.embed, (const float*)a.ws_f,
                       stats, (T*)dcoarse, a.B, a.h, a.w, a.E, a.ldc, a.c0, a.K, a.KP);
}
template <typename T>
void fh_launch_gather_t(bool mse, const FhArgs& a, const float* stats, void* dcoarse, hipStream_t st) {
    mse ? fh_launch_gather<T, true>(a, stats, dcoarse, st) : fh_launch_gather<T, false>(a, stats, dcoarse, st);
}

// every szn_fused_*head* entry point: prep = build the embedding tables first; unseen / group_mode / group_map as in
// szn_fused_head_grouped (NULL, 0, NULL: ungrouped); kind = the loss; exclude: FH_SIMCE, FH_RANK and FH_BIAS; temperature: FH_SIMCE and
// FH_BIAS; margin / hardest: FH_RANK only; bias_unseen / bias_weight / hidden_label: FH_BIAS only
enum FhKind { FH_COS, FH_MSE, FH_SIMCE, FH_RANK, FH_BIAS };
int fused_head_impl(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                    const float* coarse, const float* embed, const int64_t* target, float* loss,
                    float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace,
                    szn_stream_t stream, bool prep, const szn_class_set* unseen, int group_mode,
                    const int64_t* group_map, FhKind kind, const szn_class_set* exclude = nullptr, float temperature = 1.f,
                    float margin = 0.f, int hardest = 0, const szn_class_set* bias_unseen = nullptr, float bias_weight = 0.f,
                    int64_t hidden_label = 0) {
    const bool mse = kind == FH_MSE;
    if (stride != 32 && stride != 8) SZN_FAIL(SZN_ERR_UNSUPPORTED, "fused_head: stride %d (32 and 8 are built)", stride);
    if (!coarse || !embed || !workspace || B <= 0 || h <= 0 || w <= 0 || E <= 0 || c0 < 0 || ldc < c0 + E || H <= 0 ||
        W <= 0 || crop < 0 || K <= 0)
        SZN_FAIL(SZN_ERR_ARG, "fused_head: bad argument");
    if (K > 256) SZN_FAIL(SZN_ERR_UNSUPPORTED, "fused_head: K=%d > 256", K);
    if (H + crop > stride * h + stride || W + crop > stride * w + stride)
        SZN_FAIL(SZN_ERR_ARG, "fused_head: crop window exceeds the deconv output");
    if ((target == nullptr) != (loss == nullptr) || (loss && !stats)) SZN_FAIL(SZN_ERR_ARG, "fused_head: target/loss/stats go together");
    if (dcoarse && !target) SZN_FAIL(SZN_ERR_ARG, "fused_head: dcoarse needs target");
    if (((uintptr_t)workspace) & 15) SZN_FAIL(SZN_ERR_ARG, "fused_head: workspace must be 16-B aligned");
    const ClassBits ubits = class_bits(unseen);
    if (group_mode < 0 || group_mode > 2) SZN_FAIL(SZN_ERR_ARG, "fused_head_grouped: bad group mode %d", group_mode);
    if (group_mode != 0 && !pred) SZN_FAIL(SZN_ERR_ARG, "fused_head_grouped: group mode %d needs pred", group_mode);
    if (group_mode == 1 && !group_map) SZN_FAIL(SZN_ERR_ARG, "fused_head_grouped: group mode 1 needs group_map");
    if (group_mode == 2 && !target) SZN_FAIL(SZN_ERR_ARG, "fused_head_grouped: group mode 2 needs target");
    if (!class_bits_fit(ubits, K)) SZN_FAIL(SZN_ERR_ARG, "fused_head_grouped: the unseen set names a class >= K = %d", K);
    SceArgs sce{};
    if (kind == FH_SIMCE) {
        if (!(temperature > 0.f) || !isfinite(temperature)) SZN_FAIL(SZN_ERR_ARG, "fused_simce_head: temperature %g is not a positive finite number", (double)temperature);
        sce.excl = class_bits(exclude);
        if (!class_bits_fit(sce.excl, K)) SZN_FAIL(SZN_ERR_ARG, "fused_simce_head: the exclude set names a class >= K = %d", K);
        int n_excl = 0;
        for (int i = 0; i < 4; ++i) n_excl += __builtin_popcountll(sce.excl.w[i]);
        if (n_excl >= K) SZN_FAIL(SZN_ERR_ARG, "fused_simce_head: the exclude set leaves none of the %d classes competing", K);
        sce.inv_t = 1.f / temperature;
    }
    RankArgs rank{};
    if (kind == FH_RANK) {
        if (!(margin >= 0.f) || !isfinite(margin)) SZN_FAIL(SZN_ERR_ARG, "fused_rank_head: margin %g is not a finite number >= 0", (double)margin);
        if (hardest != 0 && hardest != 1) SZN_FAIL(SZN_ERR_ARG, "fused_rank_head: hardest %d is neither 0 nor 1", hardest);
        rank.excl = class_bits(exclude);
        if (!class_bits_fit(rank.excl, K)) SZN_FAIL(SZN_ERR_ARG, "fused_rank_head: the exclude set names a class >= K = %d", K);
        int n_excl = 0;
        for (int i = 0; i < 4; ++i) n_excl += __builtin_popcountll(rank.excl.w[i]);
        if (K - n_excl < 2) SZN_FAIL(SZN_ERR_ARG, "fused_rank_head: the exclude set leaves %d of the %d classes competing (two are needed)", K - n_excl, K);
        rank.margin = margin; rank.hardest = hardest;
    }
    BiasArgs bias{};
    if (kind == FH_BIAS) {
        if (!(temperature > 0.f) || !isfinite(temperature)) SZN_FAIL(SZN_ERR_ARG, "fused_simce_bias_head: temperature %g is not a positive finite number", (double)temperature);
        bias.excl = class_bits(exclude);
        if (!class_bits_fit(bias.excl, K)) SZN_FAIL(SZN_ERR_ARG, "fused_simce_bias_head: the exclude set names a class >= K = %d", K);
        bias.unseen = class_bits(bias_unseen);
        if (!class_bits_fit(bias.unseen, K)) SZN_FAIL(SZN_ERR_ARG, "fused_simce_bias_head: the bias set names a class >= K = %d", K);
        int n_excl = 0, n_u = 0;
        for (int i = 0; i < 4; ++i) { n_excl += __builtin_popcountll(bias.excl.w[i]); n_u += __builtin_popcountll(bias.unseen.w[i]); }
        if (n_excl >= K) SZN_FAIL(SZN_ERR_ARG, "fused_simce_bias_head: the exclude set leaves none of the %d classes competing", K);
        if (n_u == 0 || n_u >= K) SZN_FAIL(SZN_ERR_ARG, "fused_simce_bias_head: the bias set holds %d of the %d classes (at least one, not all)", n_u, K);
        if (!(bias_weight > 0.f) || !isfinite(bias_weight)) SZN_FAIL(SZN_ERR_ARG, "fused_simce_bias_head: weight %g is not a positive finite number", (double)bias_weight);
        if (hidden_label >= -1) SZN_FAIL(SZN_ERR_ARG, "fused_simce_bias_head: hidden label %lld is not below -1", (long long)hidden_label);
        bias.inv_t = 1.f / temperature; bias.weight = bias_weight; bias.hidden = (long)hidden_label;
    }
    const bool dense = kind == FH_SIMCE || kind == FH_RANK || kind == FH_BIAS;
    const bool grouped = group_mode != 0;
    hipStream_t st = (hipStream_t)stream;
    const int KP = kp_of(K);
    const int cells = (h + 1) * (w + 1);
    if (fh_lds(E, KP, mse).bytes() > 150 * 1024 || (dense && sce_lds_floats(stride, E, KP) * sizeof(float) > 150 * 1024))
        SZN_FAIL(SZN_ERR_UNSUPPORTED, "fused_head: E=%d too large for LDS", E);
    const FhWorkspace wl = fh_workspace(B, h, w, E, KP);
    char* ws = (char*)workspace;
    float* ws_f = (float*)ws;
    double* part = (double*)(ws + wl.part);
    double* sums = (double*)(ws + wl.sums);
    float* tabD = (float*)(ws + wl.tabD);
    float* tabN = (float*)(ws + wl.tabN);
    if (prep) {
        hipLaunchKernelGGL(fh_prep_kernel, dim3(szn_div_up((long)E * KP, 256)), dim3(256), 0, st, embed, ws_f, E, K, KP);
        SZN_CHECK_LAUNCH("fh_prep_kernel");
    }
    FhArgs a;
    a.coarse = coarse; a.embed = embed; a.target = target; a.pred = pred; a.ws_f = ws_f; a.part = part;
    a.B = B; a.h = h; a.w = w; a.E = E; a.ldc = ldc; a.c0 = c0; a.H = H; a.W = W; a.crop = crop; a.K = K; a.KP = KP;
    a.gmap = group_map; a.gmode = group_mode; a.unseen = ubits;
    if (kind == FH_SIMCE) sce_launch_k(KP, grouped, stride, a, sce, tabD, tabN, st);
    else if (kind == FH_RANK) sce_launch_k(KP, grouped, stride, a, rank, tabD, tabN, st);
    else if (kind == FH_BIAS) sce_launch_k(KP, grouped, stride, a, bias, tabD, tabN, st);
    else switch (KP) {
        case 24: fh_launch_kp<24>(grouped, mse, stride, a, tabD, tabN, st); break;
        case 40: fh_launch_kp<40>(grouped, mse, stride, a, tabD, tabN, st); break;
        case 64: fh_launch_kp<64>(grouped, mse, stride, a, tabD, tabN, st); break;
        case 128: fh_launch_kp<128>(grouped, mse, stride, a, tabD, tabN, st); break;
        case 192: fh_launch_kp<192>(grouped, mse, stride, a, tabD, tabN, st); break;
        default: fh_launch_kp<256>(grouped, mse, stride, a, tabD, tabN, st); break;
    }
    SZN_CHECK_LAUNCH("fh_cell_kernel");
    if (loss) {
        hipLaunchKernelGGL(fh_image_sums_kernel, dim3(B), dim3(256), 0, st, (const double*)part, cells, stats, sums);
        hipLaunchKernelGGL(fh_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)sums, B, kind != FH_COS ? 1 : 0, loss);
        SZN_CHECK_LAUNCH("fh_finalize_kernel");
    }
    if (dcoarse) {
        if (dcoarse_dtype == SZN_F32) fh_launch_gather_t<float>(mse, a, stats, dcoarse, st);
        else if (dcoarse_dtype == SZN_BF16) fh_launch_gather_t<bf16_raw>(mse, a, stats, dcoarse, st);
        else if (dcoarse_dtype == SZN_F16) fh_launch_gather_t<f16_raw>(mse, a, stats, dcoarse, st);
        else
            SZN_FAIL(SZN_ERR_ARG, "fused_head: bad dcoarse_dtype %d", dcoarse_dtype);
        SZN_CHECK_LAUNCH("fh_gather_kernel");
    }
    return SZN_OK;
}

}  // namespace

extern "C" size_t szn_fused_head_workspace_bytes(int B, int h, int w, int E, int K) {
    if (B <= 0 || h <= 0 || w <= 0 || E <= 0 || K <= 0 || K > 256) return 0;
    return fh_workspace(B, h, w, E, kp_of(K)).bytes;
}

// The class embeddings are constants of a training run (trainer_fcn.py:49-62 loads them once): their transpose and norms -- fh_prep_kernel, 23 us of
// a 2.5-8 ms step, a chain of dependent loads -- need not be rebuilt every step.  szn_fused_head_prepare writes them to the head of `workspace`
// once; the *_prepared entry points are their namesakes without that launch, for a caller that keeps the workspace and re-prepares when the
// embeddings (or the workspace) change.  Same tables, same bits.
extern "C" int szn_fused_head_prepare(int E, int K, const float* embed, void* workspace, szn_stream_t stream) {
    if (!embed || !workspace || E <= 0 || K <= 0) SZN_FAIL(SZN_ERR_ARG, "fused_head_prepare: bad argument");
    if (K > 256) SZN_FAIL(SZN_ERR_UNSUPPORTED, "fused_head_prepare: K=%d > 256", K);
    if (((uintptr_t)workspace) & 15) SZN_FAIL(SZN_ERR_ARG, "fused_head_prepare: workspace must be 16-B aligned");
    const int KP = kp_of(K);
    hipLaunchKernelGGL(fh_prep_kernel, dim3(szn_div_up((long)E * KP, 256)), dim3(256), 0, (hipStream_t)stream, embed, (float*)workspace, E, K, KP);
    SZN_CHECK_LAUNCH("fh_prep_kernel");
    return SZN_OK;
}

extern "C" int szn_fused_head(int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                              const float* coarse, const float* embed, const int64_t* target, float* loss, float* stats,
                              int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream) {
    return fused_head_impl(32, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, true, nullptr, 0, nullptr, FH_COS);
}

extern "C" int szn_fused_head_strided(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                      const float* coarse, const float* embed, const int64_t* target, float* loss,
                                      float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace,
                                      szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, true, nullptr, 0, nullptr, FH_COS);
}

extern "C" int szn_fused_head_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                       const float* coarse, const float* embed, const int64_t* target, float* loss,
                                       float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace,
                                       szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, false, nullptr, 0, nullptr, FH_COS);
}

// group mode 0: szn_fused_head_strided / _prepared bit for bit.  1: a pixel takes the unseen group where group_map == 0 (the seen-mask
// prediction, szn_seenmask_head: s1 > s0 ? 1 : 0).  2: where its target label is in `unseen` (negative labels -> seen group).
extern "C" int szn_fused_head_grouped(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                      const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                                      int group_mode, const int64_t* group_map, float* loss, float* stats, int64_t* pred,
                                      int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, true, unseen, group_mode, group_map, FH_COS);
}

extern "C" int szn_fused_head_grouped_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                               const float* coarse, const float* embed, const int64_t* target,
                                               const szn_class_set* unseen, int group_mode, const int64_t* group_map, float* loss,
                                               float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace,
                                               szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, false, unseen, group_mode, group_map, FH_COS);
}

// The MSE embedding loss (train.py -loss mse; trainer_fcn.py forward / forward_szn -> utils.py:50-73 mse_loss) through the same head:
// szn_bilinear_up_crop_fwd -> szn_mse_loss_fwd -> szn_embed_argmax_k -> szn_mse_loss_bwd -> szn_bilinear_up_crop_bwd without the score.
// Arguments, NULL rules, error codes, workspace (szn_fused_head_workspace_bytes) and prepare step (szn_fused_head_prepare) of
// szn_fused_head_grouped[_prepared]; pred is that head's pred bit for bit.
extern "C" int szn_fused_mse_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                  const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                                  int group_mode, const int64_t* group_map, float* loss, float* stats, int64_t* pred,
                                  int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, true, unseen, group_mode, group_map, FH_MSE);
}

extern "C" int szn_fused_mse_head_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                           const float* coarse, const float* embed, const int64_t* target,
                                           const szn_class_set* unseen, int group_mode, const int64_t* group_map, float* loss,
                                           float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace,
                                           szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, false, unseen, group_mode, group_map, FH_MSE);
}

// The similarity cross-entropy loss (train.py -loss sim_ce; utils.sim_ce_loss) through the same head: softmax over the cosines of the
// classes outside `exclude`, divided by `temperature`, cross-entropy against the label (include/szn.h).
extern "C" int szn_fused_simce_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                    const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                                    int group_mode, const int64_t* group_map, const szn_class_set* exclude, float temperature,
                                    float* loss, float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace,
                                    szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, true, unseen, group_mode, group_map, FH_SIMCE, exclude, temperature);
}

extern "C" int szn_fused_simce_head_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                             const float* coarse, const float* embed, const int64_t* target,
                                             const szn_class_set* unseen, int group_mode, const int64_t* group_map,
                                             const szn_class_set* exclude, float temperature, float* loss, float* stats,
                                             int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, false, unseen, group_mode, group_map, FH_SIMCE, exclude, temperature);
}

// The hinge ranking loss (train.py -loss rank; utils.rank_loss) through the same head: the label's cosine against the cosines of the
// other classes outside `exclude`, sum of hinges (hardest = 0) or the hardest negative alone (hardest = 1) (include/szn.h).
extern "C" int szn_fused_rank_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                   const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                                   int group_mode, const int64_t* group_map, const szn_class_set* exclude, float margin, int hardest,
                                   float* loss, float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace,
                                   szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, true, unseen, group_mode, group_map, FH_RANK, exclude, 1.f, margin, hardest);
}

extern "C" int szn_fused_rank_head_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                            const float* coarse, const float* embed, const int64_t* target,
                                            const szn_class_set* unseen, int group_mode, const int64_t* group_map,
                                            const szn_class_set* exclude, float margin, int hardest, float* loss, float* stats,
                                            int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, false, unseen, group_mode, group_map, FH_RANK, exclude, 1.f, margin, hardest);
}

// sim_ce with QFSL's unseen-bias term (train.py -loss sim_ce --bias-loss; utils.sim_ce_bias_loss): a pixel labelled `hidden_label` adds
// weight * -log sum_{u in bias_unseen} softmax_u over all K classes; every other pixel is szn_fused_simce_head's (include/szn.h).
extern "C" int szn_fused_simce_bias_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                         const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                                         int group_mode, const int64_t* group_map, const szn_class_set* exclude, float temperature,
                                         const szn_class_set* bias_unseen, float weight, int64_t hidden_label, float* loss, float* stats,
                                         int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, true, unseen, group_mode, group_map, FH_BIAS, exclude, temperature, 0.f, 0, bias_unseen, weight,
                           hidden_label);
}

extern "C" int szn_fused_simce_bias_head_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                                  const float* coarse, const float* embed, const int64_t* target,
                                                  const szn_class_set* unseen, int group_mode, const int64_t* group_map,
                                                  const szn_class_set* exclude, float temperature, const szn_class_set* bias_unseen,
                                                  float weight, int64_t hidden_label, float* loss, float* stats, int64_t* pred,
                                                  int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream) {
    return fused_head_impl(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, loss, stats, pred, dcoarse_dtype, dcoarse,
                           workspace, stream, false, unseen, group_mode, group_map, FH_BIAS, exclude, temperature, 0.f, 0, bias_unseen, weight,
                           hidden_label);
}

// Calibrated stacking (include/szn.h): the seen-class penalty gamma swept over n_gammas values in one pass over the pixels.
extern "C" size_t szn_calib_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int n_gammas) {
    if (calib_bad_geometry(stride, B, h, w, E, K, n_gammas)) return 0;
    return calib_workspace(B, h, w, E, K, n_gammas).bytes;
}

namespace {
// szn_calib_head (sweep == false, margin unused) and szn_seen_sweep_head (sweep == true: `gammas` are its taus, the switch is `margin`):
// the same refusals, workspace and launch sequence, another pixel kernel.  tabled: the workspace already holds the prepared embedding image
// and the stride-8 position tables of this map (szn_seen_sweep_head_tabled): neither is rebuilt.  gate: szn_soft_gate_head (sweep == true
// with the gate's pixel kernels; its eff output counts as a result).  hub: szn_hub_head (sweep == false with the table's pixel kernels)
int calib_head_impl(const char* who, const char* vals, bool sweep, bool tabled, int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W,
                    int crop, int K, const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                    const float* margin, int n_gammas, const float* gammas, int64_t* hist, int pred_index, int64_t* pred, void* workspace,
                    szn_stream_t stream, GateArgs* gate = nullptr, const float* hub = nullptr) {
    if (const char* why = calib_bad_geometry(stride, B, h, w, E, K, n_gammas)) SZN_FAIL(SZN_ERR_ARG, "%s: %s", who, why);
    if (!coarse || !embed || !workspace || !gammas) SZN_FAIL(SZN_ERR_ARG, "%s: coarse, embed, workspace and %s are required", who, vals);
    if (sweep && !margin) SZN_FAIL(SZN_ERR_ARG, "%s: margin is required", who);
    if (!sweep) margin = nullptr;
    const ClassBits ubits = class_bits(unseen);
    if (int rc = calib_check_shared(who, stride, h, w, E, ldc, c0, H, W, crop, K, ubits, workspace)) return rc;
    for (int g = 0; g < n_gammas; ++g) {
        if (!isfinite(gammas[g])) SZN_FAIL(SZN_ERR_ARG, "%s: %s[%d] is not finite", who, vals, g);
        if (g && !(gammas[g] > gammas[g - 1])) SZN_FAIL(SZN_ERR_ARG, "%s: %s must be strictly ascending (at %d)", who, vals, g);
    }
    if (gate) {
        if (!hist && !pred && !gate->eff) SZN_FAIL(SZN_ERR_ARG, "%s: hist, pred and eff are all NULL", who);
        gate->margin = margin;
    } else if (!hist && !pred) SZN_FAIL(SZN_ERR_ARG, "%s: hist and pred are both NULL", who);
    if (hist && !target) SZN_FAIL(SZN_ERR_ARG, "%s: hist needs target", who);
    if (pred && (pred_index < 0 || pred_index >= n_gammas)) SZN_FAIL(SZN_ERR_ARG, "%s: pred_index %d outside [0, %d)", who, pred_index, n_gammas);
    const int KP = kp_of(K);

    hipStream_t st = (hipStream_t)stream;
    const FhWorkspace wl = fh_workspace(B, h, w, E, KP);
    const CalWorkspace cl = calib_workspace(B, h, w, E, K, n_gammas);
    char* ws = (char*)workspace;
    if (!tabled) {
        hipLaunchKernelGGL(fh_prep_kernel, dim3(szn_div_up((long)E * KP, 256)), dim3(256), 0, st, embed, (float*)ws, E, K, KP);
        SZN_CHECK_LAUNCH("fh_prep_kernel");
    }
    FhArgs a{};
    a.coarse = coarse; a.embed = embed; a.target = target; a.ws_f = (float*)ws;
    a.B = B; a.h = h; a.w = w; a.E = E; a.ldc = ldc; a.c0 = c0; a.H = H; a.W = W; a.crop = crop; a.K = K; a.KP = KP;
    a.unseen = ubits;
    CalArgs c{};
    for (int g = 0; g < n_gammas; ++g) c.gamma[g] = gammas[g];
    c.n = n_gammas; c.pred = pred; c.pred_index = pred ? pred_index : 0;
    if (hist) {
        c.XA = (unsigned long long*)(ws + cl.XA); c.XB = (unsigned long long*)(ws + cl.XB);
        if (hipMemsetAsync(ws + cl.XA, 0, cl.bytes - cl.XA, st) != hipSuccess) SZN_FAIL(SZN_ERR_LAUNCH, "%s: clearing the crossing tables failed", who);
    }
    float* tabD = (float*)(ws + wl.tabD);
    float* tabN = (float*)(ws + wl.tabN);
    switch (KP) {
        case 24: calib_launch<24>(stride, a, c, margin, gate, tabled, tabD, tabN, st, hub); break;
        case 40: calib_launch<40>(stride, a, c, margin, gate, tabled, tabD, tabN, st, hub); break;
        case 64: calib_launch<64>(stride, a, c, margin, gate, tabled, tabD, tabN, st, hub); break;
        case 128: calib_launch<128>(stride, a, c, margin, gate, tabled, tabD, tabN, st, hub); break;
        case 192: calib_launch<192>(stride, a, c, margin, gate, tabled, tabD, tabN, st, hub); break;
        default: calib_launch<256>(stride, a, c, margin, gate, tabled, tabD, tabN, st, hub); break;
    }
    if (hub) SZN_CHECK_LAUNCH(stride == 8 ? "hub_cell_tab_kernel" : "hub_cell_kernel");
    else if (gate) SZN_CHECK_LAUNCH(stride == 8 ? "gate_cell_tab_kernel" : "gate_cell_kernel");
    else if (sweep) SZN_CHECK_LAUNCH(stride == 8 ? "sweep_cell_tab_kernel" : "sweep_cell_kernel");
    else SZN_CHECK_LAUNCH(stride == 8 ? "calib_cell_tab_kernel" : "calib_cell_kernel");
    if (hist) {
        hipLaunchKernelGGL(calib_hist_kernel, dim3(szn_div_up((long)K * K, 256)), dim3(256), 0, st, (const unsigned long long*)c.XA,
                           (const unsigned long long*)c.XB, K, n_gammas, hist);
        SZN_CHECK_LAUNCH("calib_hist_kernel");
    }
    return SZN_OK;
}
}  // namespace

extern "C" int szn_calib_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                              const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                              int n_gammas, const float* gammas, int64_t* hist, int pred_index, int64_t* pred, void* workspace,
                              szn_stream_t stream) {
    return calib_head_impl("calib_head", "gammas", false, false, stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, unseen, nullptr,
                           n_gammas, gammas, hist, pred_index, pred, workspace, stream);
}

// Seen-mask threshold sweep (include/szn.h): the grouped head's class rule with the group decided by margin > tau, n_taus thresholds in
// one pass over the pixels.  Sizes and workspace are szn_calib_head's.
static_assert(SZN_SEEN_SWEEP_MAX_TAUS == SZN_CALIB_MAX_GAMMAS, "the taus travel in CalArgs::gamma");
extern "C" size_t szn_seen_sweep_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int n_taus) {
    return szn_calib_head_workspace_bytes(stride, B, h, w, E, K, n_taus);
}

extern "C" int szn_seen_sweep_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                   const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                                   const float* margin, int n_taus, const float* taus, int64_t* hist, int pred_index, int64_t* pred,
                                   void* workspace, szn_stream_t stream) {
    return calib_head_impl("seen_sweep_head", "taus", true, false, stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, unseen, margin,
                           n_taus, taus, hist, pred_index, pred, workspace, stream);
}

// The same on a workspace in whose head a fused embedding head has just run on this map (include/szn.h): its embedding image and its
// stride-8 position tables are the ones this call would build, so it builds neither.
extern "C" int szn_seen_sweep_head_tabled(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                          const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                                          const float* margin, int n_taus, const float* taus, int64_t* hist, int pred_index, int64_t* pred,
                                          void* workspace, szn_stream_t stream) {
    return calib_head_impl("seen_sweep_head_tabled", "taus", true, true, stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, unseen,
                           margin, n_taus, taus, hist, pred_index, pred, workspace, stream);
}

// Soft seen/unseen gating (include/szn.h): the threshold sweep with the per-pixel effective margin e = margin - weight * (l_S - l_U) as the
// switch and the true in-group argmaxes as the two answers.  Sizes, workspace, refusals and launch sequence are szn_seen_sweep_head's.
extern "C" size_t szn_soft_gate_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int n_taus) {
    return szn_calib_head_workspace_bytes(stride, B, h, w, E, K, n_taus);
}

namespace {
int soft_gate_impl(const char* who, bool tabled, int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                   const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen, const float* margin,
                   float temperature, float weight, int n_taus, const float* taus, int64_t* hist, int pred_index, int64_t* pred, float* eff,
                   void* workspace, szn_stream_t stream) {
    if (!isfinite(temperature) || !(temperature > 0.f)) SZN_FAIL(SZN_ERR_ARG, "%s: temperature must be finite and > 0", who);
    if (!isfinite(weight) || !(weight >= 0.f)) SZN_FAIL(SZN_ERR_ARG, "%s: weight must be finite and >= 0", who);
    GateArgs g{};
    g.eff = eff; g.inv_t = 1.0f / temperature; g.weight = weight;
    return calib_head_impl(who, "taus", true, tabled, stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, unseen, margin, n_taus,
                           taus, hist, pred_index, pred, workspace, stream, &g);
}
}  // namespace

extern "C" int szn_soft_gate_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                  const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                                  const float* margin, float temperature, float weight, int n_taus, const float* taus, int64_t* hist,
                                  int pred_index, int64_t* pred, float* eff, void* workspace, szn_stream_t stream) {
    return soft_gate_impl("soft_gate_head", false, stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, unseen, margin, temperature,
                          weight, n_taus, taus, hist, pred_index, pred, eff, workspace, stream);
}

extern "C" int szn_soft_gate_head_tabled(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                         const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                                         const float* margin, float temperature, float weight, int n_taus, const float* taus, int64_t* hist,
                                         int pred_index, int64_t* pred, float* eff, void* workspace, szn_stream_t stream) {
    return soft_gate_impl("soft_gate_head_tabled", true, stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, unseen, margin,
                          temperature, weight, n_taus, taus, hist, pred_index, pred, eff, workspace, stream);
}

// Hubness correction (include/szn.h): szn_hub_stats leaves per image and class a (scale, shift) pair from the first two moments of the
// class's similarity over the image's pixels; szn_hub_head is szn_calib_head on fmaf(sim, scale, -shift).
extern "C" size_t szn_hub_stats_workspace_bytes(int stride, int B, int h, int w, int E, int K) {
    if (calib_bad_geometry(stride, B, h, w, E, K, 1)) return 0;
    return hub_workspace(B, h, w, E, K).bytes;
}

extern "C" int szn_hub_stats(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                             const float* coarse, const float* embed, const int64_t* target, int mode, float beta, float min_sd,
                             float* table, int64_t* sums, int64_t* counts, void* workspace, szn_stream_t stream) {
    if (const char* why = calib_bad_geometry(stride, B, h, w, E, K, 1)) SZN_FAIL(SZN_ERR_ARG, "hub_stats: %s", why);
    if (!coarse || !embed || !workspace || !table) SZN_FAIL(SZN_ERR_ARG, "hub_stats: coarse, embed, workspace and table are required");
    if (int rc = calib_check_window("hub_stats", stride, h, w, E, ldc, c0, H, W, crop, workspace)) return rc;
    if (mode != SZN_HUB_MEAN && mode != SZN_HUB_ZSCORE) SZN_FAIL(SZN_ERR_ARG, "hub_stats: mode %d is neither SZN_HUB_MEAN nor SZN_HUB_ZSCORE", mode);
    if (!isfinite(beta) || !(beta >= 0.f)) SZN_FAIL(SZN_ERR_ARG, "hub_stats: beta must be finite and >= 0");
    if (!isfinite(min_sd) || !(min_sd > 0.f)) SZN_FAIL(SZN_ERR_ARG, "hub_stats: min_sd must be finite and > 0");
    if ((long long)H * W > SZN_HUB_MAX_PIXELS) SZN_FAIL(SZN_ERR_ARG, "hub_stats: H * W above SZN_HUB_MAX_PIXELS (the second moment must fit int64)");
    const int KP = kp_of(K);
    if (fh_lds(E, KP, false).bytes() > 150 * 1024) SZN_FAIL(SZN_ERR_UNSUPPORTED, "hub_stats: E=%d too large for LDS", E);

    hipStream_t st = (hipStream_t)stream;
    const FhWorkspace wl = fh_workspace(B, h, w, E, KP);
    const HubWorkspace hl = hub_workspace(B, h, w, E, K);
    char* ws = (char*)workspace;
    hipLaunchKernelGGL(fh_prep_kernel, dim3(szn_div_up((long)E * KP, 256)), dim3(256), 0, st, embed, (float*)ws, E, K, KP);
    SZN_CHECK_LAUNCH("fh_prep_kernel");
    if (hipMemsetAsync(ws + hl.S, 0, hl.bytes - hl.S, st) != hipSuccess) SZN_FAIL(SZN_ERR_LAUNCH, "hub_stats: clearing the sums failed");
    FhArgs a{};
    a.coarse = coarse; a.embed = embed; a.target = target; a.ws_f = (float*)ws;
    a.B = B; a.h = h; a.w = w; a.E = E; a.ldc = ldc; a.c0 = c0; a.H = H; a.W = W; a.crop = crop; a.K = K; a.KP = KP;
    unsigned long long* S = (unsigned long long*)(ws + hl.S);
    unsigned long long* n = (unsigned long long*)(ws + hl.n);
    float* tabD = (float*)(ws + wl.tabD);
    float* tabN = (float*)(ws + wl.tabN);
    switch (KP) {
        case 24: hub_stats_launch<24>(stride, a, S, n, tabD, tabN, st); break;
        case 40: hub_stats_launch<40>(stride, a, S, n, tabD, tabN, st); break;
        case 64: hub_stats_launch<64>(stride, a, S, n, tabD, tabN, st); break;
        case 128: hub_stats_launch<128>(stride, a, S, n, tabD, tabN, st); break;
        case 192: hub_stats_launch<192>(stride, a, S, n, tabD, tabN, st); break;
        default: hub_stats_launch<256>(stride, a, S, n, tabD, tabN, st); break;
    }
    SZN_CHECK_LAUNCH(stride == 8 ? "hub_stats_cell_tab_kernel" : "hub_stats_cell_kernel");
    hipLaunchKernelGGL(hub_table_kernel, dim3(szn_div_up((long)B * K, 256)), dim3(256), 0, st, (const long long*)S, (const long long*)n, B, K,
                       mode, (double)beta, (double)min_sd, table, sums, counts);
    SZN_CHECK_LAUNCH("hub_table_kernel");
    return SZN_OK;
}

extern "C" size_t szn_hub_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int n_gammas) {
    return szn_calib_head_workspace_bytes(stride, B, h, w, E, K, n_gammas);
}

extern "C" int szn_hub_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                            const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                            const float* table, int n_gammas, const float* gammas, int64_t* hist, int pred_index, int64_t* pred,
                            void* workspace, szn_stream_t stream) {
    if (!table) SZN_FAIL(SZN_ERR_ARG, "hub_head: table is required");
    return calib_head_impl("hub_head", "gammas", false, false, stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, embed, target, unseen, nullptr,
                           n_gammas, gammas, hist, pred_index, pred, workspace, stream, nullptr, table);
}

// Self-training pseudo labels (include/szn.h): the calibrated rule at one gamma picks the candidates among the pixels labelled cand_label,
// the most confident keep_permille of them per unseen class take their class as the label.
extern "C" size_t szn_pseudo_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int H, int W) {
    if (calib_bad_geometry(stride, B, h, w, E, K, 1) || H <= 0 || W <= 0) return 0;
    return pseudo_workspace(B, h, w, E, K, H, W).bytes;
}

extern "C" int szn_pseudo_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                               const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                               float gamma, float conf_floor, int keep_permille, int64_t cand_label, int64_t* target_out,
                               int64_t* cand, float* conf, int64_t* qhist, int32_t* thr, int64_t* counts, void* workspace,
                               szn_stream_t stream) {
    if (const char* why = calib_bad_geometry(stride, B, h, w, E, K, 1)) SZN_FAIL(SZN_ERR_ARG, "pseudo_head: %s", why);
    if (!coarse || !embed || !workspace || !target || !target_out)
        SZN_FAIL(SZN_ERR_ARG, "pseudo_head: coarse, embed, workspace, target and target_out are required");
    const ClassBits ubits = class_bits(unseen);
    if (int rc = calib_check_shared("pseudo_head", stride, h, w, E, ldc, c0, H, W, crop, K, ubits, workspace)) return rc;
    if (!isfinite(gamma) || !isfinite(conf_floor)) SZN_FAIL(SZN_ERR_ARG, "pseudo_head: gamma and conf_floor must be finite");
    if (keep_permille < 1 || keep_permille > 1000) SZN_FAIL(SZN_ERR_ARG, "pseudo_head: keep_permille %d outside [1, 1000]", keep_permille);
    if (cand_label >= 0) SZN_FAIL(SZN_ERR_ARG, "pseudo_head: cand_label %lld must be negative (a class label cannot mark the hidden pixels)", (long long)cand_label);
    if (target_out == target) SZN_FAIL(SZN_ERR_ARG, "pseudo_head: target_out must not alias target");
    const int KP = kp_of(K);

    hipStream_t st = (hipStream_t)stream;
    const FhWorkspace wl = fh_workspace(B, h, w, E, KP);
    const PseudoWorkspace pl = pseudo_workspace(B, h, w, E, K, H, W);
    char* ws = (char*)workspace;
    hipLaunchKernelGGL(fh_prep_kernel, dim3(szn_div_up((long)E * KP, 256)), dim3(256), 0, st, embed, (float*)ws, E, K, KP);
    SZN_CHECK_LAUNCH("fh_prep_kernel");
    FhArgs a{};
    a.coarse = coarse; a.embed = embed; a.target = target; a.ws_f = (float*)ws;
    a.B = B; a.h = h; a.w = w; a.E = E; a.ldc = ldc; a.c0 = c0; a.H = H; a.W = W; a.crop = crop; a.K = K; a.KP = KP;
    a.unseen = ubits;
    PseudoArgs p{};
    p.gamma = gamma; p.conf_floor = conf_floor; p.cand_label = (long)cand_label;
    p.QH = (unsigned long long*)(ws + pl.QH); p.rec = (int2*)(ws + pl.rec);
    int32_t* thr_ws = (int32_t*)(ws + pl.thr);
    if (hipMemsetAsync(ws + pl.QH, 0, pl.thr - pl.QH, st) != hipSuccess) SZN_FAIL(SZN_ERR_LAUNCH, "pseudo_head: clearing the confidence histogram failed");
    float* tabD = (float*)(ws + wl.tabD);
    float* tabN = (float*)(ws + wl.tabN);
    switch (KP) {
        case 24: pseudo_launch<24>(stride, a, p, tabD, tabN, st); break;
        case 40: pseudo_launch<40>(stride, a, p, tabD, tabN, st); break;
        case 64: pseudo_launch<64>(stride, a, p, tabD, tabN, st); break;
        case 128: pseudo_launch<128>(stride, a, p, tabD, tabN, st); break;
        case 192: pseudo_launch<192>(stride, a, p, tabD, tabN, st); break;
        default: pseudo_launch<256>(stride, a, p, tabD, tabN, st); break;
    }
    SZN_CHECK_LAUNCH(stride == 8 ? "pseudo_cell_tab_kernel" : "pseudo_cell_kernel");
    hipLaunchKernelGGL(pseudo_thr_kernel, dim3(K), dim3(256), 0, st, (const unsigned long long*)p.QH, keep_permille, thr_ws, qhist, thr,
                       counts);
    SZN_CHECK_LAUNCH("pseudo_thr_kernel");
    const long n = (long)B * H * W;
    hipLaunchKernelGGL(pseudo_relabel_kernel, dim3((unsigned)szn_div_up(n, 256)), dim3(256), 0, st, target, (const int2*)p.rec,
                       (const int32_t*)thr_ws, n, target_out, cand, conf);
    SZN_CHECK_LAUNCH("pseudo_relabel_kernel");
    return SZN_OK;
}

// Hard-pixel mining (include/szn.h): per image the keep_permille labelled pixels with the lowest own-class cosine, and every one below
// `thresh`, keep their label; the others read drop_label.
extern "C" size_t szn_ohem_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int H, int W) {
    if (calib_bad_geometry(stride, B, h, w, E, K, 1) || H <= 0 || W <= 0) return 0;
    return ohem_workspace(B, h, w, E, K, H, W).bytes;
}

extern "C" int szn_ohem_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                             const float* coarse, const float* embed, const int64_t* target, const szn_class_set* skip,
                             int keep_permille, float thresh, int64_t drop_label, int64_t* target_out, float* conf, int64_t* qhist,
                             int32_t* cut, int64_t* counts, void* workspace, szn_stream_t stream) {
    if (const char* why = calib_bad_geometry(stride, B, h, w, E, K, 1)) SZN_FAIL(SZN_ERR_ARG, "ohem_head: %s", why);
    if (!coarse || !embed || !workspace || !target || !target_out)
        SZN_FAIL(SZN_ERR_ARG, "ohem_head: coarse, embed, workspace, target and target_out are required");
    if (int rc = calib_check_window("ohem_head", stride, h, w, E, ldc, c0, H, W, crop, workspace)) return rc;
    if (keep_permille < 1 || keep_permille > 1000) SZN_FAIL(SZN_ERR_ARG, "ohem_head: keep_permille %d outside [1, 1000]", keep_permille);
    if (!isfinite(thresh)) SZN_FAIL(SZN_ERR_ARG, "ohem_head: thresh must be finite (a value <= -1 turns it off)");
    if (drop_label >= 0) SZN_FAIL(SZN_ERR_ARG, "ohem_head: drop_label %lld must be negative (a label every head ignores)", (long long)drop_label);
    const ClassBits sbits = class_bits(skip);
    if (!class_bits_fit(sbits, K)) SZN_FAIL(SZN_ERR_ARG, "ohem_head: the skip set names a class >= K = %d", K);
    int n_skip = 0;
    for (int i = 0; i < 4; ++i) n_skip += __builtin_popcountll(sbits.w[i]);
    if (n_skip >= K) SZN_FAIL(SZN_ERR_ARG, "ohem_head: the skip set holds every class below K = %d", K);
    if (target_out == target) SZN_FAIL(SZN_ERR_ARG, "ohem_head: target_out must not alias target");
    const int KP = kp_of(K);
    if (fh_lds(E, KP, false).bytes() > 150 * 1024) SZN_FAIL(SZN_ERR_UNSUPPORTED, "ohem_head: E=%d too large for LDS", E);

    hipStream_t st = (hipStream_t)stream;
    const FhWorkspace wl = fh_workspace(B, h, w, E, KP);
    const OhemWorkspace ol = ohem_workspace(B, h, w, E, K, H, W);
    char* ws = (char*)workspace;
    hipLaunchKernelGGL(fh_prep_kernel, dim3(szn_div_up((long)E * KP, 256)), dim3(256), 0, st, embed, (float*)ws, E, K, KP);
    SZN_CHECK_LAUNCH("fh_prep_kernel");
    FhArgs a{};
    a.coarse = coarse; a.embed = embed; a.target = target; a.ws_f = (float*)ws;
    a.B = B; a.h = h; a.w = w; a.E = E; a.ldc = ldc; a.c0 = c0; a.H = H; a.W = W; a.crop = crop; a.K = K; a.KP = KP;
    OhemArgs p{};
    p.skip = sbits;
    p.QH = (unsigned long long*)(ws + ol.QH); p.rec = (float*)(ws + ol.rec);
    int32_t* cut_ws = (int32_t*)(ws + ol.cut);
    if (hipMemsetAsync(ws + ol.QH, 0, ol.cut - ol.QH, st) != hipSuccess) SZN_FAIL(SZN_ERR_LAUNCH, "ohem_head: clearing the histogram failed");
    float* tabD = (float*)(ws + wl.tabD);
    float* tabN = (float*)(ws + wl.tabN);
    switch (KP) {
        case 24: ohem_launch<24>(stride, a, p, tabD, tabN, st); break;
        case 40: ohem_launch<40>(stride, a, p, tabD, tabN, st); break;
        case 64: ohem_launch<64>(stride, a, p, tabD, tabN, st); break;
        case 128: ohem_launch<128>(stride, a, p, tabD, tabN, st); break;
        case 192: ohem_launch<192>(stride, a, p, tabD, tabN, st); break;
        default: ohem_launch<256>(stride, a, p, tabD, tabN, st); break;
    }
    SZN_CHECK_LAUNCH(stride == 8 ? "ohem_cell_tab_kernel" : "ohem_cell_kernel");
    hipLaunchKernelGGL(ohem_cut_kernel, dim3(B), dim3(256), 0, st, (const unsigned long long*)p.QH, keep_permille, thresh, cut_ws, qhist,
                       cut, counts);
    SZN_CHECK_LAUNCH("ohem_cut_kernel");
    const long n = (long)B * H * W, hw = (long)H * W;
    const bool vec = hw >= 4 && !((((uintptr_t)target) | ((uintptr_t)target_out) | ((uintptr_t)conf)) & 15);     // rec is 256-B aligned
    const dim3 grid((unsigned)szn_div_up(n, 1024));
    if (vec)
        hipLaunchKernelGGL(ohem_relabel_kernel<true>, grid, dim3(256), 0, st, target, (const float*)p.rec, (const int32_t*)cut_ws, n, hw,
                           drop_label, target_out, conf);
    else
        hipLaunchKernelGGL(ohem_relabel_kernel<false>, grid, dim3(256), 0, st, target, (const float*)p.rec, (const int32_t*)cut_ws, n, hw,
                           drop_label, target_out, conf);
    SZN_CHECK_LAUNCH("ohem_relabel_kernel");
    return SZN_OK;
}
