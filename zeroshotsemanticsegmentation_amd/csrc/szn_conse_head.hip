// szn_conse_head.hip -- ConSE zero-shot inference for the softmax FCN, fused from the coarse logit map, gfx950.
//
// ConSE (Norouzi et al., ICLR 2014) per pixel: softmax over the SEEN classes, the top T of them, f = sum_t p_t e_t (the probability-
// weighted mean of their class embeddings), then the class whose embedding has the largest cosine with f -- over all classes, with the
// seen-class penalty gamma of calibrated stacking between the two groups (include/szn.h: the contract, its tie rules).  The materialised
// chain is a (B,K,H,W) score, a softmax, a topk, a (B,E,H,W) mixture and a (B,K,H,W) cosine; none of them exists here.  f itself is never
// formed either: only its products with the class rows and its norm are needed,
//     f . e_k = sum_t p_t G[c_t][k]        |f|^2 = sum_t sum_u p_t p_u G[c_t][c_u]        G = embed embed^T  (K x K),
// so a pixel costs K logits, T K + T^2 multiply-adds on G and K divisions, whatever E is.
//
// Kernels, in launch order:
//   conse_prep_kernel    G (products accumulated in double, stored fp32, row stride ldg = K | 1) and en[k] = sqrt(G[k][k]) (0 -> 1) in the
//                        workspace, one thread per (k, j).  G[k][j] and G[j][k] are the same sum in the same order: bit-equal.
//   conse_cell_kernel / conse_cell_global_kernel    the pixels, over the stride-S cells of szn_upcell.h, mapped as ce_cell_kernel maps them
//                        (S = 32: one 256-thread block per cell, 4 pixels per thread, one after the other; S = 8: one wave per cell, 4 cells
//                        per block).  The cell's four tap vectors are staged in LDS as there ([c][tap], one 16-B broadcast read per
//                        class), the logit is ce_cell_kernel's (same weights, same fmaf chain: bit-identical).  The top-T list lives in
//                        registers (value, class; T_MAX = 4 | 8 | 16 by template): classes arrive in ascending order, a class enters
//                        only when strictly larger than the last entry and bubbles up past strictly smaller ones, so the list is ordered
//                        by (logit descending, class ascending).  conse_cell_kernel copies G into LDS first -- lanes gather different rows,
//                        and the odd row stride spreads them over the banks -- when taps + en + G fit 64 KiB (two blocks per CU stay
//                        resident; K <= 119 at stride 8, K <= 125 at stride 32); conse_cell_global_kernel reads G through L2 (256 KiB at
//                        K = 256).  Both run the same per-pixel body.
//   calib_hist_kernel    (hist given) szn_calib.h: the pixel's (t, a, b, bin) record went into szn_calib_head's crossing tables with
//                        calib_count; the prefix sums give hist[g].  The cost does not grow with n_gammas.
// No atomics except calib_count's integer adds; no allocation, no host synchronisation.
#include "szn_upcell.h"
#include "szn_calib.h"

namespace {

struct CsArgs {
    const float* coarse; const int64_t* target;
    const float* G; const float* en;     // workspace: G [K][ldg], en [K]
    int B, h, w, K, ldc, c0, H, W, crop;
    int I0, J0, nI, nJ;                  // the pixel cells the crop window touches (szn_fused_ce_head's)
    int ldg, n_top, forced;              // n_top = min(top_t, number of seen classes)
    ClassBits unseen;
};

__global__ __launch_bounds__(256) void conse_prep_kernel(const float* __restrict__ embed, int K, int E, int ldg, float* __restrict__ G,
                                                         float* __restrict__ en) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K * K) return;
    const int k = i / K, j = i % K;
    const float* ek = embed + (size_t)k * E;
    const float* ej = embed + (size_t)j * E;
    double acc = 0.0;
    for (int e = 0; e < E; ++e) acc += (double)ek[e] * (double)ej[e];
    const float g = (float)acc;
    G[(size_t)k * ldg + j] = g;
    if (k == j) {
        const float n = sqrtf(g);
        en[k] = n == 0.f ? 1.f : n;
    }
}

// szn_ce_head.hip's ce_logit: up_fwd_kernel's order (I-1,J-1), (I-1,J), (I,J-1), (I,J)
__device__ __forceinline__ float conse_logit(const float4 t, const float (&w)[4]) {
    float acc = fmaf(t.x, w[0], 0.f);
    acc = fmaf(t.y, w[1], acc);
    acc = fmaf(t.z, w[2], acc);
    acc = fmaf(t.w, w[3], acc);
    return acc;
}

// Pixel (ty, tx) of cell (I, J) of image b: the prediction (where wanted) and the pixel's key t | a << 8 | b << 16 | bin << 24, or -1
// where it is not counted (no histogram, outside the image, label outside [0, K)).  tv: the cell's taps, G: LDS or global, en: LDS
template <int S, int TM>
__device__ __forceinline__ int conse_pixel(const CsArgs& a, const CalArgs& c, const float4* tv, const float* G, const float* en, int b,
                                           int I, int J, int ty, int tx, bool live) {
    const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;
    if (!(live && y >= 0 && y < a.H && x >= 0 && x < a.W)) return -1;
    float wt[4];
    cell_weights<S>(ty, tx, wt);
    const int K = a.K;

    // the top TM seen classes by (logit descending, class ascending); empty slots (id < 0) stay at the tail
    float v[TM];
    int id[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) { v[t] = 0.f; id[t] = -1; }
    for (int k = 0; k < K; ++k) {
        if (in_set(a.unseen, k)) continue;                          // wave-uniform: unseen channels are never read
        const float z = conse_logit(tv[k], wt);
        if (id[TM - 1] < 0 || z > v[TM - 1]) {
            v[TM - 1] = z;
            id[TM - 1] = k;
#pragma unroll
            for (int j = TM - 1; j > 0; --j) {
                if (id[j - 1] < 0 || v[j] > v[j - 1]) {
                    const float fv = v[j]; v[j] = v[j - 1]; v[j - 1] = fv;
                    const int fi = id[j]; id[j] = id[j - 1]; id[j - 1] = fi;
                }
            }
        }
    }

    // p_t over the first n entries, f . f
    const int n = a.n_top;                                          // <= the number of filled slots
    int ro[TM];
    const float mx = v[0];
    float se = 0.f;
#pragma unroll
    for (int t = 0; t < TM; ++t)
        if (t < n) { v[t] = expf(v[t] - mx); se += v[t]; }
#pragma unroll
    for (int t = 0; t < TM; ++t)
        if (t < n) { v[t] = v[t] / se; ro[t] = id[t] * a.ldg; }
    float ff = 0.f;
#pragma unroll
    for (int t = 0; t < TM; ++t) {
        if (t < n) {
            float row = 0.f;
#pragma unroll
            for (int u = 0; u < TM; ++u)
                if (u < n) row = fmaf(v[u], G[ro[t] + id[u]], row);
            ff = fmaf(v[t], row, ff);
        }
    }
    float fn = sqrtf(fmaxf(ff, 0.f));
    if (fn == 0.f) fn = 1.f;

    // the cosines, two running bests (szn_calib_head's: the first class of a group starts it, only a strictly larger value replaces it)
    int ia = -1, ib = -1;
    float va = 0.f, vb = 0.f;
    for (int k = 0; k < K; ++k) {
        float d = 0.f;
#pragma unroll
        for (int t = 0; t < TM; ++t)
            if (t < n) d = fmaf(v[t], G[ro[t] + k], d);
        const float s = d / (fn * en[k]);
        if (in_set(a.unseen, k)) {
            if (ib < 0 || s > vb) { vb = s; ib = k; }
        } else {
            if (ia < 0 || s > va) { va = s; ia = k; }
        }
    }
    const float m = va - vb;
    int bin = 0;
    if (m != m) { ia = 0; ib = 0; bin = c.n; }                      // NaN: class 0 at every gamma
    else
        for (int g = 0; g < c.n; ++g) bin += (m > c.gamma[g] || (m == c.gamma[g] && ia < ib)) ? 1 : 0;     // ascending: a prefix
    const size_t pix = ((size_t)b * a.H + y) * a.W + x;
    if (a.forced) {                                                 // -fu: the group comes from the target
        c.pred[pix] = in_set(a.unseen, a.target[pix]) ? ib : ia;
        return -1;
    }
    if (c.pred) c.pred[pix] = bin > c.pred_index ? ia : ib;
    if (!c.XA) return -1;
    const long t = a.target[pix];
    if (t < 0 || t >= K) return -1;
    return (int)t | ia << 8 | ib << 16 | bin << 24;
}

// lds: taps [CPB][K][4] | en [K] | G [K][ldg] (GLDS)
template <int S, int TM, bool GLDS>
__device__ __forceinline__ void conse_cell_body(const CsArgs& a, const CalArgs& c, float* lds) {
    constexpr int TPC = S == 32 ? 256 : 64;      // threads per cell
    constexpr int PPT = S * S / TPC;             // pixels per thread
    constexpr int CPB = 256 / TPC;               // cells per block
    static_assert(PPT * TPC == S * S && CPB * TPC == 256, "cell mapping");
    const int K = a.K;
    const int tid = threadIdx.x, lane = tid & 63;
    const int lc = tid / TPC, ct = tid % TPC;
    const long ncell = (long)a.B * a.nI * a.nJ;
    const long q = (long)blockIdx.x * CPB + lc;
    const bool active = q < ncell;
    int b = 0, I = 0, J = 0;
    if (active) {
        J = a.J0 + (int)(q % a.nJ);
        const long t = q / a.nJ;
        I = a.I0 + (int)(t % a.nI);
        b = (int)(t / a.nI);
    }
    float* taps = lds + (long)lc * 4 * K;
    float* en = lds + (long)CPB * 4 * K;
    float* Gs = en + K;
    for (int k = ct; k < 4 * K; k += TPC) {
        const int cls = k >> 2, tap = k & 3;
        const int i = tap_i(I, tap), j = tap_j(J, tap);
        taps[k] = (active && i >= 0 && i < a.h && j >= 0 && j < a.w) ? a.coarse[(((long)b * a.h + i) * a.w + j) * a.ldc + a.c0 + cls] : 0.f;
    }
    for (int k = tid; k < K; k += 256) en[k] = a.en[k];
    if (GLDS)
        for (int k = tid; k < K * a.ldg; k += 256) Gs[k] = a.G[k];
    __syncthreads();
    const float* G = GLDS ? Gs : a.G;
#pragma unroll 1
    for (int r = 0; r < PPT; ++r) {              // one pixel at a time: the top-T list is the register budget
        const int p = ct + TPC * r;
        calib_count(a, c, conse_pixel<S, TM>(a, c, (const float4*)taps, G, en, b, I, J, p / S, p % S, active), lane);
    }
}

template <int S, int TM>
__global__ __launch_bounds__(256) void conse_cell_kernel(CsArgs a, CalArgs c) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    conse_cell_body<S, TM, true>(a, c, lds);
}

template <int S, int TM>
__global__ __launch_bounds__(256) void conse_cell_global_kernel(CsArgs a, CalArgs c) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    conse_cell_body<S, TM, false>(a, c, lds);
}

constexpr size_t CONSE_LDS_LIMIT = 64 * 1024;

inline int conse_ldg(int K) { return K | 1; }
inline size_t conse_lds_bytes(int stride, int K, bool with_G) {
    const size_t cpb = stride == 32 ? 1 : 4;
    return (cpb * 4 * K + K + (with_G ? (size_t)K * conse_ldg(K) : 0)) * sizeof(float);
}

// workspace: G | en | XA | XB (the crossing tables only with gammas)
struct ConseWorkspace { size_t G, en, XA, XB, bytes; };
inline ConseWorkspace conse_workspace(int K, int n) {
    ConseWorkspace L;
    const size_t tab = n > 0 ? (size_t)K * K * (n + 1) * sizeof(unsigned long long) : 0;
    L.G = 0;
    L.en = align256((size_t)K * conse_ldg(K) * sizeof(float));
    L.XA = L.en + align256((size_t)K * sizeof(float));
    L.XB = L.XA + tab;
    L.bytes = L.XB + tab;
    return L;
}

// what szn_conse_head and its workspace query refuse about sizes; 0 = fine.  n_gammas = 0 is the forced call's
const char* conse_bad_geometry(int stride, int B, int h, int w, int E, int K, int n_gammas) {
    if (stride != 32 && stride != 8) return "stride must be 8 or 32";
    if (n_gammas < 0 || n_gammas > SZN_CALIB_MAX_GAMMAS) return "n_gammas outside [1, SZN_CALIB_MAX_GAMMAS]";
    if (B <= 0 || h <= 0 || w <= 0 || E <= 0 || K <= 0) return "a size that is not positive";
    if (K > SZN_MAX_CLASSES) return "K above SZN_MAX_CLASSES";
    return nullptr;
}

template <int S, int TM>
void conse_launch(const CsArgs& a, const CalArgs& c, bool glds, hipStream_t st) {
    constexpr int CPB = S == 32 ? 1 : 4;
    const long ncell = (long)a.B * a.nI * a.nJ;
    const dim3 grid((unsigned)szn_div_up(ncell, CPB));
    const size_t lds = conse_lds_bytes(S, a.K, glds);
    if (glds) {
        auto kern = conse_cell_kernel<S, TM>;
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a, c);
    } else {
        hipLaunchKernelGGL((conse_cell_global_kernel<S, TM>), grid, dim3(256), lds, st, a, c);
    }
}

template <int S>
void conse_launch_t(const CsArgs& a, const CalArgs& c, bool glds, hipStream_t st) {
    if (a.n_top <= 4) conse_launch<S, 4>(a, c, glds, st);
    else if (a.n_top <= 8) conse_launch<S, 8>(a, c, glds, st);
    else conse_launch<S, 16>(a, c, glds, st);
}

}  // namespace

extern "C" size_t szn_conse_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int n_gammas) {
    if (conse_bad_geometry(stride, B, h, w, E, K, n_gammas)) return 0;
    return conse_workspace(K, n_gammas).bytes;
}

extern "C" int szn_conse_head(int stride, int B, int h, int w, int K, int ldc, int c0, int H, int W, int crop, int E,
                              const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                              int top_t, int forced, int n_gammas, const float* gammas, int64_t* hist, int pred_index, int64_t* pred,
                              void* workspace, szn_stream_t stream) {
    static_assert(SZN_CONSE_MAX_TOP == 16, "the T_MAX templates end at 16");
    if (forced != 0 && forced != 1) SZN_FAIL(SZN_ERR_ARG, "conse_head: forced must be 0 or 1, got %d", forced);
    if (forced && (n_gammas != 0 || gammas || hist))
        SZN_FAIL(SZN_ERR_ARG, "conse_head: a forced call takes no gammas and no hist (n_gammas 0, both NULL)");
    if (!forced && n_gammas == 0) SZN_FAIL(SZN_ERR_ARG, "conse_head: n_gammas outside [1, SZN_CALIB_MAX_GAMMAS]");
    if (const char* why = conse_bad_geometry(stride, B, h, w, E, K, n_gammas)) SZN_FAIL(SZN_ERR_ARG, "conse_head: %s", why);
    if (top_t < 1 || top_t > SZN_CONSE_MAX_TOP) SZN_FAIL(SZN_ERR_ARG, "conse_head: top_t %d outside [1, SZN_CONSE_MAX_TOP]", top_t);
    if (!coarse || !embed || !workspace) SZN_FAIL(SZN_ERR_ARG, "conse_head: coarse, embed and workspace are required");
    if (!forced && !gammas) SZN_FAIL(SZN_ERR_ARG, "conse_head: coarse, embed, workspace and gammas are required");
    if (c0 < 0 || ldc < c0 + K || H <= 0 || W <= 0 || crop < 0) SZN_FAIL(SZN_ERR_ARG, "conse_head: bad argument (ldc < c0 + K, H, W, crop)");
    if (H + crop > stride * h + stride || W + crop > stride * w + stride)
        SZN_FAIL(SZN_ERR_ARG, "conse_head: crop window exceeds the deconv output");
    if (((uintptr_t)workspace) & 15) SZN_FAIL(SZN_ERR_ARG, "conse_head: workspace must be 16-B aligned");
    const ClassBits ubits = class_bits(unseen);
    if (!class_bits_any(ubits)) SZN_FAIL(SZN_ERR_ARG, "conse_head: the unseen set is empty");
    if (!class_bits_fit(ubits, K)) SZN_FAIL(SZN_ERR_ARG, "conse_head: the unseen set names a class >= K = %d", K);
    int n_unseen = 0;
    for (int i = 0; i < 4; ++i) n_unseen += __builtin_popcountll(ubits.w[i]);
    if (n_unseen >= K) SZN_FAIL(SZN_ERR_ARG, "conse_head: every class below K = %d is unseen (both groups must be non-empty)", K);
    if (forced) {
        if (!target || !pred) SZN_FAIL(SZN_ERR_ARG, "conse_head: a forced call needs target and pred");
    } else {
        for (int g = 0; g < n_gammas; ++g) {
            if (!isfinite(gammas[g])) SZN_FAIL(SZN_ERR_ARG, "conse_head: gammas[%d] is not finite", g);
            if (g && !(gammas[g] > gammas[g - 1])) SZN_FAIL(SZN_ERR_ARG, "conse_head: gammas must be strictly ascending (at %d)", g);
        }
        if (!hist && !pred) SZN_FAIL(SZN_ERR_ARG, "conse_head: hist and pred are both NULL");
        if (hist && !target) SZN_FAIL(SZN_ERR_ARG, "conse_head: hist needs target");
        if (pred && (pred_index < 0 || pred_index >= n_gammas))
            SZN_FAIL(SZN_ERR_ARG, "conse_head: pred_index %d outside [0, %d)", pred_index, n_gammas);
    }
    if (conse_lds_bytes(stride, K, false) > CONSE_LDS_LIMIT)
        SZN_FAIL(SZN_ERR_UNSUPPORTED, "conse_head: K = %d: the cell's taps do not fit LDS", K);

    hipStream_t st = (hipStream_t)stream;
    const ConseWorkspace wl = conse_workspace(K, n_gammas);
    char* ws = (char*)workspace;
    CsArgs a{};
    a.coarse = coarse; a.target = target; a.G = (const float*)(ws + wl.G); a.en = (const float*)(ws + wl.en);
    a.B = B; a.h = h; a.w = w; a.K = K; a.ldc = ldc; a.c0 = c0; a.H = H; a.W = W; a.crop = crop;
    a.I0 = crop / stride; a.J0 = crop / stride;
    a.nI = (crop + H - 1) / stride - a.I0 + 1;
    a.nJ = (crop + W - 1) / stride - a.J0 + 1;
    a.ldg = conse_ldg(K);
    a.n_top = top_t < K - n_unseen ? top_t : K - n_unseen;
    a.forced = forced;
    a.unseen = ubits;
    CalArgs c{};
    for (int g = 0; g < n_gammas; ++g) c.gamma[g] = gammas[g];
    c.n = n_gammas; c.pred = pred; c.pred_index = (pred && !forced) ? pred_index : 0;

    hipLaunchKernelGGL(conse_prep_kernel, dim3(szn_div_up((long)K * K, 256)), dim3(256), 0, st, embed, K, E, a.ldg, (float*)(ws + wl.G),
                       (float*)(ws + wl.en));
    SZN_CHECK_LAUNCH("conse_prep_kernel");
    if (hist) {
        c.XA = (unsigned long long*)(ws + wl.XA); c.XB = (unsigned long long*)(ws + wl.XB);
        if (hipMemsetAsync(ws + wl.XA, 0, wl.bytes - wl.XA, st) != hipSuccess)
            SZN_FAIL(SZN_ERR_LAUNCH, "conse_head: clearing the crossing tables failed");
    }
    const bool glds = conse_lds_bytes(stride, K, true) <= CONSE_LDS_LIMIT;
    if (stride == 32) conse_launch_t<32>(a, c, glds, st);
    else conse_launch_t<8>(a, c, glds, st);
    SZN_CHECK_LAUNCH(glds ? "conse_cell_kernel" : "conse_cell_global_kernel");
    if (hist) {
        hipLaunchKernelGGL(calib_hist_kernel, dim3(szn_div_up((long)K * K, 256)), dim3(256), 0, st, (const unsigned long long*)c.XA,
                           (const unsigned long long*)c.XB, K, n_gammas, hist);
        SZN_CHECK_LAUNCH("calib_hist_kernel");
    }
    return SZN_OK;
}
