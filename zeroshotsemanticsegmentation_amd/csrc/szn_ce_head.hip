// szn_ce_head.hip -- the K-class softmax cross-entropy head fused from the coarse map, gfx950.
//
// Reference chain (models.py:94,146-147 upscore + crop; utils.py:19-48 cross_entropy2d; trainer_fcn.py:117 channel argmax):
//   score = fixed bilinear ConvTranspose2d(C, C, 2S, stride S)(coarse)[crop:crop+H, crop:crop+W]
//   loss  = sum (or mean) over valid pixels of -weight[t] * log_softmax(score)[t];   pred = first argmax over channels
//   d loss / d coarse through the same upscore.
// S = 32 is FCN32s' upscore, S = 8 the upscore8 stage of the FCN8s skip head.  The (B,C,H,W) score and its gradient never exist
// in HBM.  Every pixel of the S x S "pixel cell" (I, J) of the uncropped deconv output blends the same four coarse vectors
// (I-1,J-1), (I-1,J), (I,J-1), (I,J) (zero outside the map) with its own bilinear weights, so one cell needs 4 x C floats: they are
// staged in LDS (interleaved [c][tap]: one 16-B broadcast read per class) and the logits are recomputed from them in each of the
// three passes (argmax, sum of exps, gradient) instead of being held in registers.
//
// Mapping: S = 32: one 256-thread block per cell, 4 pixels per thread; S = 8: one wave per cell, 4 cells per block, 1 pixel per lane.
// Per-pixel arithmetic is that of up_fwd_kernel / ce_fwd_kernel / ce_bwd_kernel (szn_head.hip; -ffp-contract=off): the logits,
// the prediction and the loss terms are bit-identical to the materialised chain.  d(coarse) is accumulated as the per-cell table
// A[t][c] = sum_px w_t(px) * d_c(px): a lane sums over its own pixels, a reduce-scatter butterfly sums the wave (7 shuffles per
// class for the 4 taps), the waves of a cell are combined through LDS in a fixed order.  A gather kernel sums the <= 4 cells that
// use each coarse position.  Bilinear weights and tap <-> position mappings: szn_upcell.h.  Loss partials are doubles per cell, combined in a fixed order by a one-block finalize kernel, which
// also forms the 1/N of size_average (the gradient is linear in it: the cell pass runs with N = 1).  No atomics anywhere.
#include "szn_upcell.h"

namespace {

struct CeGeom {
    int B, h, w, C, ldc, c0, H, W, crop;
    int I0, J0, nI, nJ;          // the pixel cells the crop window touches: I in [I0, I0 + nI), J likewise
};

// workspace cell index: every (b, I, J) with I in [0, h], J in [0, w] has a slot (the window is a sub-range)
__device__ __forceinline__ long ce_cell_id(const CeGeom& g, int b, int I, int J) { return ((long)b * (g.h + 1) + I) * (g.w + 1) + J; }

__device__ __forceinline__ float ce_logit(const float4 t, const float (&w)[4]) {
    float acc = fmaf(t.x, w[0], 0.f);            // up_fwd_kernel's order: (I-1,J-1), (I-1,J), (I,J-1), (I,J)
    acc = fmaf(t.y, w[1], acc);
    acc = fmaf(t.z, w[2], acc);
    acc = fmaf(t.w, w[3], acc);
    return acc;
}

// sum of (a0..a3) over the wave; lanes with (lane & 15) == 0 hold the total of tap (lane >> 4)
__device__ __forceinline__ float reduce4_scatter(float a0, float a1, float a2, float a3, int lane) {
    const bool h5 = (lane & 32) != 0;
    float k0 = h5 ? a2 : a0, k1 = h5 ? a3 : a1;
    const float s0 = h5 ? a0 : a2, s1 = h5 ? a1 : a3;
    k0 += __shfl_xor(s0, 32, 64);
    k1 += __shfl_xor(s1, 32, 64);
    const bool h4 = (lane & 16) != 0;
    float v = (h4 ? k1 : k0) + __shfl_xor(h4 ? k0 : k1, 16, 64);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// cellL[cell] = {sum of loss terms, valid pixels} (doubles); cellA[cell][tap][c] (GRAD)
template <int S, bool GRAD>
__global__ __launch_bounds__(256) void ce_cell_kernel(const float* __restrict__ coarse, const int64_t* __restrict__ target,
                                                      const float* __restrict__ cweight, int64_t* __restrict__ pred,
                                                      double* __restrict__ cellL, float* __restrict__ cellA, CeGeom g) {
    constexpr int TPC = S == 32 ? 256 : 64;      // threads per cell
    constexpr int PPT = S * S / TPC;             // pixels per thread
    constexpr int CPB = 256 / TPC;               // cells per block
    static_assert(PPT * TPC == S * S && CPB * TPC == 256, "cell mapping");
    extern __shared__ __attribute__((aligned(16))) float lds[];      // taps [CPB][C][4] | red [4 waves][4][C] (GRAD)
    __shared__ double dred[4][2];
    const int C = g.C;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lc = tid / TPC, ct = tid % TPC;
    const long ncell = (long)g.B * g.nI * g.nJ;
    const long q = (long)blockIdx.x * CPB + lc;
    const bool active = q < ncell;
    int b = 0, I = 0, J = 0;
    if (active) {
        J = g.J0 + (int)(q % g.nJ);
        const long t = q / g.nJ;
        I = g.I0 + (int)(t % g.nI);
        b = (int)(t / g.nI);
    }
    float* taps = lds + (long)lc * 4 * C;
    for (int k = ct; k < 4 * C; k += TPC) {
        const int c = k >> 2, tap = k & 3;
        const int i = tap_i(I, tap), j = tap_j(J, tap);
        taps[k] = (active && i >= 0 && i < g.h && j >= 0 && j < g.w) ? coarse[(((long)b * g.h + i) * g.w + j) * g.ldc + g.c0 + c] : 0.f;
    }
    __syncthreads();
    const float4* tv = (const float4*)taps;

    float wt[PPT][4];
    long pix[PPT];
    int lbl[PPT];
    bool inb[PPT];
#pragma unroll
    for (int r = 0; r < PPT; ++r) {
        const int p = ct + TPC * r, ty = p / S, tx = p % S;
        const int y = S * I + ty - g.crop, x = S * J + tx - g.crop;
        inb[r] = active && y >= 0 && y < g.H && x >= 0 && x < g.W;
        cell_weights<S>(ty, tx, wt[r]);
        pix[r] = inb[r] ? ((long)b * g.H + y) * g.W + x : 0;
        lbl[r] = -1;
        if (target && inb[r]) {
            const long l = target[pix[r]];
            if (l >= 0 && l < C) lbl[r] = (int)l;            // -1 unlabelled, -2 padding and >= C: ignored (szn_ce2d)
        }
    }

    // pass 1: max and first-index argmax (ce_fwd_kernel)
    float mx[PPT];
    int am[PPT];
    {
        const float4 t0 = tv[0];
#pragma unroll
        for (int r = 0; r < PPT; ++r) { mx[r] = ce_logit(t0, wt[r]); am[r] = 0; }
    }
    for (int c = 1; c < C; ++c) {
        const float4 t = tv[c];
#pragma unroll
        for (int r = 0; r < PPT; ++r) {
            const float s = ce_logit(t, wt[r]);
            if (s > mx[r]) { mx[r] = s; am[r] = c; }
        }
    }
    if (pred) {
#pragma unroll
        for (int r = 0; r < PPT; ++r)
            if (inb[r]) pred[pix[r]] = am[r];
    }
    if (!target) return;

    // pass 2: sum of exps in class order, the per-pixel term
    float se[PPT];
#pragma unroll
    for (int r = 0; r < PPT; ++r) se[r] = 0.f;
    for (int c = 0; c < C; ++c) {
        const float4 t = tv[c];
#pragma unroll
        for (int r = 0; r < PPT; ++r) se[r] += expf(ce_logit(t, wt[r]) - mx[r]);
    }
    double lsum = 0.0, lcnt = 0.0;
#pragma unroll
    for (int r = 0; r < PPT; ++r) {
        if (lbl[r] < 0) continue;
        double term = (double)(-(ce_logit(tv[lbl[r]], wt[r]) - mx[r] - logf(se[r])));
        if (cweight) term = (double)(cweight[lbl[r]] * (float)term);          // F.nll_loss(weight=): fp32 product
        lsum += term;
        lcnt += 1.0;
    }
    lsum = wave_sum_d(lsum);
    lcnt = wave_sum_d(lcnt);
    if (lane == 0) { dred[wave][0] = lsum; dred[wave][1] = lcnt; }

    if (GRAD) {
        // pass 3: d_c = g * (softmax_c - [c == label]) (ce_bwd_kernel with gout = 1, N = 1), A[t][c] = sum_px w_t * d_c
        float* red = lds + (long)CPB * 4 * C;
        float gq[PPT], inv[PPT];
#pragma unroll
        for (int r = 0; r < PPT; ++r) {
            const bool v = lbl[r] >= 0;
            gq[r] = v ? (cweight ? 1.f * cweight[lbl[r]] : 1.f) : 0.f;
            inv[r] = v ? 1.f / se[r] : 0.f;
        }
        for (int c = 0; c < C; ++c) {
            const float4 t = tv[c];
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
            for (int r = 0; r < PPT; ++r) {
                const float sm = expf(ce_logit(t, wt[r]) - mx[r]) * inv[r];
                const float d = gq[r] * (sm - (c == lbl[r] ? 1.f : 0.f));
                a0 = fmaf(wt[r][0], d, a0);
                a1 = fmaf(wt[r][1], d, a1);
                a2 = fmaf(wt[r][2], d, a2);
                a3 = fmaf(wt[r][3], d, a3);
            }
            const float v = reduce4_scatter(a0, a1, a2, a3, lane);
            if ((lane & 15) == 0) red[((long)wave * 4 + (lane >> 4)) * C + c] = v;
        }
    }
    __syncthreads();
    if (!active) return;
    const long cid = ce_cell_id(g, b, I, J);
    if (ct == 0) {
        double s = dred[wave][0], n = dred[wave][1];
        if (TPC == 256) { s = combine4(dred[0][0], dred[1][0], dred[2][0], dred[3][0]); n = combine4(dred[0][1], dred[1][1], dred[2][1], dred[3][1]); }
        cellL[cid * 2] = s;
        cellL[cid * 2 + 1] = n;
    }
    if (GRAD) {
        const float* red = lds + (long)CPB * 4 * C;
        float* out = cellA + cid * 4 * C;
        for (int k = ct; k < 4 * C; k += TPC) {
            float v;
            if (TPC == 256) v = combine4(red[k], red[4 * C + k], red[8 * C + k], red[12 * C + k]);
            else v = red[(long)wave * 4 * C + k];
            out[k] = v;
        }
    }
}

// one block: per image the sum of its cells' partials in a fixed order -> stats, loss; gscale = 1 / N (size_average) or 1
__global__ __launch_bounds__(256) void ce_finalize_kernel(const double* __restrict__ cellL, int size_average, float* __restrict__ loss,
                                                          float* __restrict__ stats, float* __restrict__ gscale, CeGeom g) {
    __shared__ double sh[4][2];
    const int t = threadIdx.x;
    const int per = g.nI * g.nJ;
    double tot = 0.0, totn = 0.0;
    float nf = 0.f;
    for (int b = 0; b < g.B; ++b) {
        double s = 0.0, n = 0.0;
        for (int k = t; k < per; k += 256) {
            const long cid = ce_cell_id(g, b, g.I0 + k / g.nJ, g.J0 + k % g.nJ);
            s += cellL[cid * 2];
            n += cellL[cid * 2 + 1];
        }
        s = wave_sum_d(s);
        n = wave_sum_d(n);
        __syncthreads();                     // the previous image's readers are done with sh
        if ((t & 63) == 0) { sh[t >> 6][0] = s; sh[t >> 6][1] = n; }
        __syncthreads();
        s = combine4(sh[0][0], sh[1][0], sh[2][0], sh[3][0]);
        n = combine4(sh[0][1], sh[1][1], sh[2][1], sh[3][1]);
        if (t == 0 && stats) { stats[2 * b] = (float)s; stats[2 * b + 1] = (float)n; }
        tot += s;
        totn += n;
        nf += (float)n;                      // ce_bwd_kernel's float sum of the per-image counts
    }
    if (t == 0) {
        loss[0] = (float)(size_average ? tot / totn : tot);
        gscale[0] = size_average ? (nf > 0.f ? 1.f / nf : 0.f) : 1.f;
    }
}

// dcoarse[b][i][j][c0 + c] = gscale * sum over the <= 4 window cells that use (i, j) of A[cell][tap][c]
template <typename T>
__global__ __launch_bounds__(256) void ce_gather_kernel(const float* __restrict__ cellA, const float* __restrict__ gscale,
                                                        T* __restrict__ dcoarse, CeGeom g) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)g.B * g.h * g.w * g.C) return;
    const int c = (int)(e % g.C);
    const long pos = e / g.C;
    const int j = (int)(pos % g.w);
    const int i = (int)((pos / g.w) % g.h);
    const int b = (int)(pos / ((long)g.w * g.h));
    float acc = 0.f;
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) {
        const int I = tap_cell_I(i, tap), J = tap_cell_J(j, tap);
        if (I < g.I0 || I >= g.I0 + g.nI || J < g.J0 || J >= g.J0 + g.nJ) continue;
        acc += cellA[(ce_cell_id(g, b, I, J) * 4 + tap) * g.C + c];
    }
    elem<T>::st(dcoarse + pos * g.ldc + g.c0 + c, acc * gscale[0]);
}

size_t ce_cells(int B, int h, int w) { return (size_t)B * (h + 1) * (w + 1); }

template <int S>
int ce_launch(const CeGeom& g, const float* coarse, const int64_t* target, const float* weight, int size_average, float* loss,
              float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace, hipStream_t st) {
    constexpr int CPB = S == 32 ? 1 : 4;
    const size_t ncell_all = ce_cells(g.B, g.h, g.w);
    char* ws = (char*)workspace;
    double* cellL = (double*)ws;
    float* cellA = (float*)(ws + align256(ncell_all * 2 * sizeof(double)));
    float* gscale = (float*)(ws + align256(ncell_all * 2 * sizeof(double)) + align256(ncell_all * 4 * g.C * sizeof(float)));
    const long ncell = (long)g.B * g.nI * g.nJ;
    const int blocks = szn_div_up(ncell, CPB);
    const bool grad = dcoarse != nullptr;
    const size_t lds = ((size_t)CPB * 4 * g.C + (grad ? (size_t)16 * g.C : 0)) * sizeof(float);
    if (grad) hipLaunchKernelGGL((ce_cell_kernel<S, true>), dim3(blocks), dim3(256), lds, st, coarse, target, weight, pred, cellL, cellA, g);
    else hipLaunchKernelGGL((ce_cell_kernel<S, false>), dim3(blocks), dim3(256), lds, st, coarse, target, weight, pred, cellL, cellA, g);
    SZN_CHECK_LAUNCH("ce_cell_kernel");
    if (!target) return SZN_OK;
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, st, cellL, size_average, loss, stats, gscale, g);
    SZN_CHECK_LAUNCH("ce_finalize_kernel");
    if (!grad) return SZN_OK;
    const int gblocks = szn_div_up((long)g.B * g.h * g.w * g.C, 256);
    if (dcoarse_dtype == SZN_F32)
        hipLaunchKernelGGL(ce_gather_kernel<float>, dim3(gblocks), dim3(256), 0, st, cellA, gscale, (float*)dcoarse, g);
    else if (dcoarse_dtype == SZN_BF16)
        hipLaunchKernelGGL(ce_gather_kernel<bf16_raw>, dim3(gblocks), dim3(256), 0, st, cellA, gscale, (bf16_raw*)dcoarse, g);
    else
        hipLaunchKernelGGL(ce_gather_kernel<f16_raw>, dim3(gblocks), dim3(256), 0, st, cellA, gscale, (f16_raw*)dcoarse, g);
    SZN_CHECK_LAUNCH("ce_gather_kernel");
    return SZN_OK;
}

}  // namespace

extern "C" size_t szn_fused_ce_head_workspace_bytes(int stride, int B, int h, int w, int C) {
    if ((stride != 32 && stride != 8) || B < 1 || h < 1 || w < 1 || C < 1 || C > SZN_MAX_CLASSES) return 0;
    const size_t n = ce_cells(B, h, w);
    return align256(n * 2 * sizeof(double)) + align256(n * 4 * C * sizeof(float)) + 256;
}

extern "C" int szn_fused_ce_head(int stride, int B, int h, int w, int C, int ldc, int c0, int H, int W, int crop,
                                 const float* coarse, const int64_t* target, const float* weight, int size_average,
                                 float* loss, float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse,
                                 void* workspace, szn_stream_t stream) {
    if (stride != 32 && stride != 8) SZN_FAIL(SZN_ERR_UNSUPPORTED, "szn_fused_ce_head: stride %d (32 and 8 are built)", stride);
    if (C > SZN_MAX_CLASSES) SZN_FAIL(SZN_ERR_UNSUPPORTED, "szn_fused_ce_head: C = %d > %d", C, SZN_MAX_CLASSES);
    if (B < 1 || h < 1 || w < 1 || C < 1 || H < 1 || W < 1 || crop < 0 || c0 < 0 || ldc < c0 + C)
        SZN_FAIL(SZN_ERR_ARG, "szn_fused_ce_head: bad geometry");
    if (H + crop > stride * h + stride || W + crop > stride * w + stride)
        SZN_FAIL(SZN_ERR_ARG, "szn_fused_ce_head: crop window [%d,%d)+%d exceeds the %dx%d deconv output", H, W, crop,
                 stride * h + stride, stride * w + stride);
    if (!coarse || !workspace) SZN_FAIL(SZN_ERR_ARG, "szn_fused_ce_head: null pointer");
    if ((target == nullptr) != (loss == nullptr)) SZN_FAIL(SZN_ERR_ARG, "szn_fused_ce_head: target and loss go together");
    if (!target && (!pred || stats || dcoarse)) SZN_FAIL(SZN_ERR_ARG, "szn_fused_ce_head: a call without target writes pred only");
    if (dcoarse && dcoarse_dtype != SZN_F32 && dcoarse_dtype != SZN_BF16 && dcoarse_dtype != SZN_F16)
        SZN_FAIL(SZN_ERR_ARG, "szn_fused_ce_head: dcoarse_dtype %d", dcoarse_dtype);
    CeGeom g;
    g.B = B; g.h = h; g.w = w; g.C = C; g.ldc = ldc; g.c0 = c0; g.H = H; g.W = W; g.crop = crop;
    g.I0 = crop / stride; g.J0 = crop / stride;
    g.nI = (crop + H - 1) / stride - g.I0 + 1;
    g.nJ = (crop + W - 1) / stride - g.J0 + 1;
    hipStream_t st = (hipStream_t)stream;
    if (stride == 32) return ce_launch<32>(g, coarse, target, weight, size_average, loss, stats, pred, dcoarse_dtype, dcoarse, workspace, st);
    return ce_launch<8>(g, coarse, target, weight, size_average, loss, stats, pred, dcoarse_dtype, dcoarse, workspace, st);
}
