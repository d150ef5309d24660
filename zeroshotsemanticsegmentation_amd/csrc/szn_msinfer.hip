// szn_msinfer.hip -- multi-scale / mirrored inference: the view of the network input (szn_resize_flip_f32) and the view-ensemble
// embedding head (szn_ms_head), which reads the coarse maps of all views and writes the prediction at the original size without a
// per-pixel score in memory.  The contracts are stated in include/szn.h.
//
// An original pixel lands between 2 x 2 pixels of a view (the 11-bit map of szn_augment_u8); each of those blends the four coarse
// vectors of its stride-S cell (szn_upcell.h).  Adjacent view pixels lie in the same or in adjacent cells, so the pixel's composite
// score is a blend of at most 3 x 3 coarse vectors, s = sum_p W_p C_p, and the weights separate: W_p = ry[i] * rx[j].  Hence
//     s . e_k = sum_p W_p (C_p . e_k)                -> per-position table D[pos][KP]
//     |s|^2   = sum_{p,q} W_p W_q (C_p . C_q)        -> per-position Gram table N[pos][13]: q - p over the 13 offsets (0,0..2),
//                                                       (1,-2..2), (2,-2..2); the other 12 of the 5 x 5 are their mirror images
// Kernels, in launch order:
//   fh_prep_kernel    (szn_fused_head_prepare) the class matrix transposed + its norms, at the head of the workspace
//   ms_tables_kernel  per view: one wave per coarse position writes its row of D (ascending fmaf chain over E) and of N
//                     (64 strided partial chains + xor butterfly)
//   ms_pixel_kernel   one thread per original pixel: up to 64 class accumulators in registers across the view loop (classes above
//                     64 in further turns of the same loop), then the group rule and the first-index argmax; writes pred (and acc)
#include "szn_upcell.h"

namespace {

constexpr int kGram = 13, kGramLd = 16;       // Gram entries per position, and their row pitch (one 64-byte line)

// one axis of the position map: destination coordinate g of n_dst -> source taps i0, i1 of n_src with the 11-bit weight w of i1
struct MsAxis {
    int i0, i1, w;
};
__host__ __device__ __forceinline__ int ms_step(int n_src, int n_dst) { return (int)((((long)n_src << 16) + n_dst / 2) / n_dst); }
__device__ __forceinline__ MsAxis ms_axis(int g, int step, int n_src) {
    const long s = (((2 * (long)g + 1) * (long)step) >> 1) - 32768;          // pixel centres, 16.16
    const long hi = (long)(n_src - 1) << 16;
    const long sc = s < 0 ? 0 : (s > hi ? hi : s);
    MsAxis a;
    a.i0 = (int)(sc >> 16);
    a.i1 = a.i0 + 1 < n_src ? a.i0 + 1 : n_src - 1;
    a.w = (int)(sc & 0xffff) >> 5;
    return a;
}

// ---- the view of the input ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resize_flip_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                              int Hs, int Ws, int step_y, int step_x, int flip) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)Hs * Ws) return;
    const int yo = (int)(g / Ws), xo = (int)(g - (long)yo * Ws);
    const int b = blockIdx.y;
    const MsAxis ay = ms_axis(yo, step_y, H), ax = ms_axis(flip ? Ws - 1 - xo : xo, step_x, W);
    const int wy = ay.w, wx = ax.w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = in + ((long)b * 3 + c) * H * W;
        const double p00 = p[(long)ay.i0 * W + ax.i0], p01 = p[(long)ay.i0 * W + ax.i1];
        const double p10 = p[(long)ay.i1 * W + ax.i0], p11 = p[(long)ay.i1 * W + ax.i1];
        const double top = (2048 - wx) * p00 + wx * p01;
        const double bot = (2048 - wx) * p10 + wx * p11;
        out[((long)b * 3 + c) * Hs * Ws + g] = (float)(((2048 - wy) * top + wy * bot) / 4194304.0);
    }
}

// ---- the ensemble head -------------------------------------------------------------------------------------------------------------
struct MsView {
    const float* coarse;
    float* D;             // [B h w][KP]
    float* N;             // [B h w][kGramLd]
    int h, w, ldc, c0, Hs, Ws, flip, step_y, step_x;
};
struct MsArgs {
    MsView v[SZN_MS_MAX_VIEWS];
    const float* prep;    // embT [E][KP] | en [KP] | ent [KP]
    const int64_t* gmap;
    const int64_t* target;
    int64_t* pred;
    float* acc;
    ClassBits unseen;
    int n_views, S, B, E, K, KP, H, W, crop, gmode;
};

// Gram slot of the offset (di, dj), di in 0..2, dj in -2..2 (di == 0: dj >= 0)
__host__ __device__ __forceinline__ constexpr int gram_slot(int di, int dj) { return di == 0 ? dj : 3 + (di - 1) * 5 + (dj + 2); }

__global__ __launch_bounds__(256) void ms_tables_kernel(const float* __restrict__ coarse, const float* __restrict__ embT,
                                                        float* __restrict__ D, float* __restrict__ N, int B, int h, int w, int E,
                                                        int ldc, int c0, int KP) {
    extern __shared__ __attribute__((aligned(16))) float sm[];            // [4 waves][E]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long npos = (long)B * h * w;
    const long pos = (long)blockIdx.x * 4 + wave;
    const bool ok = pos < npos;
    const long p = ok ? pos : 0;
    const int b = (int)(p / (h * w)), r = (int)(p % (h * w));
    const int i = r / w, j = r % w;
    const float* cv = coarse + (size_t)p * ldc + c0;
    float* Cs = sm + wave * E;
    for (int c = lane; c < E; c += 64) Cs[c] = cv[c];
    __syncthreads();
    for (int k = lane; ok && k < KP; k += 64) {
        float g = 0.f;
        for (int c = 0; c < E; ++c) g = fmaf(Cs[c], embT[(size_t)c * KP + k], g);
        D[(size_t)pos * KP + k] = g;
    }
    for (int n = 0; n < kGramLd; ++n) {
        const int di = n < 3 ? 0 : 1 + (n - 3) / 5, dj = n < 3 ? n : (n - 3) % 5 - 2;
        const int ni = i + di, nj = j + dj;
        float q = 0.f;
        if (n < kGram && ni < h && nj >= 0 && nj < w) {                    // wave-uniform
            const float* nv = coarse + (((size_t)b * h + ni) * w + nj) * ldc + c0;
            for (int c = lane; c < E; c += 64) q = fmaf(Cs[c], nv[c], q);
        }
        q = wave_sum(q);
        if (ok && lane == 0) N[(size_t)pos * kGramLd + n] = q;
    }
}

// the weights of the three coarse rows (columns) base-1+{0,1,2} that the two view rows t.i0, t.i1 of one axis blend, in double (exact:
// 11-bit weights times the cell's taps, which are odd multiples of 1/(2S)); base = the first view row's cell
__device__ __forceinline__ void ms_axis_weights(const MsAxis& t, int S, int crop, int& base, double (&r)[3]) {
    r[0] = r[1] = r[2] = 0.0;
    const int Y0 = t.i0 + crop, Y1 = t.i1 + crop;
    base = Y0 / S;
    const int Yv[2] = {Y0, Y1}, av[2] = {2048 - t.w, t.w};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int I = Yv[j] / S, ty = Yv[j] - I * S, off = I - base;          // off = 0 | 1
        const double f1 = 1.0 - fabs((double)ty - ((double)S - 0.5)) / (double)S;          // bil1d<S>(ty): the cell's own vertex I
        const double f0 = 1.0 - fabs((double)(ty + S) - ((double)S - 0.5)) / (double)S;    // bil1d<S>(ty + S): vertex I - 1
        const double a = (double)av[j] / 2048.0;
        if (off == 0) { r[0] += a * f0; r[1] += a * f1; }
        else { r[1] += a * f0; r[2] += a * f1; }
    }
}

template <int CH>
__global__ __launch_bounds__(256) void ms_pixel_kernel(const MsArgs a) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)a.H * a.W) return;
    const int y = (int)(g / a.W), x = (int)(g - (long)y * a.W);
    const int b = blockIdx.y;
    const size_t pix = ((size_t)b * a.H + y) * a.W + x;
    const float* en = a.prep + (size_t)a.E * a.KP;
    bool take_unseen = false;
    if (a.gmode == 1) take_unseen = a.gmap[pix] == 0;
    else if (a.gmode == 2) take_unseen = in_set(a.unseen, a.target[pix]);
    int best = 0;
    float bv = 0.f;
    for (int k0 = 0; k0 < a.K; k0 += CH) {
        float acc[CH];
#pragma unroll
        for (int kk = 0; kk < CH; ++kk) acc[kk] = 0.f;
        for (int v = 0; v < a.n_views; ++v) {
            const MsView& vw = a.v[v];
            // ---- the 3 x 3 composite taps of this pixel in view v ----
            const MsAxis ay = ms_axis(y, vw.step_y, vw.Hs), ax = ms_axis(vw.flip ? a.W - 1 - x : x, vw.step_x, vw.Ws);
            int I0, J0;
            double ry[3], rx[3];
            ms_axis_weights(ay, a.S, a.crop, I0, ry);
            ms_axis_weights(ax, a.S, a.crop, J0, rx);
            float wt[9];
            size_t pos[9];                 // zero-weight and outside taps: weight 0, position 0 (read, then discarded)
#pragma unroll
            for (int p = 0; p < 9; ++p) {
                const int i = I0 - 1 + p / 3, j = J0 - 1 + p % 3;
                const bool in = i >= 0 && i < vw.h && j >= 0 && j < vw.w;
                wt[p] = in ? (float)(ry[p / 3] * rx[p % 3]) : 0.f;
                pos[p] = wt[p] != 0.f ? ((size_t)b * vw.h + i) * vw.w + j : 0;
            }
            // ---- |s|^2 from the Gram rows: the 9 squares and twice the 36 pairs p < q ----
            float ss = 0.f;
#pragma unroll
            for (int p = 0; p < 9; ++p) {
                const f32x4_t* np = (const f32x4_t*)(vw.N + pos[p] * kGramLd);
                const f32x4_t n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
                const float n[16] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, n3.x, n3.y, n3.z, n3.w};
                float row = wt[p] * n[0];
#pragma unroll
                for (int q = p + 1; q < 9; ++q) {
                    const float nq = wt[q] != 0.f ? n[gram_slot(q / 3 - p / 3, q % 3 - p % 3)] : 0.f;
                    row = fmaf(2.f * wt[q], nq, row);
                }
                if (wt[p] != 0.f) ss = fmaf(wt[p], row, ss);
            }
            const float sn = sqrtf(ss);
            // ---- the classes of this turn, four at a time ----
#pragma unroll
            for (int kk = 0; kk < CH; kk += 4) {
                if (k0 + kk < a.KP) {                                        // uniform; KP is a multiple of 4
                    float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int p = 0; p < 9; ++p) {
                        const f32x4_t t = *(const f32x4_t*)(vw.D + pos[p] * a.KP + k0 + kk);
                        if (wt[p] != 0.f) {
                            d[0] = fmaf(wt[p], t.x, d[0]); d[1] = fmaf(wt[p], t.y, d[1]);
                            d[2] = fmaf(wt[p], t.z, d[2]); d[3] = fmaf(wt[p], t.w, d[3]);
                        }
                    }
                    const f32x4_t e4 = *(const f32x4_t*)(en + k0 + kk);
                    acc[kk] += d[0] / (sn * e4.x); acc[kk + 1] += d[1] / (sn * e4.y);
                    acc[kk + 2] += d[2] / (sn * e4.z); acc[kk + 3] += d[3] / (sn * e4.w);
                }
            }
        }
        // ---- group rule and first-index argmax over this turn's classes ----
#pragma unroll
        for (int kk = 0; kk < CH; ++kk) {
            const int k = k0 + kk;
            if (k < a.K) {
                if (a.acc) a.acc[pix * a.K + k] = acc[kk];
                const bool in_group = a.gmode == 0 || (bool)((class_word(a.unseen, k >> 6) >> (k & 63)) & 1ull) == take_unseen;
                const float c = in_group ? acc[kk] : 0.f;
                if (k == 0 || c > bv) { bv = c; best = k; }
            }
        }
    }
    a.pred[pix] = best;
}

struct MsLayout {
    size_t D[SZN_MS_MAX_VIEWS], N[SZN_MS_MAX_VIEWS], bytes;       // byte offsets
};
MsLayout ms_layout(int B, int E, int KP, int n_views, const szn_ms_view_t* views) {
    MsLayout L;
    size_t at = align256(prep_floats(E, KP) * sizeof(float));
    for (int v = 0; v < n_views; ++v) {
        const size_t npos = (size_t)B * views[v].h * views[v].w;
        L.D[v] = at;
        at = align256(at + npos * KP * sizeof(float));
        L.N[v] = at;
        at = align256(at + npos * kGramLd * sizeof(float));
    }
    L.bytes = at;
    return L;
}

// what both entry points refuse about the geometry (NULL pointers apart); 0 = fine
const char* ms_bad_geometry(int stride, int B, int E, int K, int n_views, const szn_ms_view_t* views) {
    if (n_views < 1 || n_views > SZN_MS_MAX_VIEWS) return "n_views outside [1, SZN_MS_MAX_VIEWS]";
    if (stride != 8 && stride != 32) return "stride must be 8 or 32";
    if (!views) return "views is NULL";
    if (B <= 0 || B > 65535 || E <= 0 || K <= 0) return "B, E and K must be positive (B <= 65535)";
    if (K > SZN_MAX_CLASSES) return "K above SZN_MAX_CLASSES";
    for (int v = 0; v < n_views; ++v) {
        const szn_ms_view_t& s = views[v];
        if (s.h <= 0 || s.w <= 0 || s.c0 < 0 || s.ldc < s.c0 + E) return "a view's map: h, w must be positive, c0 >= 0, ldc >= c0 + E";
        if (s.Hs < 1 || s.Ws < 1) return "a view's Hs or Ws below 1";
        // h * w stays an int in the kernels, and the tables pass launches one wave per position: (B h w + 3) / 4 blocks
        if (s.h > 32767 || s.w > 32767 || ((long)B * s.h * s.w + 3) / 4 > 0x7fffffffL) return "a view's map is too large (h, w <= 32767, B h w < 2^33)";
    }
    return nullptr;
}

}  // namespace

extern "C" int szn_resize_flip_f32(int B, int H, int W, const float* in_nchw, int Hs, int Ws, int flip, float* out_nchw,
                                   szn_stream_t stream) {
    if (!in_nchw || !out_nchw) SZN_FAIL(SZN_ERR_ARG, "resize_flip_f32: in_nchw and out_nchw are required");
    if (B <= 0 || H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0 || B > 65535 || H > 32767 || W > 32767)
        SZN_FAIL(SZN_ERR_ARG, "resize_flip_f32: bad shape (B %d, %d x %d -> %d x %d)", B, H, W, Hs, Ws);
    const long n = (long)Hs * Ws;
    if ((n + 255) / 256 > 0x7fffffffL) SZN_FAIL(SZN_ERR_ARG, "resize_flip_f32: view %d x %d too large", Hs, Ws);
    hipLaunchKernelGGL(resize_flip_f32_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, in_nchw,
                       out_nchw, H, W, Hs, Ws, ms_step(H, Hs), ms_step(W, Ws), flip ? 1 : 0);
    SZN_CHECK_LAUNCH("resize_flip_f32_kernel");
    return SZN_OK;
}

extern "C" size_t szn_ms_head_workspace_bytes(int stride, int B, int E, int K, int n_views, const szn_ms_view_t* views) {
    if (ms_bad_geometry(stride, B, E, K, n_views, views)) return 0;
    return ms_layout(B, E, kp_of(K), n_views, views).bytes;
}

extern "C" int szn_ms_head(int stride, int B, int E, int K, int H, int W, int crop, int n_views, const szn_ms_view_t* views,
                           const float* embed, const szn_class_set* unseen, int group_mode, const int64_t* group_map,
                           const int64_t* target, int64_t* pred, float* acc, void* workspace, szn_stream_t stream) {
    if (const char* why = ms_bad_geometry(stride, B, E, K, n_views, views)) SZN_FAIL(SZN_ERR_ARG, "ms_head: %s", why);
    if (!embed || !pred || !workspace) SZN_FAIL(SZN_ERR_ARG, "ms_head: embed, pred and workspace are required");
    if (((uintptr_t)workspace) & 15) SZN_FAIL(SZN_ERR_ARG, "ms_head: workspace must be 16-B aligned");
    if (H <= 0 || W <= 0 || H > 32767 || W > 32767 || crop < 0) SZN_FAIL(SZN_ERR_ARG, "ms_head: bad output size %d x %d or crop %d", H, W, crop);
    for (int v = 0; v < n_views; ++v) {
        const szn_ms_view_t& s = views[v];
        if (!s.coarse) SZN_FAIL(SZN_ERR_ARG, "ms_head: view %d has no coarse map", v);
        if (s.Hs > 32767 || s.Ws > 32767) SZN_FAIL(SZN_ERR_ARG, "ms_head: view %d is %d x %d (at most 32767)", v, s.Hs, s.Ws);
        if (s.Hs + crop > stride * s.h + stride || s.Ws + crop > stride * s.w + stride)
            SZN_FAIL(SZN_ERR_ARG, "ms_head: view %d: crop window [%d,%d)+%d exceeds the %dx%d deconv output", v, s.Hs, s.Ws, crop,
                     stride * s.h + stride, stride * s.w + stride);
    }
    if (group_mode < 0 || group_mode > 2) SZN_FAIL(SZN_ERR_ARG, "ms_head: bad group mode %d", group_mode);
    if (group_mode == 1 && !group_map) SZN_FAIL(SZN_ERR_ARG, "ms_head: group mode 1 needs group_map");
    if (group_mode == 2 && !target) SZN_FAIL(SZN_ERR_ARG, "ms_head: group mode 2 needs target");
    const ClassBits ubits = class_bits(unseen);
    if (!class_bits_fit(ubits, K)) SZN_FAIL(SZN_ERR_ARG, "ms_head: the unseen set names a class >= K = %d", K);
    const long npix = (long)H * W;
    if ((size_t)4 * E * sizeof(float) > 60 * 1024) SZN_FAIL(SZN_ERR_UNSUPPORTED, "ms_head: E=%d too large for LDS", E);

    hipStream_t st = (hipStream_t)stream;
    const int KP = kp_of(K);
    const MsLayout L = ms_layout(B, E, KP, n_views, views);
    char* ws = (char*)workspace;
    int rc = szn_fused_head_prepare(E, K, embed, workspace, stream);
    if (rc) return rc;
    MsArgs a{};
    for (int v = 0; v < n_views; ++v) {
        const szn_ms_view_t& s = views[v];
        MsView& d = a.v[v];
        d.coarse = s.coarse; d.D = (float*)(ws + L.D[v]); d.N = (float*)(ws + L.N[v]);
        d.h = s.h; d.w = s.w; d.ldc = s.ldc; d.c0 = s.c0; d.Hs = s.Hs; d.Ws = s.Ws; d.flip = s.flip ? 1 : 0;
        d.step_y = ms_step(s.Hs, H); d.step_x = ms_step(s.Ws, W);
        const long npos = (long)B * s.h * s.w;
        hipLaunchKernelGGL(ms_tables_kernel, dim3((unsigned)((npos + 3) / 4)), dim3(256), (size_t)4 * E * sizeof(float), st, s.coarse,
                           (const float*)workspace, d.D, d.N, B, s.h, s.w, E, s.ldc, s.c0, KP);
        SZN_CHECK_LAUNCH("ms_tables_kernel");
    }
    a.prep = (const float*)workspace; a.gmap = group_map; a.target = target; a.pred = pred; a.acc = acc; a.unseen = ubits;
    a.n_views = n_views; a.S = stride; a.B = B; a.E = E; a.K = K; a.KP = KP; a.H = H; a.W = W; a.crop = crop; a.gmode = group_mode;
    const dim3 grid((unsigned)((npix + 255) / 256), (unsigned)B);
    if (KP <= 32) hipLaunchKernelGGL(ms_pixel_kernel<32>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(ms_pixel_kernel<64>, grid, dim3(256), 0, st, a);
    SZN_CHECK_LAUNCH("ms_pixel_kernel");
    return SZN_OK;
}
