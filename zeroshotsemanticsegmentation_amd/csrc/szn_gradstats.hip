// szn_gradstats.hip -- per-segment sums and sums of squares of a flat gradient buffer (fp32, or the 16-bit wire image of the exchange),
// taken on the device in a fixed order, and the clipping decision of a step made from them (torch.nn.utils.clip_grad_norm_'s rule).
//
// Reference site: trainer_fcn.py:160-162 prints score_fr's gradient sum every iteration; the reference does not clip.
#include "szn_common.h"

namespace {

// A segment is cut into chunks of GS_CHUNK elements from its own start; one block of 256 lanes reduces one chunk.  Lane t takes the
// 16-byte vectors (8-byte for 16-bit input) t, t + 256, ... of the chunk's aligned body in ascending order, four of them loaded before
// the first is used, then at most one of the <= 6 scalar elements in front of the first vector boundary and behind the last whole vector.
// Every element is widened to double before anything else: g * g is then exact (24 x 24 bits) and the additions are the only roundings.
// 16384 elements per chunk: the 135 M-element weight buffer of FCN32s is 8.3 K blocks, one round of the grid, and fc6 (102.8 M) leaves
// 6.3 K chunk pairs to the second kernel.
constexpr int GS_CHUNK = 16384;
constexpr int GS_THREADS = 256;

struct gs_table {                                   // travels by value in the kernel arguments: nothing is copied to the device
    int64_t seg_end[SZN_GRAD_STATS_MAX_SEGS];       // as given by the caller
    int chunk_begin[SZN_GRAD_STATS_MAX_SEGS + 1];   // first chunk of segment s; [n_seg] = the number of chunks
    int n_seg;
};

template <typename G> struct gs_src;                // four consecutive elements as one non-temporal load, and one element
template <> struct gs_src<float> {
    typedef f32x4_t vec_t;
    __device__ static __forceinline__ vec_t ldv(const void* g, long i) { return __builtin_nontemporal_load((const vec_t*)g + i); }
    __device__ static __forceinline__ double get(const vec_t& v, int e) { return (double)v[e]; }
    __device__ static __forceinline__ double ld1(const void* g, long i) { return (double)((const float*)g)[i]; }
};
typedef __attribute__((ext_vector_type(2))) uint32_t gs_u32x2_t;
template <typename G> struct gs_src16 {
    typedef gs_u32x2_t vec_t;
    __device__ static __forceinline__ vec_t ldv(const void* g, long i) { return __builtin_nontemporal_load((const vec_t*)g + i); }
    __device__ static __forceinline__ double get(const vec_t& v, int e) {
        return (double)from_bits16<G>((uint16_t)((v[e >> 1] >> ((e & 1) * 16)) & 0xffffu));
    }
    __device__ static __forceinline__ double ld1(const void* g, long i) { return (double)from_bits16<G>(((const uint16_t*)g)[i]); }
};
template <> struct gs_src<bf16_raw> : gs_src16<bf16_raw> {};
template <> struct gs_src<f16_raw> : gs_src16<f16_raw> {};

template <typename V, typename G> __device__ __forceinline__ void gs_add4(const V& v, double& s, double& q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { const double d = gs_src<G>::get(v, e); s += d; q += d * d; }
}

template <typename G>
__global__ __launch_bounds__(GS_THREADS) void grad_stats_chunk_kernel(const void* __restrict__ g, gs_table tab, double* __restrict__ ws) {
    const int b = blockIdx.x, t = threadIdx.x;
    int sg = 0;
    while (tab.chunk_begin[sg + 1] <= b) ++sg;           // (uniform: the table sits in scalar registers; empty segments own no chunk)
    const long seg_lo = sg ? tab.seg_end[sg - 1] : 0;
    const long lo = seg_lo + (long)(b - tab.chunk_begin[sg]) * GS_CHUNK;
    const long rem = tab.seg_end[sg] - lo;
    const long len = rem < GS_CHUNK ? rem : GS_CHUNK;    // >= 1
    constexpr int ES = (int)sizeof(G) == 4 ? 4 : 2;      // bytes per element; a vector is 4 elements
    const char* base = (const char*)g + lo * ES;
    long head = (long)(((4 * ES) - ((uintptr_t)base & (4 * ES - 1))) & (4 * ES - 1)) / ES;
    if (head > len) head = len;
    const long nvec = (len - head) >> 2;
    const void* body = base + head * ES;
    double s = 0.0, q = 0.0;
    long i = t;
    for (; i + 3 * GS_THREADS < nvec; i += 4 * GS_THREADS) {      // four vectors in flight per lane before the first use
        const auto v0 = gs_src<G>::ldv(body, i), v1 = gs_src<G>::ldv(body, i + GS_THREADS);
        const auto v2 = gs_src<G>::ldv(body, i + 2 * GS_THREADS), v3 = gs_src<G>::ldv(body, i + 3 * GS_THREADS);
        gs_add4<decltype(v0), G>(v0, s, q); gs_add4<decltype(v0), G>(v1, s, q);
        gs_add4<decltype(v0), G>(v2, s, q); gs_add4<decltype(v0), G>(v3, s, q);
    }
    for (; i < nvec; i += GS_THREADS) {
        const auto v0 = gs_src<G>::ldv(body, i);
        gs_add4<decltype(v0), G>(v0, s, q);
    }
    const long body_end = head + nvec * 4, rest = len - nvec * 4;      // scalar elements: [0, head) and [body_end, len), rest <= 6
    if (t < rest) {
        const long k = t < head ? t : body_end + (t - head);
        const double d = gs_src<G>::ld1(base, k);
        s += d; q += d * d;
    }
    // fixed tree: the wave's 64 lane partials by halving shuffles, then the four wave partials in ascending order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o, 64); q += __shfl_down(q, o, 64); }
    __shared__ double part[GS_THREADS / 64][2];
    if ((t & 63) == 0) { part[t >> 6][0] = s; part[t >> 6][1] = q; }
    __syncthreads();
    if (t == 0) {
        double S = part[0][0], Q = part[0][1];
#pragma unroll
        for (int w = 1; w < GS_THREADS / 64; ++w) { S += part[w][0]; Q += part[w][1]; }
        ws[2 * (long)b] = S;
        ws[2 * (long)b + 1] = Q;
    }
}

// one wave per segment: lane l adds the l-th of 64 contiguous runs of the segment's chunk pairs in ascending chunk order, lane 0 then
// adds the 64 run sums in ascending order.  A segment without chunks (empty) gives {0, 0}; rows are overwritten.
__global__ __launch_bounds__(64) void grad_stats_sum_kernel(gs_table tab, const double* __restrict__ ws, double* __restrict__ stats) {
    const int sg = blockIdx.x, l = threadIdx.x;
    const int c0 = tab.chunk_begin[sg], cnt = tab.chunk_begin[sg + 1] - c0;
    const int per = (cnt + 63) / 64;
    const int lo = l * per < cnt ? l * per : cnt, hi = lo + per < cnt ? lo + per : cnt;
    double s = 0.0, q = 0.0;
    for (int c = c0 + lo; c < c0 + hi; ++c) { s += ws[2 * (long)c]; q += ws[2 * (long)c + 1]; }
    __shared__ double run[64][2];
    run[l][0] = s; run[l][1] = q;
    __syncthreads();
    if (l == 0) {
        double S = run[0][0], Q = run[0][1];
        for (int r = 1; r < 64; ++r) { S += run[r][0]; Q += run[r][1]; }
        stats[2 * sg] = S;
        stats[2 * sg + 1] = Q;
    }
}

__global__ void clip_coef_kernel(int n_seg, const double* __restrict__ stats, float max_norm, float grad_scale, float* __restrict__ dyn,
                                 float* __restrict__ clip) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double total = 0.0;
    for (int s = 0; s < n_seg; ++s) total += stats[2 * s + 1];
    const double S = dyn ? (double)dyn[0] : 1.0;
    const double norm = sqrt(total) * (double)grad_scale / S;
    if (!(total - total == 0.0)) {                       // inf or NaN: an element was (finite fp32 squares cannot overflow a double)
        clip[0] = 1.f;
        clip[1] = (float)norm;
        if (dyn) dyn[1] = 1.f;                           // found_inf: the optimizer entries skip the step
        return;
    }
    const double d = norm + 1e-6;                        // torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6))
    const float coef = d > (double)max_norm ? (float)((double)max_norm / d) : 1.f;
    clip[0] = coef;
    clip[1] = (float)norm;
    clip[2] += coef < 1.f ? 1.f : 0.f;
    clip[3] += 1.f;
}

long gs_chunks(long len) { return (len + GS_CHUNK - 1) / GS_CHUNK; }

}  // namespace

extern "C" size_t szn_grad_stats_workspace_bytes(long n, int n_seg) {
    if (n < 0) n = 0;
    if (n_seg < 1) n_seg = 1;
    return (size_t)(n / GS_CHUNK + n_seg) * 2 * sizeof(double);      // every segment ends in at most one partial chunk
}

extern "C" int szn_grad_stats(long n, const void* grad, int grad_dtype, int n_seg, const int64_t* seg_end, double* stats,
                              void* workspace, szn_stream_t stream) {
    if (n < 0) SZN_FAIL(SZN_ERR_ARG, "grad_stats: n must be >= 0");
    if (n_seg < 1 || n_seg > SZN_GRAD_STATS_MAX_SEGS) SZN_FAIL(SZN_ERR_ARG, "grad_stats: n_seg must lie in [1, %d]", SZN_GRAD_STATS_MAX_SEGS);
    if (grad_dtype != SZN_F32 && !szn_is16(grad_dtype)) SZN_FAIL(SZN_ERR_ARG, "grad_stats: the gradient must be SZN_F32, SZN_BF16 or SZN_F16");
    if (!seg_end || !stats) SZN_FAIL(SZN_ERR_ARG, "grad_stats: NULL seg_end or stats");
    if (n > 0 && (!grad || !workspace)) SZN_FAIL(SZN_ERR_ARG, "grad_stats: NULL buffer");
    const uintptr_t esize = grad_dtype == SZN_F32 ? 4 : 2;
    if (((uintptr_t)grad & (esize - 1)) != 0 || (((uintptr_t)stats | (uintptr_t)workspace) & 7) != 0)
        SZN_FAIL(SZN_ERR_ARG, "grad_stats: the gradient must be aligned to its element size, stats and workspace to 8 bytes");
    gs_table tab;
    long prev = 0, chunks = 0;
    for (int s = 0; s < SZN_GRAD_STATS_MAX_SEGS; ++s) {
        if (s < n_seg) {
            if (seg_end[s] < prev || seg_end[s] > n) SZN_FAIL(SZN_ERR_ARG, "grad_stats: seg_end must ascend within [0, n]");
            tab.chunk_begin[s] = (int)chunks;
            chunks += gs_chunks(seg_end[s] - prev);
            prev = seg_end[s];
            if (chunks > 0x7fffffffL) SZN_FAIL(SZN_ERR_ARG, "grad_stats: too many chunks");
        } else {
            tab.chunk_begin[s] = (int)chunks;
        }
        tab.seg_end[s] = prev;
    }
    if (prev != n) SZN_FAIL(SZN_ERR_ARG, "grad_stats: seg_end[n_seg - 1] must equal n");
    tab.chunk_begin[SZN_GRAD_STATS_MAX_SEGS] = (int)chunks;
    tab.n_seg = n_seg;
    if (chunks > 0) {
        szn_by_dtype(grad_dtype, [&](auto gtag) {
            using G = decltype(gtag);
            hipLaunchKernelGGL(grad_stats_chunk_kernel<G>, dim3((unsigned)chunks), dim3(GS_THREADS), 0, (hipStream_t)stream, grad, tab,
                               (double*)workspace);
        });
    }
    SZN_CHECK_LAUNCH("grad_stats_chunk_kernel");
    hipLaunchKernelGGL(grad_stats_sum_kernel, dim3(n_seg), dim3(64), 0, (hipStream_t)stream, tab, (const double*)workspace, stats);
    SZN_CHECK_LAUNCH("grad_stats_sum_kernel");
    return SZN_OK;
}

extern "C" int szn_clip_coef(int n_seg, const double* stats, float max_norm, float grad_scale, float* scale_state, float* clip_state,
                             szn_stream_t stream) {
    if (n_seg < 1 || !stats || !clip_state) SZN_FAIL(SZN_ERR_ARG, "clip_coef: n_seg must be >= 1 and stats / clip_state not NULL");
    if (!(max_norm > 0.f)) SZN_FAIL(SZN_ERR_ARG, "clip_coef: max_norm must be > 0 (+inf: measure only)");
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, n_seg, stats, max_norm, grad_scale, scale_state,
                       clip_state);
    SZN_CHECK_LAUNCH("clip_coef_kernel");
    return SZN_OK;
}
