// szn_pool.hip -- MaxPool2d(2, 2, ceil_mode=True) on NHWC: forward (optionally with winner codes), backward with the ReLU gate of the
// conv in front of it, from the pool's input or from the winner codes; column sums of din = that conv's bias gradient.
//
// Reference sites: models.py:43-47 (pools).
#include "szn_common.h"

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;

namespace {

// ---- MaxPool2d(2,2,ceil_mode=True) on NHWC: thread = (output pixel, 16-B channel chunk) -----------
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ in, T* __restrict__ out, int B, int Hi,
                                                          int Wi, int C, int Ho, int Wo, uint8_t* __restrict__ code) {
    constexpr int CH = elem<T>::kPer16B;
    const int cpp = C / CH;
    const long total = (long)B * Ho * Wo * cpp;
    for (long gid = (long)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (long)gridDim.x * 256) {
        const int cc = (int)(gid % cpp);
        const long p = gid / cpp;
        const int ow = (int)(p % Wo);
        const long t = p / Wo;
        const int oh = (int)(t % Ho), b = (int)(t / Ho);
        float best[CH];
        int win[CH];                                     // position (2 dy + dx) of the FIRST maximum (strict >, scan order)
#pragma unroll
        for (int e = 0; e < CH; ++e) { best[e] = -INFINITY; win[e] = 0; }
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int ih = 2 * oh + dy;
            if (ih >= Hi) continue;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int iw = 2 * ow + dx;
                if (iw >= Wi) continue;
                const u32x4_t v = *(const u32x4_t*)(in + (((long)b * Hi + ih) * Wi + iw) * C + cc * CH);
                const T* ve = (const T*)&v;
#pragma unroll
                for (int e = 0; e < CH; ++e) {
                    const float x = elem<T>::ld(ve + e);
                    if (x > best[e]) { best[e] = x; win[e] = 2 * dy + dx; }
                }
            }
        }
        u32x4_t o;
        T* oe = (T*)&o;
#pragma unroll
        for (int e = 0; e < CH; ++e) elem<T>::st(oe + e, best[e]);
        *(u32x4_t*)(out + p * C + cc * CH) = o;
        if (code) {                                      // winner code per pooled element: 0 .. 3, or 4 = maximum not positive (ReLU gate)
            uint8_t* cp = code + p * C + cc * CH;
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const uint32_t cd = best[e] > 0.f ? (uint32_t)win[e] : 4u;
                if (e < 4) lo |= cd << (8 * e); else hi |= cd << (8 * (e - 4));
            }
            *(uint32_t*)cp = lo;
            if (CH == 8) *(uint32_t*)(cp + 4) = hi;
        }
    }
}

// din[b][ih][iw][c] = (in is the FIRST max of its window, scan order (0,0),(0,1),(1,0),(1,1)) ? dout[win] : 0,
// then gated by in > 0 (the ReLU in front of every pool).  thread = (OUTPUT pixel, 16-B chunk): the 2x2 window is
// loaded once (4 + 1 loads, 4 stores per 4 input pixels; the pooled tensor itself is not needed -- its value is the
// window maximum).  `out` stays in the signature for the C-ABI.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ in, const T* __restrict__ out,
                                                          const T* __restrict__ dout, T* __restrict__ din, int B, int Hi,
                                                          int Wi, int C, int Ho, int Wo, float* __restrict__ colsum,
                                                          float* __restrict__ cslab) {
    constexpr int CH = elem<T>::kPer16B;
    __shared__ float red[256 * CH];
    (void)out;
    const int cpp = C / CH;
    const long total = (long)B * Ho * Wo * cpp;
    float cs[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) cs[e] = 0.f;
    for (long gid = (long)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (long)gridDim.x * 256) {
        const int cc = (int)(gid % cpp);
        const long po = gid / cpp;
        const int ow = (int)(po % Wo);
        const long t = po / Wo;
        const int oh = (int)(t % Ho), b = (int)(t / Ho);
        const int ih = 2 * oh, iw = 2 * ow;
        const bool okw = iw + 1 < Wi, okh = ih + 1 < Hi;
        const long p00 = ((long)b * Hi + ih) * Wi + iw;
        const T* ip = in + p00 * C + cc * CH;
        u32x4_t v[4];
        const u32x4_t zero = {0, 0, 0, 0};
        v[0] = *(const u32x4_t*)ip;
        v[1] = okw ? *(const u32x4_t*)(ip + C) : zero;
        v[2] = okh ? *(const u32x4_t*)(ip + (long)Wi * C) : zero;
        v[3] = (okh && okw) ? *(const u32x4_t*)(ip + (long)Wi * C + C) : zero;
        const u32x4_t vd = *(const u32x4_t*)(dout + po * C + cc * CH);
        const T* de = (const T*)&vd;
        const bool ok[4] = {true, okw, okh, okh && okw};
        u32x4_t o[4];
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            float s[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = elem<T>::ld((const T*)&v[k] + e);
            float m = s[0];
            int win = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (ok[k] && s[k] > m) { m = s[k]; win = k; }       // strict >: the first maximum keeps the gradient
            const float dv = (m > 0.f) ? elem<T>::ld(de + e) : 0.f;  // ReLU gate of the winner
#pragma unroll
            for (int k = 0; k < 4; ++k) elem<T>::st((T*)&o[k] + e, k == win ? dv : 0.f);
            cs[e] += elem<T>::ld((const T*)&o[0] + e) + elem<T>::ld((const T*)&o[1] + e) +
                     elem<T>::ld((const T*)&o[2] + e) + elem<T>::ld((const T*)&o[3] + e);   // what was stored (one non-zero term)
        }
        T* op = din + p00 * C + cc * CH;
        *(u32x4_t*)op = o[0];
        if (okw) *(u32x4_t*)(op + C) = o[1];
        if (okh) *(u32x4_t*)(op + (long)Wi * C) = o[2];
        if (okh && okw) *(u32x4_t*)(op + (long)Wi * C + C) = o[3];
    }
    if (colsum) {
        // bias gradient of the conv in front of this pool: column sums of din.  The launcher makes the grid stride a
        // multiple of cpp, so a thread keeps one channel chunk (cc = threadIdx.x % cpp) for all its pixels.
#pragma unroll
        for (int e = 0; e < CH; ++e) red[threadIdx.x * CH + e] = cs[e];
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            const int cc = c / CH, e = c - cc * CH;
            float t = 0.f;
            for (int r = cc; r < 256; r += cpp) t += red[r * CH + e];
            if (cslab) cslab[(long)blockIdx.x * C + c] = t;      // one partial row per block, reduced in a fixed order later
            else if (t != 0.f) atomicAdd(colsum + c, t);
        }
    }
}

// The same backward pass from the WINNER CODES the forward pass wrote (szn_conv_desc_t.pool_code / szn_maxpool2x2_ceil_fwd_code)
// instead of the pool's input: code 0 .. 3 = position 2 dy + dx of the first maximum, 4 = maximum not positive (no gradient: the
// ReLU gate).  2.75 B instead of 4.5 B of traffic per input element, and the forward pass no longer has to store the un-pooled
// tensor for this kernel alone.  Same result bit for bit.
// SKIP = 1 / 2: one / two more sets of column sums, over the pixels of din inside rows x columns {fy0, fy1, fx0, fx1} and outside {wy0, wy1,
// wx0, wx1} (all even: a 2 x 2 window never straddles them) -- the regions the consumers of din do not run tile by tile but replace by
// region sums: the weight gradient of the conv in front of the pool (szn_conv2d_wgrad_cb_region) and that conv's dgrad
// (szn_conv2d_dgrad_border_region).  Rows of cslab2 [SKIP][rows][C] like cslab's.
struct PoolSkip { int fy0, fy1, fx0, fx1, wy0, wy1, wx0, wx1; };
// GATHER (round 5, szn_maxpool2x2_ceil_bwd_code_gather): the gradient of pooled pixel (oh, ow) is not dout[oh][ow] but the SUM of the source block
// rows ytab[oh] = {start, count} x columns xtab[ow] = {start, count} of dout [B][Hs][Ws][C] -- the transposed band map (szn_band_remap's backward
// forms: a plain shift for almost every pixel, the few rows / columns that stood in for removed copies sum theirs), read here instead of being
// applied by two passes over the tensor in front of this kernel.  fp32 sum, rounded once; count 1 x 1 moves the bits; count 0 = no gradient.
struct PoolGather { const int* ytab; const int* xtab; int Hs, Ws; };
template <typename T, int SKIP, bool GATHER = false>
__global__ __launch_bounds__(256) void maxpool_bwd_code_kernel(const uint8_t* __restrict__ code, const T* __restrict__ dout,
                                                               T* __restrict__ din, int B, int Hi, int Wi, int C, int Ho, int Wo,
                                                               float* __restrict__ colsum, float* __restrict__ cslab, PoolSkip sk,
                                                               PoolSkip sk2, float* __restrict__ cslab2, PoolGather pg = PoolGather{}) {
    constexpr int CH = elem<T>::kPer16B;
    __shared__ float red[256 * CH];
    const int cpp = C / CH;
    const long total = (long)B * Ho * Wo * cpp;
    float cs[CH], cs2[CH], cs3[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) { cs[e] = 0.f; cs2[e] = 0.f; cs3[e] = 0.f; }
    for (long gid = (long)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (long)gridDim.x * 256) {
        const int cc = (int)(gid % cpp);
        const long po = gid / cpp;
        const int ow = (int)(po % Wo);
        const long t = po / Wo;
        const int oh = (int)(t % Ho), b = (int)(t / Ho);
        const int ih = 2 * oh, iw = 2 * ow;
        const bool okw = iw + 1 < Wi, okh = ih + 1 < Hi;
        const long p00 = ((long)b * Hi + ih) * Wi + iw;
        u32x4_t vd;
        if constexpr (GATHER) {
            const int2 ye = ((const int2*)pg.ytab)[oh], xe = ((const int2*)pg.xtab)[ow];          // {start, count}: one 8-B load per axis
            const int ys = ye.x, yc = ye.y, xs = xe.x, xc = xe.y;
            const T* src = dout + (((long)b * pg.Hs + ys) * pg.Ws + xs) * C + cc * CH;
            if (yc == 1 && xc == 1) {
                vd = *(const u32x4_t*)src;
            } else {
                float acc[CH];
#pragma unroll
                for (int e = 0; e < CH; ++e) acc[e] = 0.f;
                for (int yy = 0; yy < yc; ++yy)
                    for (int xx = 0; xx < xc; ++xx) {
                        const u32x4_t q = *(const u32x4_t*)(src + ((long)yy * pg.Ws + xx) * C);
#pragma unroll
                        for (int e = 0; e < CH; ++e) acc[e] += elem<T>::ld((const T*)&q + e);
                    }
#pragma unroll
                for (int e = 0; e < CH; ++e) elem<T>::st((T*)&vd + e, acc[e]);
            }
        } else {
            vd = *(const u32x4_t*)(dout + po * C + cc * CH);
        }
        const T* de = (const T*)&vd;
        const uint8_t* cp = code + po * C + cc * CH;
        const uint32_t clo = *(const uint32_t*)cp, chi = CH == 8 ? *(const uint32_t*)(cp + 4) : 0u;
        const bool skip = SKIP >= 1 && ih >= sk.fy0 && ih < sk.fy1 && iw >= sk.fx0 && iw < sk.fx1 &&
                          !(ih >= sk.wy0 && ih < sk.wy1 && iw >= sk.wx0 && iw < sk.wx1);
        const bool skipb = SKIP >= 2 && ih >= sk2.fy0 && ih < sk2.fy1 && iw >= sk2.fx0 && iw < sk2.fx1 &&
                           !(ih >= sk2.wy0 && ih < sk2.wy1 && iw >= sk2.wx0 && iw < sk2.wx1);
        u32x4_t o[4];
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            const int win = (int)(((e < 4 ? clo : chi) >> (8 * (e & 3))) & 0xffu);
            const float dv = elem<T>::ld(de + e);                  // a value of type T: storing it back is exact
#pragma unroll
            for (int k = 0; k < 4; ++k) elem<T>::st((T*)&o[k] + e, k == win ? dv : 0.f);
            cs[e] += win < 4 ? dv : 0.f;                           // what was stored (one non-zero term)
            if (SKIP >= 1) cs2[e] += (skip && win < 4) ? dv : 0.f;
            if (SKIP >= 2) cs3[e] += (skipb && win < 4) ? dv : 0.f;
        }
        T* op = din + p00 * C + cc * CH;
        *(u32x4_t*)op = o[0];
        if (okw) *(u32x4_t*)(op + C) = o[1];
        if (okh) *(u32x4_t*)(op + (long)Wi * C) = o[2];
        if (okh && okw) *(u32x4_t*)(op + (long)Wi * C + C) = o[3];
    }
    if (colsum) {
#pragma unroll
        for (int e = 0; e < CH; ++e) red[threadIdx.x * CH + e] = cs[e];
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            const int cc = c / CH, e = c - cc * CH;
            float t = 0.f;
            for (int r = cc; r < 256; r += cpp) t += red[r * CH + e];
            if (cslab) cslab[(long)blockIdx.x * C + c] = t;
            else if (t != 0.f) atomicAdd(colsum + c, t);
        }
    }
#pragma unroll
    for (int m = 0; m < SKIP; ++m) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < CH; ++e) red[threadIdx.x * CH + e] = m == 0 ? cs2[e] : cs3[e];
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            const int cc = c / CH, e = c - cc * CH;
            float t = 0.f;
            for (int r = cc; r < 256; r += cpp) t += red[r * CH + e];
            cslab2[((long)m * gridDim.x + blockIdx.x) * C + c] = t;
        }
    }
}

// out[c] = sum over the rows of slab [rows][C], fixed order (four running sums per thread group, then a tree over 32 groups)
__global__ __launch_bounds__(256) void slab_rows_sum_kernel(const float* __restrict__ slab, int rows, int C, float* __restrict__ out) {
    __shared__ float part[32][8];
    const int cl = threadIdx.x & 7, grp = threadIdx.x >> 3, c = blockIdx.x * 8 + cl;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (c < C) {
        int r = grp;
        for (; r + 96 < rows; r += 128) {
            s0 += slab[(size_t)r * C + c]; s1 += slab[(size_t)(r + 32) * C + c];
            s2 += slab[(size_t)(r + 64) * C + c]; s3 += slab[(size_t)(r + 96) * C + c];
        }
        for (; r < rows; r += 32) s0 += slab[(size_t)r * C + c];
    }
    part[grp][cl] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (threadIdx.x < 8 && c < C) {
        float t = 0.f;
        for (int g2 = 0; g2 < 32; ++g2) t += part[g2][cl];
        out[c] = t;
    }
}

}  // namespace

extern "C" int szn_maxpool2x2_ceil_fwd_code(int dtype, int B, int Hi, int Wi, int C, const void* in, void* out, void* code,
                                            szn_stream_t stream);
extern "C" int szn_maxpool2x2_ceil_fwd(int dtype, int B, int Hi, int Wi, int C, const void* in, void* out,
                                       szn_stream_t stream) {
    return szn_maxpool2x2_ceil_fwd_code(dtype, B, Hi, Wi, C, in, out, nullptr, stream);
}

extern "C" int szn_maxpool2x2_ceil_fwd_code(int dtype, int B, int Hi, int Wi, int C, const void* in, void* out, void* code,
                                            szn_stream_t stream) {
    if (!in || !out || B <= 0 || Hi <= 0 || Wi <= 0 || C <= 0) SZN_FAIL(SZN_ERR_ARG, "maxpool_fwd: bad argument");
    if (code && (((uintptr_t)code) & 3)) SZN_FAIL(SZN_ERR_ARG, "maxpool_fwd: code must be 4-B aligned");
    const int ch = szn_is16(dtype) ? 8 : 4;
    if (C % ch) SZN_FAIL(SZN_ERR_UNSUPPORTED, "maxpool_fwd: C must be a multiple of %d", ch);
    const int Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2;
    const long total = (long)B * Ho * Wo * (C / ch);
    const bool known = szn_by_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(maxpool_fwd_kernel<T>, dim3(szn_grid_for(total, 256, 65536)), dim3(256), 0, (hipStream_t)stream, (const T*)in,
                           (T*)out, B, Hi, Wi, C, Ho, Wo, (uint8_t*)code);
    });
    if (!known) SZN_FAIL(SZN_ERR_ARG, "maxpool_fwd: bad dtype %d", dtype);
    SZN_CHECK_LAUNCH("maxpool_fwd_kernel");
    return SZN_OK;
}

extern "C" int szn_maxpool2x2_ceil_bwd(int dtype, int B, int Hi, int Wi, int C, const void* in, const void* out,
                                       const void* dout, void* din, float* colsum, float* colsum_slab, int colsum_slab_rows,
                                       int* colsum_rows_out, szn_stream_t stream) {
    if (colsum_rows_out) *colsum_rows_out = 0;
    if (!in || !out || !dout || !din || B <= 0 || Hi <= 0 || Wi <= 0 || C <= 0)
        SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd: bad argument");
    const int ch = szn_is16(dtype) ? 8 : 4;
    if (C % ch) SZN_FAIL(SZN_ERR_UNSUPPORTED, "maxpool_bwd: C must be a multiple of %d", ch);
    const int Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2;
    const long total = (long)B * Ho * Wo * (C / ch);
    if (colsum && (256 % (C / ch)) != 0) SZN_FAIL(SZN_ERR_UNSUPPORTED, "maxpool_bwd: colsum needs C/%d to divide 256", ch);
    // with column sums every block ends in C atomicAdds on the same C addresses: 4096 blocks spent more time there than streaming
    // (pool3 .. pool5); two blocks per CU stream at 5.3 TB/s (tools/bench sweep in profiles/r02_ablations.txt section 13)
    const int grid = szn_grid_for(total, 256, colsum ? 512 : 65536);
    float* cslab = colsum ? colsum_slab : nullptr;
    if (cslab && colsum_slab_rows < grid)
        SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd: colsum_slab holds %d rows, %d needed", colsum_slab_rows, grid);
    szn_note_colsum_rows(cslab ? grid : 0);
    if (colsum_rows_out) *colsum_rows_out = cslab ? grid : 0;
    const bool known = szn_by_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)in, (const T*)out,
                           (const T*)dout, (T*)din, B, Hi, Wi, C, Ho, Wo, colsum, cslab);
    });
    if (!known) SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd: bad dtype %d", dtype);
    SZN_CHECK_LAUNCH("maxpool_bwd_kernel");
    return SZN_OK;
}

static int maxpool_bwd_code_impl(int dtype, int B, int Hi, int Wi, int C, const void* code, const void* dout, void* din, float* colsum,
                                 float* colsum_slab, int colsum_slab_rows, int* colsum_rows_out, const int* skip_tiles, int n_regions,
                                 float* skip_sum, float* skip_slab, szn_stream_t stream, const PoolGather* gather = nullptr) {
    if (colsum_rows_out) *colsum_rows_out = 0;
    if (!code || !dout || !din || B <= 0 || Hi <= 0 || Wi <= 0 || C <= 0) SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd_code: bad argument");
    const int ch = szn_is16(dtype) ? 8 : 4;
    if (C % ch) SZN_FAIL(SZN_ERR_UNSUPPORTED, "maxpool_bwd_code: C must be a multiple of %d", ch);
    if (((uintptr_t)code) & 3) SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd_code: code must be 4-B aligned");
    const int Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2;
    const long total = (long)B * Ho * Wo * (C / ch);
    const bool sums = colsum || skip_tiles;
    if (sums && (256 % (C / ch)) != 0) SZN_FAIL(SZN_ERR_UNSUPPORTED, "maxpool_bwd_code: colsum needs C/%d to divide 256", ch);
    if (skip_tiles && (!skip_sum || !skip_slab || !colsum || !colsum_slab || n_regions < 1 || n_regions > 2))
        SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd_code_cb: skip_sum, skip_slab, colsum, colsum_slab and 1 or 2 regions are required");
    if (skip_tiles)
        for (int i = 0; i < 8 * n_regions; ++i)
            if (skip_tiles[i] & 1) SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd_code_cb: region bounds must be even (2 x 2 windows must not straddle them)");
    const int grid = szn_grid_for(total, 256, sums ? 512 : 65536);      // (512: see szn_maxpool2x2_ceil_bwd)
    float* cslab = colsum ? colsum_slab : nullptr;
    if (cslab && colsum_slab_rows < grid)
        SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd_code: colsum_slab holds %d rows, %d needed", colsum_slab_rows, grid);
    szn_note_colsum_rows(cslab ? grid : 0);
    if (colsum_rows_out) *colsum_rows_out = cslab ? grid : 0;
    PoolSkip sk = {}, sk2 = {};
    if (skip_tiles) { sk.fy0 = skip_tiles[0]; sk.fy1 = skip_tiles[1]; sk.fx0 = skip_tiles[2]; sk.fx1 = skip_tiles[3];
                      sk.wy0 = skip_tiles[4]; sk.wy1 = skip_tiles[5]; sk.wx0 = skip_tiles[6]; sk.wx1 = skip_tiles[7]; }
    if (skip_tiles && n_regions == 2) { const int* q = skip_tiles + 8; sk2.fy0 = q[0]; sk2.fy1 = q[1]; sk2.fx0 = q[2]; sk2.fx1 = q[3];
                                        sk2.wy0 = q[4]; sk2.wy1 = q[5]; sk2.wx0 = q[6]; sk2.wx1 = q[7]; }
    const int nsk = skip_tiles ? n_regions : 0;
    hipStream_t st = (hipStream_t)stream;
    const PoolGather pg = gather ? *gather : PoolGather{};
    const bool known = szn_by_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, (const uint8_t*)code, (const T*)dout, (T*)din, B, Hi, Wi, C, Ho, Wo, colsum,
                               cslab, sk, sk2, skip_slab, pg);
        };
        if (gather) launch(maxpool_bwd_code_kernel<T, 0, true>);
        else if (nsk == 2) launch(maxpool_bwd_code_kernel<T, 2>);
        else if (nsk == 1) launch(maxpool_bwd_code_kernel<T, 1>);
        else launch(maxpool_bwd_code_kernel<T, 0>);
    });
    if (!known) SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd_code: bad dtype %d", dtype);
    SZN_CHECK_LAUNCH("maxpool_bwd_code_kernel");
    for (int m = 0; m < nsk; ++m) {
        hipLaunchKernelGGL(slab_rows_sum_kernel, dim3((unsigned)szn_div_up(C, 8)), dim3(256), 0, st, (const float*)skip_slab + (size_t)m * grid * C,
                           grid, C, skip_sum + (size_t)m * C);
        SZN_CHECK_LAUNCH("slab_rows_sum_kernel");
    }
    return SZN_OK;
}

extern "C" int szn_maxpool2x2_ceil_bwd_code(int dtype, int B, int Hi, int Wi, int C, const void* code, const void* dout, void* din,
                                            float* colsum, float* colsum_slab, int colsum_slab_rows, int* colsum_rows_out, szn_stream_t stream) {
    return maxpool_bwd_code_impl(dtype, B, Hi, Wi, C, code, dout, din, colsum, colsum_slab, colsum_slab_rows, colsum_rows_out, nullptr, 0, nullptr,
                                 nullptr, stream);
}

// dout given in ANOTHER coordinate system, [B][Hs][Ws][C], with the transposed band map to this pool's output as per-axis tables
// ytab[(Hi + 1) / 2][2], xtab[(Wi + 1) / 2][2] = {start, count} (device memory; what szn_band_remap takes): see PoolGather
extern "C" int szn_maxpool2x2_ceil_bwd_code_gather(int dtype, int B, int Hi, int Wi, int C, const void* code, const void* dsrc, int Hs, int Ws,
                                                   const int* ytab, const int* xtab, void* din, float* colsum, float* colsum_slab,
                                                   int colsum_slab_rows, int* colsum_rows_out, szn_stream_t stream) {
    if (!ytab || !xtab || Hs <= 0 || Ws <= 0) SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd_code_gather: tables and source size are required");
    if ((long)B * Hs * Ws * C >= (1L << 40)) SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd_code_gather: source too large");
    const PoolGather pg = {ytab, xtab, Hs, Ws};
    return maxpool_bwd_code_impl(dtype, B, Hi, Wi, C, code, dsrc, din, colsum, colsum_slab, colsum_slab_rows, colsum_rows_out, nullptr, 0, nullptr,
                                 nullptr, stream, &pg);
}

extern "C" int szn_maxpool2x2_ceil_bwd_code_cb(int dtype, int B, int Hi, int Wi, int C, const void* code, const void* dout, void* din,
                                               float* colsum, float* colsum_slab, int colsum_slab_rows, int* colsum_rows_out,
                                               const int* skip_regions, int n_regions, float* skip_sum, float* skip_slab, szn_stream_t stream) {
    if (!skip_regions) SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd_code_cb: skip_regions is NULL (use szn_maxpool2x2_ceil_bwd_code)");
    return maxpool_bwd_code_impl(dtype, B, Hi, Wi, C, code, dout, din, colsum, colsum_slab, colsum_slab_rows, colsum_rows_out, skip_regions, n_regions,
                                 skip_sum, skip_slab, stream);
}
