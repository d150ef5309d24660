// szn_elementwise.hip -- true element-wise / streaming kernels: casts, Dropout2d factors, the u8 RGB -> mean-subtracted BGR fp32 image,
// the fixed-order reduction of column-sum partial rows.
//
// Reference sites: models.py:86,91 (Dropout2d).
#include "szn_common.h"
#include <algorithm>

namespace {

template <typename S, typename D>
__global__ void cast_kernel(const S* __restrict__ s, D* __restrict__ d, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        elem<D>::st(d + i, elem<S>::ld(s + i));
}

// (splitmix64: szn_common.h -- shared with the visualisation kernel's noise)
__global__ void dropout_mask_kernel(float* __restrict__ scale, long n, float p, uint64_t seed, uint64_t offset) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t h = splitmix64(seed * 0xD1342543DE82EF95ull + offset + (uint64_t)i);
    const float u = (float)(h >> 40) * (1.0f / 16777216.0f);   // 24-bit uniform in [0,1)
    scale[i] = (u >= p) ? 1.0f / (1.0f - p) : 0.f;
}

}  // namespace

extern "C" int szn_cast(int src_dtype, int dst_dtype, long n, const void* src, void* dst, szn_stream_t stream) {
    if (!src || !dst || n < 0) SZN_FAIL(SZN_ERR_ARG, "cast: bad argument");
    if (n == 0) return SZN_OK;
    hipStream_t st = (hipStream_t)stream;
    const int grid = szn_grid_for(n);
    if (src_dtype == SZN_F32 && dst_dtype == SZN_BF16)
        hipLaunchKernelGGL((cast_kernel<float, bf16_raw>), dim3(grid), dim3(256), 0, st, (const float*)src, (bf16_raw*)dst, n);
    else if (src_dtype == SZN_BF16 && dst_dtype == SZN_F32)
        hipLaunchKernelGGL((cast_kernel<bf16_raw, float>), dim3(grid), dim3(256), 0, st, (const bf16_raw*)src, (float*)dst, n);
    else if (src_dtype == SZN_F32 && dst_dtype == SZN_F16)
        hipLaunchKernelGGL((cast_kernel<float, f16_raw>), dim3(grid), dim3(256), 0, st, (const float*)src, (f16_raw*)dst, n);
    else if (src_dtype == SZN_F16 && dst_dtype == SZN_F32)
        hipLaunchKernelGGL((cast_kernel<f16_raw, float>), dim3(grid), dim3(256), 0, st, (const f16_raw*)src, (float*)dst, n);
    else if (src_dtype == SZN_F32 && dst_dtype == SZN_F32)
        hipLaunchKernelGGL((cast_kernel<float, float>), dim3(grid), dim3(256), 0, st, (const float*)src, (float*)dst, n);
    else
        SZN_FAIL(SZN_ERR_ARG, "cast: unsupported dtype pair %d -> %d", src_dtype, dst_dtype);
    SZN_CHECK_LAUNCH("cast_kernel");
    return SZN_OK;
}

extern "C" int szn_dropout2d_mask(long n, float p, uint64_t seed, uint64_t offset, float* scale, szn_stream_t stream) {
    if (!scale || n <= 0 || p < 0.f || p >= 1.f) SZN_FAIL(SZN_ERR_ARG, "dropout2d_mask: bad argument");
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scale, n, p,
                       seed, offset);
    SZN_CHECK_LAUNCH("dropout_mask_kernel");
    return SZN_OK;
}

namespace {
// one thread per pixel: 3 byte loads (one 3-byte RGB triple), three coalesced f32 plane stores
__global__ __launch_bounds__(256) void image_u8_to_bgr_kernel(const uint8_t* __restrict__ rgb, float* __restrict__ out, long npx,
                                                              long hw, double m0, double m1, double m2) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npx) return;
    const long b = i / hw, r = i - b * hw;
    const uint8_t* p = rgb + i * 3;
    float* o = out + b * 3 * hw + r;
    o[0] = (float)((double)p[2] - m0);          // B
    o[hw] = (float)((double)p[1] - m1);         // G
    o[2 * hw] = (float)((double)p[0] - m2);     // R
}
}  // namespace

extern "C" int szn_image_u8_to_bgr_f32(int B, int H, int W, const uint8_t* rgb_hwc, const double* mean_bgr, float* out_nchw,
                                       szn_stream_t stream) {
    if (!rgb_hwc || !mean_bgr || !out_nchw || B <= 0 || H <= 0 || W <= 0) SZN_FAIL(SZN_ERR_ARG, "image_u8_to_bgr_f32: bad argument");
    const long hw = (long)H * W, npx = (long)B * hw;
    hipLaunchKernelGGL(image_u8_to_bgr_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rgb_hwc,
                       out_nchw, npx, hw, mean_bgr[0], mean_bgr[1], mean_bgr[2]);
    SZN_CHECK_LAUNCH("image_u8_to_bgr_kernel");
    return SZN_OK;
}

// ---- fixed-order reduction of the column-sum partial rows (bias gradients) ------------------------------------------------------
// job j: out[c] += sum_{r < rows} slab[r][c], c < C.  One block = 64 channels of one job (16 float4 columns x 64 row groups): each
// thread adds every 64th row (independent 16-B loads), the 64 groups are combined in ascending order.  (16 row groups per block left
// a 64-channel layer's 2,000 rows to 128 dependent steps per thread: 32 us for the whole launch; 1024 threads: a third of that.)
struct ColsumJobs { const float* slab[32]; float* out[32]; int rows[32]; int C[32]; int first_block[33]; };

constexpr int kCsGroups = 64;

__global__ __launch_bounds__(1024) void colsum_reduce_kernel(ColsumJobs jb, int njobs) {
    __shared__ f32x4_t part[kCsGroups][16];
    int j = 0;
    while (j + 1 < njobs && (int)blockIdx.x >= jb.first_block[j + 1]) ++j;
    const int c0 = ((int)blockIdx.x - jb.first_block[j]) * 64;
    const int C = jb.C[j], rows = jb.rows[j];
    const float* slab = jb.slab[j];
    const int q = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = c0 + q * 4;
    f32x4_t a = {0.f, 0.f, 0.f, 0.f};
    if (c < C) {
        if ((C & 3) == 0) {
            for (int r = rg; r < rows; r += kCsGroups) a += *(const f32x4_t*)(slab + (long)r * C + c);
        } else {
            for (int r = rg; r < rows; r += kCsGroups)
#pragma unroll
                for (int e = 0; e < 4; ++e) if (c + e < C) a[e] += slab[(long)r * C + c + e];
        }
    }
    part[rg][q] = a;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int cc = c0 + threadIdx.x;
        if (cc < C) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < kCsGroups; ++g) s += part[g][threadIdx.x >> 2][threadIdx.x & 3];
            jb.out[j][cc] += s;
        }
    }
}

extern "C" int szn_colsum_reduce_batch(int n, const float* const* slabs, const int* rows, const int* C, float* const* out,
                                       szn_stream_t stream) {
    if (n < 0 || (n > 0 && (!slabs || !rows || !C || !out))) SZN_FAIL(SZN_ERR_ARG, "colsum_reduce_batch: bad argument");
    for (int base = 0; base < n; base += 32) {
        ColsumJobs jb;
        const int m = std::min(32, n - base);
        int blocks = 0;
        for (int j = 0; j < m; ++j) {
            if (!slabs[base + j] || !out[base + j] || rows[base + j] < 0 || C[base + j] <= 0 || ((uintptr_t)slabs[base + j] & 15))
                SZN_FAIL(SZN_ERR_ARG, "colsum_reduce_batch: bad job %d", base + j);
            jb.slab[j] = slabs[base + j]; jb.out[j] = out[base + j]; jb.rows[j] = rows[base + j]; jb.C[j] = C[base + j];
            jb.first_block[j] = blocks;
            blocks += (C[base + j] + 63) / 64;
        }
        jb.first_block[m] = blocks;
        if (blocks == 0) continue;
        hipLaunchKernelGGL(colsum_reduce_kernel, dim3(blocks), dim3(1024), 0, (hipStream_t)stream, jb, m);
        SZN_CHECK_LAUNCH("colsum_reduce_kernel");
    }
    return SZN_OK;
}
