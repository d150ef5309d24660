// szn_augment.hip -- training augmentation on the device: per-image random scale, crop window and horizontal flip of a raw uint8 batch
// and its labels, written at a fixed crop size as the f32 BGR-minus-mean network input and the int64 target, by one kernel.
//
// Integer-exact (the contract is stated in include/szn.h).  One thread owns a run of 4 horizontally adjacent OUTPUT pixels of one
// image: the row terms (source rows, row weight, label row) are computed once per thread, the four columns gather their 2x2 source
// bytes through the cache, and the run leaves as one 16-byte store per colour plane and two for the label (v4 kernel, Wo % 4 == 0) or
// as scalar stores (any other Wo: rows are then not 16-byte aligned, and the last run of a row is partial).  blockIdx.y is the image,
// so its record is block-uniform and read once.
#include "szn_common.h"

namespace {

struct AugArgs {
    const uint8_t* rgb;
    const int64_t* label;
    const int32_t* params;
    float* out;
    int64_t* out_label;
    double mean[3];                          // BGR
    int Hm, Wm, Ho, Wo;
};

// one axis of the source position of grid coordinate g (already known to be inside the scaled image): bilinear taps i0, i1 with the
// 11-bit weight w of i1, and the nearest index l of the label
struct AugAxis {
    int i0, i1, w, l;
};

__device__ __forceinline__ AugAxis aug_axis(long g, int step, int n) {
    const long s = (((2 * g + 1) * (long)step) >> 1) - 32768;            // pixel centres, 16.16
    const long hi = (long)(n - 1) << 16;
    const long sc = s < 0 ? 0 : (s > hi ? hi : s);
    const long l = (s + 32768) >> 16;
    AugAxis a;
    a.i0 = (int)(sc >> 16);
    a.i1 = a.i0 + 1 < n ? a.i0 + 1 : n - 1;
    a.w = (int)(sc & 0xffff) >> 5;
    a.l = (int)(l < 0 ? 0 : (l > n - 1 ? n - 1 : l));
    return a;
}

template <bool V4>
__device__ __forceinline__ void augment_body(const AugArgs& a) {
    const int w4 = (a.Wo + 3) / 4;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)a.Ho * w4) return;
    const int yo = (int)(g / w4), x0 = (int)(g - (long)yo * w4) * 4;
    const int b = blockIdx.y;
    const int n = V4 ? 4 : (a.Wo - x0 < 4 ? a.Wo - x0 : 4);

    // the record; sizes that cannot be right are clamped so that no read leaves the canvas
    const int32_t* r = a.params + (long)b * SZN_AUG_NPARAM;
    const int h = r[0] < 1 ? 1 : (r[0] > a.Hm ? a.Hm : r[0]);
    const int w = r[1] < 1 ? 1 : (r[1] > a.Wm ? a.Wm : r[1]);
    const int Hs = r[2], Ws = r[3], step_y = r[4], step_x = r[5];
    const long oy = r[6], ox = r[7];
    const bool flip = r[8] != 0;

    const long gy = yo + oy;
    const bool row_in = gy >= 0 && gy < Hs;
    const AugAxis ay = aug_axis(row_in ? gy : 0, step_y, h);
    const long canvas = (long)a.Hm * a.Wm;
    const uint8_t* img = a.rgb + (long)b * canvas * 3;
    const uint8_t* row0 = img + (long)ay.i0 * a.Wm * 3;
    const uint8_t* row1 = img + (long)ay.i1 * a.Wm * 3;
    const int64_t* lrow = a.label + (long)b * canvas + (long)ay.l * a.Wm;

    float v[3][4];
    int64_t lab[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= n) continue;
        const int xo = x0 + j;
        const long gx = (flip ? a.Wo - 1 - xo : xo) + ox;
        if (!row_in || gx < 0 || gx >= Ws) {
            v[0][j] = v[1][j] = v[2][j] = 0.0f;
            lab[j] = SZN_PAD_LABEL;
            continue;
        }
        const AugAxis ax = aug_axis(gx, step_x, w);
        const uint8_t *p00 = row0 + ax.i0 * 3, *p01 = row0 + ax.i1 * 3, *p10 = row1 + ax.i0 * 3, *p11 = row1 + ax.i1 * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {                                    // output plane c reads source byte 2 - c (RGB -> BGR)
            const int top = (2048 - ax.w) * p00[2 - c] + ax.w * p01[2 - c];
            const int bot = (2048 - ax.w) * p10[2 - c] + ax.w * p11[2 - c];
            const int acc = (2048 - ay.w) * top + ay.w * bot;            // <= 255 * 2^22
            v[c][j] = (float)((double)acc / 4194304.0 - a.mean[c]);
        }
        lab[j] = lrow[ax.l];
    }

    const long plane = (long)a.Ho * a.Wo, at = (long)yo * a.Wo + x0;
    float* o = a.out + (long)b * 3 * plane + at;
    int64_t* ol = a.out_label + (long)b * plane + at;
    if (V4) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *(f32x4_t*)(o + c * plane) = f32x4_t{v[c][0], v[c][1], v[c][2], v[c][3]};
        typedef __attribute__((ext_vector_type(2))) long i64x2_t;
        *(i64x2_t*)ol = i64x2_t{(long)lab[0], (long)lab[1]};
        *(i64x2_t*)(ol + 2) = i64x2_t{(long)lab[2], (long)lab[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                o[j] = v[0][j];
                o[plane + j] = v[1][j];
                o[2 * plane + j] = v[2][j];
                ol[j] = lab[j];
            }
    }
}

__global__ __launch_bounds__(256) void augment_u8_kernel(const AugArgs a) { augment_body<false>(a); }
__global__ __launch_bounds__(256) void augment_u8_kernel_v4(const AugArgs a) { augment_body<true>(a); }

}  // namespace

extern "C" int szn_augment_u8(int B, int Hm, int Wm, const uint8_t* rgb_hwc, const int64_t* label, const int32_t* params,
                              const double* mean_bgr, int Ho, int Wo, float* out_nchw, int64_t* out_label, szn_stream_t stream) {
    if (!rgb_hwc || !label || !params || !mean_bgr || !out_nchw || !out_label)
        SZN_FAIL(SZN_ERR_ARG, "augment_u8: rgb_hwc, label, params, mean_bgr, out_nchw and out_label are required");
    if (B <= 0 || Hm <= 0 || Wm <= 0 || Ho <= 0 || Wo <= 0)
        SZN_FAIL(SZN_ERR_ARG, "augment_u8: empty batch, canvas or crop (B %d, canvas %d x %d, crop %d x %d)", B, Hm, Wm, Ho, Wo);
    if (B > 65535) SZN_FAIL(SZN_ERR_ARG, "augment_u8: B %d above 65535 (one grid row per image)", B);
    if ((long)Hm * Wm * 3 > 0x7fffffffL) SZN_FAIL(SZN_ERR_ARG, "augment_u8: canvas %d x %d too large", Hm, Wm);
    const long groups = (long)Ho * ((Wo + 3) / 4);
    if ((groups + 255) / 256 > 0x7fffffffL) SZN_FAIL(SZN_ERR_ARG, "augment_u8: crop %d x %d too large", Ho, Wo);
    AugArgs a{};
    a.rgb = rgb_hwc; a.label = label; a.params = params; a.out = out_nchw; a.out_label = out_label;
    for (int c = 0; c < 3; ++c) a.mean[c] = mean_bgr[c];
    a.Hm = Hm; a.Wm = Wm; a.Ho = Ho; a.Wo = Wo;
    const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)B);
    // every run of a thread is then 16 bytes at a multiple of 16 in each plane, and 32 in the label
    const bool v4 = Wo % 4 == 0 && ((uintptr_t)out_nchw & 15) == 0 && ((uintptr_t)out_label & 15) == 0;
    if (v4) {
        hipLaunchKernelGGL(augment_u8_kernel_v4, grid, dim3(256), 0, (hipStream_t)stream, a);
        SZN_CHECK_LAUNCH("augment_u8_kernel_v4");
    } else {
        hipLaunchKernelGGL(augment_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
        SZN_CHECK_LAUNCH("augment_u8_kernel");
    }
    return SZN_OK;
}

// ---- szn_augment_affine_u8: rotation and colour jitter.  The same thread geometry (4 adjacent output pixels of a row, blockIdx.y the
// image), but the position map is a 2 x 3 affine one, so nothing is shared along a row: every pixel computes its own two source positions
// and gathers its 2 x 2 x 3 bytes through the cache.  The three interpolated channels then go through a 3 x 4 fixed-point colour matrix.
// Integer arithmetic only up to the final double subtraction (contract in include/szn.h).
namespace {

// a*b and a+b modulo 2^64: the contract's int64 arithmetic never overflows for a record the host builds; a garbage record or an output
// side beyond 2^29 wraps instead of being undefined, and every index derived from the result is range-checked before use
__device__ __forceinline__ long auga_mad(long a, long b, long c) { return (long)((unsigned long)a * (unsigned long)b + (unsigned long)c); }

template <bool V4>
__device__ __forceinline__ void augment_affine_body(const AugArgs& a) {
    const int w4 = (a.Wo + 3) / 4;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)a.Ho * w4) return;
    const int yo = (int)(g / w4), x0 = (int)(g - (long)yo * w4) * 4;
    const int b = blockIdx.y;
    const int n = V4 ? 4 : (a.Wo - x0 < 4 ? a.Wo - x0 : 4);

    // the record; sizes that cannot be right are clamped so that no read leaves the canvas, matrix words so that no sum overflows
    const int32_t* r = a.params + (long)b * SZN_AUGA_NPARAM;
    const int h = r[0] < 1 ? 1 : (r[0] > a.Hm ? a.Hm : r[0]);
    const int w = r[1] < 1 ? 1 : (r[1] > a.Wm ? a.Wm : r[1]);
    const long mxx = r[2], mxy = r[3], tx = r[4], myx = r[5], myy = r[6], ty = r[7];
    long cm[9], co[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) cm[i] = r[8 + i] < -1048576 ? -1048576 : (r[8 + i] > 1048576 ? 1048576 : r[8 + i]);
#pragma unroll
    for (int c = 0; c < 3; ++c) co[c] = (long)((unsigned long)(long)r[17 + c] << 22);

    const long Y = 2L * yo + 1;
    const long row_x = auga_mad(mxy, Y, 0), row_y = auga_mad(myy, Y, 0);
    const long hi_x = (long)(w - 1) << 16, hi_y = (long)(h - 1) << 16;
    const long canvas = (long)a.Hm * a.Wm;
    const uint8_t* img = a.rgb + (long)b * canvas * 3;
    const int64_t* limg = a.label + (long)b * canvas;

    float v[3][4];
    int64_t lab[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= n) continue;
        const long X = 2L * (x0 + j) + 1;
        const long sx = (auga_mad(mxx, X, row_x) >> 1) + tx - 32768;
        const long sy = (auga_mad(myx, X, row_y) >> 1) + ty - 32768;
        const long lx = (sx + 32768) >> 16, ly = (sy + 32768) >> 16;
        // no branch on the padding decision: a padding pixel gathers at the clamped position (inside the image, so inside the canvas) and
        // its results are replaced by selects at the end.  Every lane runs the same straight-line code.
        const bool inside = (lx >= 0) & (lx < w) & (ly >= 0) & (ly < h);
        const long lxc = lx < 0 ? 0 : (lx > w - 1 ? w - 1 : lx), lyc = ly < 0 ? 0 : (ly > h - 1 ? h - 1 : ly);
        const long cx = sx < 0 ? 0 : (sx > hi_x ? hi_x : sx), cy = sy < 0 ? 0 : (sy > hi_y ? hi_y : sy);
        const int ix0 = (int)(cx >> 16), iy0 = (int)(cy >> 16);
        const int ix1 = ix0 + 1 < w ? ix0 + 1 : w - 1, iy1 = iy0 + 1 < h ? iy0 + 1 : h - 1;
        const int wx = (int)(cx & 0xffff) >> 5, wy = (int)(cy & 0xffff) >> 5;
        const uint8_t *row0 = img + (long)iy0 * a.Wm * 3, *row1 = img + (long)iy1 * a.Wm * 3;
        const uint8_t *p00 = row0 + ix0 * 3, *p01 = row0 + ix1 * 3, *p10 = row1 + ix0 * 3, *p11 = row1 + ix1 * 3;
        long acc[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {                                    // source byte d, RGB order
            const int top = (2048 - wx) * p00[d] + wx * p01[d];
            const int bot = (2048 - wx) * p10[d] + wx * p11[d];
            acc[d] = (2048 - wy) * top + wy * bot;                       // <= 255 * 2^22
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {                                    // colour channel c (RGB) leaves in plane 2 - c (BGR)
            long u = cm[3 * c] * acc[0] + cm[3 * c + 1] * acc[1] + cm[3 * c + 2] * acc[2] + co[c];   // |.| <= 3 * 2^50 + 2^53
            const long top = 255L << 38;
            u = u < 0 ? 0 : (u > top ? top : u);                         // < 2^46: the conversion and the division are exact
            const float f = (float)((double)u / 274877906944.0 - a.mean[2 - c]);
            v[2 - c][j] = inside ? f : 0.0f;
        }
        const int64_t l = limg[lyc * a.Wm + lxc];
        lab[j] = inside ? l : (int64_t)SZN_PAD_LABEL;
    }

    const long plane = (long)a.Ho * a.Wo, at = (long)yo * a.Wo + x0;
    float* o = a.out + (long)b * 3 * plane + at;
    int64_t* ol = a.out_label + (long)b * plane + at;
    if (V4) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *(f32x4_t*)(o + c * plane) = f32x4_t{v[c][0], v[c][1], v[c][2], v[c][3]};
        typedef __attribute__((ext_vector_type(2))) long i64x2_t;
        *(i64x2_t*)ol = i64x2_t{(long)lab[0], (long)lab[1]};
        *(i64x2_t*)(ol + 2) = i64x2_t{(long)lab[2], (long)lab[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                o[j] = v[0][j];
                o[plane + j] = v[1][j];
                o[2 * plane + j] = v[2][j];
                ol[j] = lab[j];
            }
    }
}

__global__ __launch_bounds__(256) void augment_affine_u8_kernel(const AugArgs a) { augment_affine_body<false>(a); }
__global__ __launch_bounds__(256) void augment_affine_u8_kernel_v4(const AugArgs a) { augment_affine_body<true>(a); }

}  // namespace

extern "C" int szn_augment_affine_u8(int B, int Hm, int Wm, const uint8_t* rgb_hwc, const int64_t* label, const int32_t* params,
                                     const double* mean_bgr, int Ho, int Wo, float* out_nchw, int64_t* out_label, szn_stream_t stream) {
    if (!rgb_hwc || !label || !params || !mean_bgr || !out_nchw || !out_label)
        SZN_FAIL(SZN_ERR_ARG, "augment_affine_u8: rgb_hwc, label, params, mean_bgr, out_nchw and out_label are required");
    if (B <= 0 || Hm <= 0 || Wm <= 0 || Ho <= 0 || Wo <= 0)
        SZN_FAIL(SZN_ERR_ARG, "augment_affine_u8: empty batch, canvas or crop (B %d, canvas %d x %d, crop %d x %d)", B, Hm, Wm, Ho, Wo);
    if (B > 65535) SZN_FAIL(SZN_ERR_ARG, "augment_affine_u8: B %d above 65535 (one grid row per image)", B);
    if ((long)Hm * Wm * 3 > 0x7fffffffL) SZN_FAIL(SZN_ERR_ARG, "augment_affine_u8: canvas %d x %d too large", Hm, Wm);
    const long groups = (long)Ho * ((Wo + 3) / 4);
    if ((groups + 255) / 256 > 0x7fffffffL) SZN_FAIL(SZN_ERR_ARG, "augment_affine_u8: crop %d x %d too large", Ho, Wo);
    AugArgs a{};
    a.rgb = rgb_hwc; a.label = label; a.params = params; a.out = out_nchw; a.out_label = out_label;
    for (int c = 0; c < 3; ++c) a.mean[c] = mean_bgr[c];
    a.Hm = Hm; a.Wm = Wm; a.Ho = Ho; a.Wo = Wo;
    const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)B);
    const bool v4 = Wo % 4 == 0 && ((uintptr_t)out_nchw & 15) == 0 && ((uintptr_t)out_label & 15) == 0;
    if (v4) {
        hipLaunchKernelGGL(augment_affine_u8_kernel_v4, grid, dim3(256), 0, (hipStream_t)stream, a);
        SZN_CHECK_LAUNCH("augment_affine_u8_kernel_v4");
    } else {
        hipLaunchKernelGGL(augment_affine_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
        SZN_CHECK_LAUNCH("augment_affine_u8_kernel");
    }
    return SZN_OK;
}
