// szn_ema.hip -- averaged weights: the exponential moving average of the flat fp32 parameter buffers (Polyak averaging) and the exact
// in-place exchange that puts the average under validation.
//
// The reference has no counterpart (train.py / trainer_fcn.py validate and save the last iterate).
#include "szn_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;

// Both kernels are pure streaming passes over buffers larger than the last-level cache (12 B per element for the average, 16 B for the
// exchange), laid out like adam_kernel (szn_optim.hip): 16-B non-temporal accesses on the aligned body, two vectors of both streams
// loaded before either is used (four 16-B requests in flight per lane), a scalar path for what is left.  Unlike the optimizer entries
// they take any 4-byte-aligned pointer pair: `head` elements in front of the first 16-B boundary and the tail behind the last whole
// vector go through the scalar path, and a pair whose addresses differ modulo 16 goes through it entirely (head == n, n4 == 0).
// Grid: one pair of vectors per lane up to 2^17 blocks (2^28 elements: the 135 M-element weight buffer of FCN32s is one round, as the
// optimizer kernels launch theirs), the grid-stride loop beyond.  A grid capped at 2048 blocks (8 per CU, ~32 rounds per lane) measured
// a fifth slower on that buffer (tools/bench_ema.py --capped-lib); -DSZN_EMA_MAX_BLOCKS=2048 builds that variant.
#ifndef SZN_EMA_MAX_BLOCKS
#define SZN_EMA_MAX_BLOCKS (1 << 17)
#endif
constexpr int EMA_MAX_BLOCKS = SZN_EMA_MAX_BLOCKS;

// one element: param + D * (avg - param), the subtraction rounded once and the multiply-add once (an explicit fmaf: the library is
// built with -ffp-contract=off).  D == 0 hands back param itself, also where avg - param is not finite or param is -0.
__device__ __forceinline__ float ema_elem(float a, float p, float D) { return D == 0.f ? p : fmaf(D, a - p, p); }

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ avg, const float* __restrict__ param, long n, long head, long n4,
                                                  float decay, int every, int step, const float* __restrict__ dyn) {
    double s = (double)step - 1.0;                       // optimizer steps applied before this one
    if (dyn) {          // dynamic loss scaling: {scale S, found_inf, steps applied, ...}; see szn_adam_step_scaled
        if (dyn[1] != 0.f) return;                       // the optimizer kernels skipped this step: so does the average
        s = (double)dyn[2];
    }
    double d = (double)decay;
    if (step > 0) d = fmin(d, (1.0 + s) / (10.0 + s));   // warm-up ramp; step == 0 switches it off (with scale_state too)
    const float D = (float)pow(d, (double)every);
    if (D == 1.f) return;                                // avg stays as it is, bit for bit (the formula would round avg - param first)
    const long G = (long)gridDim.x * 256;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    f32x4_t* __restrict__ a4 = (f32x4_t*)(avg + head);
    const f32x4_t* __restrict__ p4 = (const f32x4_t*)(param + head);
    long i = t;
    for (; i + G < n4; i += 2 * G) {                     // two vectors of both streams per round: four requests before the first use
        const long j = i + G;
        f32x4_t a0 = __builtin_nontemporal_load(a4 + i), a1 = __builtin_nontemporal_load(a4 + j);
        const f32x4_t p0 = __builtin_nontemporal_load(p4 + i), p1 = __builtin_nontemporal_load(p4 + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) { a0[e] = ema_elem(a0[e], p0[e], D); a1[e] = ema_elem(a1[e], p1[e], D); }
        __builtin_nontemporal_store(a0, a4 + i);
        __builtin_nontemporal_store(a1, a4 + j);
    }
    if (i < n4) {                                        // a lane's odd last vector
        f32x4_t a0 = __builtin_nontemporal_load(a4 + i);
        const f32x4_t p0 = __builtin_nontemporal_load(p4 + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) a0[e] = ema_elem(a0[e], p0[e], D);
        __builtin_nontemporal_store(a0, a4 + i);
    }
    const long body_end = head + n4 * 4, rest = n - n4 * 4;     // scalar elements: [0, head) and [body_end, n)
    for (long r = t; r < rest; r += G) {
        const long k = r < head ? r : body_end + (r - head);
        avg[k] = ema_elem(avg[k], param[k], D);
    }
}

__global__ __launch_bounds__(256) void swap_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, long n, long head, long n4) {
    const long G = (long)gridDim.x * 256;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    u32x4_t* __restrict__ a4 = (u32x4_t*)(a + head);
    u32x4_t* __restrict__ b4 = (u32x4_t*)(b + head);
    long i = t;
    for (; i + G < n4; i += 2 * G) {                     // (as in ema_kernel; all four loads precede the first store)
        const long j = i + G;
        const u32x4_t x0 = __builtin_nontemporal_load(a4 + i), y0 = __builtin_nontemporal_load(b4 + i);
        const u32x4_t x1 = __builtin_nontemporal_load(a4 + j), y1 = __builtin_nontemporal_load(b4 + j);
        __builtin_nontemporal_store(y0, a4 + i); __builtin_nontemporal_store(x0, b4 + i);
        __builtin_nontemporal_store(y1, a4 + j); __builtin_nontemporal_store(x1, b4 + j);
    }
    if (i < n4) {
        const u32x4_t x0 = __builtin_nontemporal_load(a4 + i), y0 = __builtin_nontemporal_load(b4 + i);
        __builtin_nontemporal_store(y0, a4 + i); __builtin_nontemporal_store(x0, b4 + i);
    }
    const long body_end = head + n4 * 4, rest = n - n4 * 4;
    for (long r = t; r < rest; r += G) {
        const long k = r < head ? r : body_end + (r - head);
        const uint32_t x = a[k], y = b[k];
        a[k] = y; b[k] = x;
    }
}

}  // namespace

extern "C" int szn_ema_step(long n, float* avg, const float* param, float decay, int every, int step, const float* scale_state,
                            szn_stream_t stream) {
    if (n < 0 || every < 1 || step < 0) SZN_FAIL(SZN_ERR_ARG, "ema_step: n and step must be >= 0 and every >= 1");
    if (!(decay >= 0.f && decay <= 1.f)) SZN_FAIL(SZN_ERR_ARG, "ema_step: decay must lie in [0, 1]");
    if (n == 0) return SZN_OK;
    if (!avg || !param) SZN_FAIL(SZN_ERR_ARG, "ema_step: NULL buffer");
    if ((((uintptr_t)avg | (uintptr_t)param) & 3) != 0) SZN_FAIL(SZN_ERR_ARG, "ema_step: buffers must be 4-byte aligned");
    long head, n4;
    szn_split16(avg, param, n, &head, &n4);
    hipLaunchKernelGGL(ema_kernel, dim3(szn_stream_grid(n, n4, EMA_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, avg, param, n, head, n4, decay, every,
                       step, scale_state);
    SZN_CHECK_LAUNCH("ema_kernel");
    return SZN_OK;
}

extern "C" int szn_swap_f32(long n, float* a, float* b, szn_stream_t stream) {
    if (n < 0) SZN_FAIL(SZN_ERR_ARG, "swap_f32: n must be >= 0");
    if (n == 0) return SZN_OK;
    if (!a || !b) SZN_FAIL(SZN_ERR_ARG, "swap_f32: NULL buffer");
    if ((((uintptr_t)a | (uintptr_t)b) & 3) != 0) SZN_FAIL(SZN_ERR_ARG, "swap_f32: buffers must be 4-byte aligned");
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * 4;
    if (ua < ub + bytes && ub < ua + bytes) SZN_FAIL(SZN_ERR_ARG, "swap_f32: the buffers overlap");
    long head, n4;
    szn_split16(a, b, n, &head, &n4);
    hipLaunchKernelGGL(swap_kernel, dim3(szn_stream_grid(n, n4, EMA_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, (uint32_t*)a, (uint32_t*)b, n, head,
                       n4);
    SZN_CHECK_LAUNCH("swap_kernel");
    return SZN_OK;
}
