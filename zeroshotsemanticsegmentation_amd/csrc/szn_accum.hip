// szn_accum.hip -- gradient accumulation: the running fp32 sum of the step's flat gradient buffers over a window of micro-steps.
//
// The reference has no counterpart (trainer_fcn.py calls optim.step() after every backward()); the semantics are torch's: A backward()
// calls without zero_grad() leave ((g1 + g2) + g3) + ... + gA in .grad.
#include "szn_common.h"

namespace {

// One IEEE addition per element and nothing else (the library is built with -ffp-contract=off, and there is nothing to contract).
// A pure streaming pass laid out like ema_kernel (szn_ema.hip): 16-B non-temporal accesses on the aligned body, two vectors of both
// streams loaded before either is used, one pair of vectors per lane up to 2^17 blocks with the grid-stride loop beyond, a scalar
// path for the head in front of the first 16-B boundary and for the tail; a pointer pair whose addresses differ modulo 16 goes
// through the scalar path entirely (szn_split16).  MODE is uniform per launch, hence a template parameter:
//   SET    acc = grad           reads grad,       writes acc    ( 8 B / element)
//   ADD    acc = acc + grad     reads both,       writes acc    (12 B / element)
//   FINAL  grad = acc + grad    reads both,       writes grad   (12 B / element)
// No atomics, no reduction: every element has one owner, two calls give the same bits.
constexpr int ACCUM_MAX_BLOCKS = 1 << 17;

template <int MODE>
__global__ __launch_bounds__(256) void grad_accum_kernel(float* __restrict__ acc, float* __restrict__ grad, long n, long head, long n4) {
    const long G = (long)gridDim.x * 256;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    f32x4_t* __restrict__ a4 = (f32x4_t*)(acc + head);
    f32x4_t* __restrict__ g4 = (f32x4_t*)(grad + head);
    f32x4_t* __restrict__ o4 = MODE == SZN_ACCUM_FINAL ? g4 : a4;
    long i = t;
    for (; i + G < n4; i += 2 * G) {                     // two vectors of both streams per round: four requests before the first use
        const long j = i + G;
        f32x4_t s0 = __builtin_nontemporal_load(g4 + i), s1 = __builtin_nontemporal_load(g4 + j);
        if (MODE != SZN_ACCUM_SET) {
            const f32x4_t a0 = __builtin_nontemporal_load(a4 + i), a1 = __builtin_nontemporal_load(a4 + j);
            s0 = a0 + s0;
            s1 = a1 + s1;
        }
        __builtin_nontemporal_store(s0, o4 + i);
        __builtin_nontemporal_store(s1, o4 + j);
    }
    if (i < n4) {                                        // a lane's odd last vector
        f32x4_t s0 = __builtin_nontemporal_load(g4 + i);
        if (MODE != SZN_ACCUM_SET) s0 = __builtin_nontemporal_load(a4 + i) + s0;
        __builtin_nontemporal_store(s0, o4 + i);
    }
    const long body_end = head + n4 * 4, rest = n - n4 * 4;     // scalar elements: [0, head) and [body_end, n)
    float* __restrict__ out = MODE == SZN_ACCUM_FINAL ? grad : acc;
    for (long r = t; r < rest; r += G) {
        const long k = r < head ? r : body_end + (r - head);
        out[k] = MODE == SZN_ACCUM_SET ? grad[k] : acc[k] + grad[k];
    }
}

template <int MODE> void launch(float* acc, float* grad, long n, long head, long n4, hipStream_t stream) {
    hipLaunchKernelGGL(grad_accum_kernel<MODE>, dim3(szn_stream_grid(n, n4, ACCUM_MAX_BLOCKS)), dim3(256), 0, stream, acc, grad, n,
                       head, n4);
}

}  // namespace

extern "C" int szn_grad_accum(long n, float* acc, float* grad, int mode, szn_stream_t stream) {
    if (n < 0) SZN_FAIL(SZN_ERR_ARG, "grad_accum: n must be >= 0");
    if (mode != SZN_ACCUM_SET && mode != SZN_ACCUM_ADD && mode != SZN_ACCUM_FINAL)
        SZN_FAIL(SZN_ERR_ARG, "grad_accum: mode must be SZN_ACCUM_SET, _ADD or _FINAL");
    if (n == 0) return SZN_OK;
    if (!acc || !grad) SZN_FAIL(SZN_ERR_ARG, "grad_accum: NULL buffer");
    if ((((uintptr_t)acc | (uintptr_t)grad) & 3) != 0) SZN_FAIL(SZN_ERR_ARG, "grad_accum: buffers must be 4-byte aligned");
    const uintptr_t ua = (uintptr_t)acc, ug = (uintptr_t)grad, bytes = (uintptr_t)n * 4;
    if (ua < ug + bytes && ug < ua + bytes) SZN_FAIL(SZN_ERR_ARG, "grad_accum: the buffers overlap");
    long head, n4;
    szn_split16(acc, grad, n, &head, &n4);
    if (mode == SZN_ACCUM_SET) launch<SZN_ACCUM_SET>(acc, grad, n, head, n4, (hipStream_t)stream);
    else if (mode == SZN_ACCUM_ADD) launch<SZN_ACCUM_ADD>(acc, grad, n, head, n4, (hipStream_t)stream);
    else launch<SZN_ACCUM_FINAL>(acc, grad, n, head, n4, (hipStream_t)stream);
    SZN_CHECK_LAUNCH("grad_accum_kernel");
    return SZN_OK;
}
