// szn_optim.hip -- Adam / SGD-momentum steps over the flat fp32 parameter buffers, and dynamic loss scaling (fp16 path).
//
// Reference sites: train.py:126-133,174-175 (torch.optim.SGD / Adam with two parameter groups).
#include "szn_common.h"

namespace {

// Optimizer steps over the flat fp32 parameter / gradient / moment buffers: pure streaming (28-30 B per element), so each
// lane moves 16 B per access (four elements) and keeps two such groups in flight; the per-element arithmetic is the
// scalar chain of torch.optim (no contraction: -ffp-contract=off), identical for the vector body and the scalar tail.
// (adam_elem: szn_common.h -- shared with the weight-gradient kernel that applies the update in its epilogue)

// Master, gradient and moments are loaded and stored non-temporally: 4 GB per step that nobody reads again before the next optimizer pass
// stays out of the caches' way (with the default policy the NEXT step's first kernels pay for it -- the whole step 0.05 ms slower with
// fc6's update fused, 0.21 ms with the separate pass: profiles/r04_ablations.txt 18).

// the gradient as the optimizer kernels read it: fp32, or a 16-bit image (szn_*_step_g16: the summed wire buffer of the exchange)
template <typename G> struct grad_src {
    __device__ static __forceinline__ f32x4_t ld4(const void* g, long i) {
        return __builtin_nontemporal_load((const f32x4_t*)g + i);
    }
    __device__ static __forceinline__ float ld1(const void* g, long i) { return ((const float*)g)[i]; }
};
template <typename G> __device__ __forceinline__ f32x4_t grad16_ld4(const void* g, long i) {
    typedef __attribute__((ext_vector_type(2))) uint32_t g_u32x2_t;
    const g_u32x2_t r = __builtin_nontemporal_load((const g_u32x2_t*)g + i);
    return f32x4_t{from_bits16<G>((uint16_t)(r[0] & 0xffffu)), from_bits16<G>((uint16_t)(r[0] >> 16)),
                   from_bits16<G>((uint16_t)(r[1] & 0xffffu)), from_bits16<G>((uint16_t)(r[1] >> 16))};
}
template <> struct grad_src<bf16_raw> {
    __device__ static __forceinline__ f32x4_t ld4(const void* g, long i) { return grad16_ld4<bf16_raw>(g, i); }
    __device__ static __forceinline__ float ld1(const void* g, long i) { return bf16_bits_to_f32(((const uint16_t*)g)[i]); }
};
template <> struct grad_src<f16_raw> {
    __device__ static __forceinline__ f32x4_t ld4(const void* g, long i) { return grad16_ld4<f16_raw>(g, i); }
    __device__ static __forceinline__ float ld1(const void* g, long i) { return f16_bits_to_f32(((const uint16_t*)g)[i]); }
};

template <typename LP, typename G = float>      // LP: element type of the optional 16-bit weight image (bf16_raw | f16_raw); G: the gradient's
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const void* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                   float b1, float b2, float eps, float wd, float step_size,
                                                   float inv_bc2_sqrt, float gscale, uint16_t* __restrict__ wlp, int vec,
                                                   const float* __restrict__ dyn, const float* __restrict__ clip) {
    if (dyn) {          // dynamic loss scaling: {scale S, found_inf, steps applied, ...}; see szn_adam_step_scaled
        if (dyn[1] != 0.f) return;                       // a non-finite gradient somewhere: the whole step is skipped
        gscale = gscale / dyn[0];
        const double step = (double)dyn[2] + 1.0;
        step_size = (float)((double)lr / (1.0 - pow((double)b1, step)));
        inv_bc2_sqrt = (float)(1.0 / sqrt(1.0 - pow((double)b2, step)));
    }
    if (clip) gscale = gscale * clip[0];                 // szn_*_step_clipped: the step's clipping coefficient (szn_clip_coef), one fp32 multiply
    const long n4 = vec ? (n >> 2) : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4_t gq = grad_src<G>::ld4(g, i);
        f32x4_t pq = __builtin_nontemporal_load((const f32x4_t*)p + i),
                mq = __builtin_nontemporal_load((const f32x4_t*)m + i), vq = __builtin_nontemporal_load((const f32x4_t*)v + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pq[e], me = mq[e], ve = vq[e];
            adam_elem(pe, gq[e], me, ve, b1, b2, eps, wd, step_size, inv_bc2_sqrt, gscale);
            pq[e] = pe; mq[e] = me; vq[e] = ve;
        }
        __builtin_nontemporal_store(mq, (f32x4_t*)m + i); __builtin_nontemporal_store(vq, (f32x4_t*)v + i);
        __builtin_nontemporal_store(pq, (f32x4_t*)p + i);
        if (wlp) {
            uint2 pk;
            pk.x = pack2<LP>(pq[0], pq[1]);
            pk.y = pack2<LP>(pq[2], pq[3]);
            ((uint2*)wlp)[i] = pk;
        }
    }
    for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float pi = p[i], mi = m[i], vi = v[i];
        adam_elem(pi, grad_src<G>::ld1(g, i), mi, vi, b1, b2, eps, wd, step_size, inv_bc2_sqrt, gscale);
        m[i] = mi; v[i] = vi; p[i] = pi;
        if (wlp) wlp[i] = to_bits16<LP>(pi);
    }
}

__device__ __forceinline__ void sgd_elem(float& pi, float gi, float& bi, float lr, float mom, float wd, int first, float gscale) {
    gi = gi * gscale;
    if (wd != 0.f) gi = fmaf(wd, pi, gi);
    bi = first ? gi : mom * bi + gi;
    pi -= lr * bi;
}

template <typename LP, typename G = float>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const void* __restrict__ g,
                                                  float* __restrict__ buf, long n, float lr, float mom, float wd,
                                                  int first, float gscale, uint16_t* __restrict__ wlp, int vec,
                                                  const float* __restrict__ dyn, const float* __restrict__ clip) {
    if (dyn) {
        if (dyn[1] != 0.f) return;
        gscale = gscale / dyn[0];
        first = dyn[2] == 0.f;
    }
    if (clip) gscale = gscale * clip[0];
    const long n4 = vec ? (n >> 2) : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4_t gq = grad_src<G>::ld4(g, i);
        f32x4_t pq = __builtin_nontemporal_load((const f32x4_t*)p + i);
        f32x4_t bq = first ? f32x4_t{0.f, 0.f, 0.f, 0.f} : __builtin_nontemporal_load((const f32x4_t*)buf + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pq[e], be = bq[e];
            sgd_elem(pe, gq[e], be, lr, mom, wd, first, gscale);
            pq[e] = pe; bq[e] = be;
        }
        __builtin_nontemporal_store(bq, (f32x4_t*)buf + i); __builtin_nontemporal_store(pq, (f32x4_t*)p + i);
        if (wlp) {
            uint2 pk;
            pk.x = pack2<LP>(pq[0], pq[1]);
            pk.y = pack2<LP>(pq[2], pq[3]);
            ((uint2*)wlp)[i] = pk;
        }
    }
    for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float pi = p[i], bi = first ? 0.f : buf[i];
        sgd_elem(pi, grad_src<G>::ld1(g, i), bi, lr, mom, wd, first, gscale);
        buf[i] = bi; p[i] = pi;
        if (wlp) wlp[i] = to_bits16<LP>(pi);
    }
}

}  // namespace

static int adam_impl(long n, float* param, const void* grad, int grad_dtype, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int step, float grad_scale, void* w_lp, int w_lp_dtype,
                     const float* dyn, szn_stream_t stream, const float* clip = nullptr) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step < 1) SZN_FAIL(SZN_ERR_ARG, "adam_step: bad argument");
    if (w_lp && !szn_is16(w_lp_dtype)) SZN_FAIL(SZN_ERR_ARG, "adam_step: the weight image must be SZN_BF16 or SZN_F16");
    if (grad_dtype != SZN_F32 && !szn_is16(grad_dtype)) SZN_FAIL(SZN_ERR_ARG, "adam_step: the gradient must be SZN_F32, SZN_BF16 or SZN_F16");
    float step_size, inv_bc2_sqrt;
    szn_adam_scalars(lr, beta1, beta2, step, &step_size, &inv_bc2_sqrt);
    const uintptr_t galign = grad_dtype == SZN_F32 ? 15 : 7;
    const int vec = ((((uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0 && ((uintptr_t)grad & galign) == 0 &&
                     (((uintptr_t)w_lp) & 7) == 0) ? 1 : 0;
    // one 16-B group per thread, no grid-stride loop: measured 6.1 TB/s on the 135 M-element buffer vs 5.6 with 16 Ki blocks
    const dim3 grid(szn_grid_for(vec ? (n + 3) / 4 : n, 256, 1 << 24));
    const bool lp_f16 = w_lp && w_lp_dtype == SZN_F16;    // (grad_dtype was checked above)
    szn_by_dtype(grad_dtype, [&](auto gtag) {
        using G = decltype(gtag);
        const auto kernel = lp_f16 ? adam_kernel<f16_raw, G> : adam_kernel<bf16_raw, G>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps,
                           weight_decay, step_size, inv_bc2_sqrt, grad_scale, (uint16_t*)w_lp, vec, dyn, clip);
    });
    SZN_CHECK_LAUNCH(grad_dtype == SZN_F32 ? "adam_kernel" : "adam_kernel_g16");
    return SZN_OK;
}

extern "C" int szn_adam_step(long n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                             float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                             void* w_lp, int w_lp_dtype, szn_stream_t stream) {
    return adam_impl(n, param, grad, SZN_F32, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale, w_lp, w_lp_dtype,
                     nullptr, stream);
}

extern "C" int szn_adam_step_g16(long n, float* param, const void* grad, int grad_dtype, float* exp_avg, float* exp_avg_sq, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                 void* w_lp, int w_lp_dtype, szn_stream_t stream) {
    if (!szn_is16(grad_dtype)) SZN_FAIL(SZN_ERR_ARG, "adam_step_g16: the gradient image must be SZN_BF16 or SZN_F16");
    return adam_impl(n, param, grad, grad_dtype, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale, w_lp,
                     w_lp_dtype, nullptr, stream);
}

extern "C" int szn_adam_step_scaled(long n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, const float* scale_state,
                                    float grad_scale, void* w_lp, int w_lp_dtype, szn_stream_t stream) {
    if (!scale_state) SZN_FAIL(SZN_ERR_ARG, "adam_step_scaled: scale_state is NULL");
    return adam_impl(n, param, grad, SZN_F32, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, 1, grad_scale, w_lp, w_lp_dtype,
                     scale_state, stream);
}

static int sgd_impl(long n, float* param, const void* grad, int grad_dtype, float* momentum_buf, float lr, float momentum,
                    float weight_decay, int first_step, float grad_scale, void* w_lp, int w_lp_dtype, const float* dyn,
                    szn_stream_t stream, const float* clip = nullptr) {
    if (!param || !grad || !momentum_buf || n <= 0) SZN_FAIL(SZN_ERR_ARG, "sgd_momentum_step: bad argument");
    if (w_lp && !szn_is16(w_lp_dtype)) SZN_FAIL(SZN_ERR_ARG, "sgd_momentum_step: the weight image must be SZN_BF16 or SZN_F16");
    if (grad_dtype != SZN_F32 && !szn_is16(grad_dtype)) SZN_FAIL(SZN_ERR_ARG, "sgd_momentum_step: the gradient must be SZN_F32, SZN_BF16 or SZN_F16");
    const uintptr_t galign = grad_dtype == SZN_F32 ? 15 : 7;
    const int vec = ((((uintptr_t)param | (uintptr_t)momentum_buf) & 15) == 0 && ((uintptr_t)grad & galign) == 0 &&
                     (((uintptr_t)w_lp) & 7) == 0) ? 1 : 0;
    const dim3 grid(szn_grid_for(vec ? (n + 3) / 4 : n, 256, 1 << 24));
    const bool lp_f16 = w_lp && w_lp_dtype == SZN_F16;    // (grad_dtype was checked above)
    szn_by_dtype(grad_dtype, [&](auto gtag) {
        using G = decltype(gtag);
        const auto kernel = lp_f16 ? sgd_kernel<f16_raw, G> : sgd_kernel<bf16_raw, G>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, param, grad, momentum_buf, n, lr, momentum, weight_decay,
                           first_step, grad_scale, (uint16_t*)w_lp, vec, dyn, clip);
    });
    SZN_CHECK_LAUNCH(grad_dtype == SZN_F32 ? "sgd_kernel" : "sgd_kernel_g16");
    return SZN_OK;
}

extern "C" int szn_sgd_momentum_step(long n, float* param, const float* grad, float* momentum_buf, float lr,
                                     float momentum, float weight_decay, int first_step, float grad_scale, void* w_lp,
                                     int w_lp_dtype, szn_stream_t stream) {
    return sgd_impl(n, param, grad, SZN_F32, momentum_buf, lr, momentum, weight_decay, first_step, grad_scale, w_lp, w_lp_dtype, nullptr, stream);
}

extern "C" int szn_sgd_momentum_step_g16(long n, float* param, const void* grad, int grad_dtype, float* momentum_buf, float lr,
                                         float momentum, float weight_decay, int first_step, float grad_scale, void* w_lp,
                                         int w_lp_dtype, szn_stream_t stream) {
    if (!szn_is16(grad_dtype)) SZN_FAIL(SZN_ERR_ARG, "sgd_momentum_step_g16: the gradient image must be SZN_BF16 or SZN_F16");
    return sgd_impl(n, param, grad, grad_dtype, momentum_buf, lr, momentum, weight_decay, first_step, grad_scale, w_lp, w_lp_dtype, nullptr,
                    stream);
}

extern "C" int szn_sgd_momentum_step_scaled(long n, float* param, const float* grad, float* momentum_buf, float lr,
                                            float momentum, float weight_decay, const float* scale_state, float grad_scale,
                                            void* w_lp, int w_lp_dtype, szn_stream_t stream) {
    if (!scale_state) SZN_FAIL(SZN_ERR_ARG, "sgd_momentum_step_scaled: scale_state is NULL");
    return sgd_impl(n, param, grad, SZN_F32, momentum_buf, lr, momentum, weight_decay, 0, grad_scale, w_lp, w_lp_dtype, scale_state, stream);
}

// ---- the steps under gradient-norm clipping: supersets of the three forms above, the effective scale times clip_state[0] ----
extern "C" int szn_adam_step_clipped(long n, float* param, const void* grad, int grad_dtype, float* exp_avg, float* exp_avg_sq, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                     const float* scale_state, const float* clip_state, void* w_lp, int w_lp_dtype, szn_stream_t stream) {
    if (!clip_state) SZN_FAIL(SZN_ERR_ARG, "adam_step_clipped: clip_state is NULL");
    if (scale_state && grad_dtype != SZN_F32) SZN_FAIL(SZN_ERR_ARG, "adam_step_clipped: scale_state goes with an SZN_F32 gradient only");
    return adam_impl(n, param, grad, grad_dtype, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, scale_state ? 1 : step,
                     grad_scale, w_lp, w_lp_dtype, scale_state, stream, clip_state);
}

extern "C" int szn_sgd_momentum_step_clipped(long n, float* param, const void* grad, int grad_dtype, float* momentum_buf, float lr,
                                             float momentum, float weight_decay, int first_step, float grad_scale,
                                             const float* scale_state, const float* clip_state, void* w_lp, int w_lp_dtype,
                                             szn_stream_t stream) {
    if (!clip_state) SZN_FAIL(SZN_ERR_ARG, "sgd_momentum_step_clipped: clip_state is NULL");
    if (scale_state && grad_dtype != SZN_F32)
        SZN_FAIL(SZN_ERR_ARG, "sgd_momentum_step_clipped: scale_state goes with an SZN_F32 gradient only");
    return sgd_impl(n, param, grad, grad_dtype, momentum_buf, lr, momentum, weight_decay, scale_state ? 0 : first_step, grad_scale, w_lp,
                    w_lp_dtype, scale_state, stream, clip_state);
}

// ---- dynamic loss scaling (fp16 path) ------------------------------------------------------------------------------------------
// state = {scale S, found_inf, optimizer steps applied, clean steps since S last changed}
__global__ __launch_bounds__(256) void grad_finite_kernel(const float* __restrict__ g, long n, float* __restrict__ state, int vec) {
    const long n4 = vec ? (n >> 2) : 0;
    bool bad = false;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4_t q = ((const f32x4_t*)g)[i];
        // x - x is 0 for every finite x and NaN for +-inf / NaN
        const float z = (q[0] - q[0]) + (q[1] - q[1]) + (q[2] - q[2]) + (q[3] - q[3]);
        bad |= !(z == 0.f);
    }
    for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) bad |= !((g[i] - g[i]) == 0.f);
    if (__any(bad) && (threadIdx.x & 63) == 0) state[1] = 1.f;      // every writer stores the same value
}

__global__ void loss_scale_update_kernel(float* __restrict__ st, float growth, float backoff, int interval, float lo, float hi) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st[1] != 0.f) {                                  // overflow: the optimizer kernels skipped this step
        st[0] = fmaxf(st[0] * backoff, lo);
        st[3] = 0.f;
    } else {
        st[2] += 1.f;
        st[3] += 1.f;
        if (st[3] >= (float)interval) { if (st[0] < hi) st[0] = fminf(st[0] * growth, hi); st[3] = 0.f; }   // growth never lowers S
    }
    st[1] = 0.f;
}

extern "C" int szn_grad_check_finite(long n, const float* grad, float* scale_state, szn_stream_t stream) {
    if (!grad || !scale_state || n <= 0) SZN_FAIL(SZN_ERR_ARG, "grad_check_finite: bad argument");
    const int vec = (((uintptr_t)grad) & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(grad_finite_kernel, dim3(szn_grid_for(vec ? (n + 3) / 4 : n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, grad,
                       n, scale_state, vec);
    SZN_CHECK_LAUNCH("grad_finite_kernel");
    return SZN_OK;
}

extern "C" int szn_loss_scale_update(float* scale_state, float growth, float backoff, int growth_interval, float min_scale,
                                     float max_scale, szn_stream_t stream) {
    if (!scale_state || growth < 1.f || backoff <= 0.f || backoff > 1.f || growth_interval < 1)
        SZN_FAIL(SZN_ERR_ARG, "loss_scale_update: bad argument");
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scale_state, growth, backoff,
                       growth_interval, min_scale, max_scale);
    SZN_CHECK_LAUNCH("loss_scale_update_kernel");
    return SZN_OK;
}
