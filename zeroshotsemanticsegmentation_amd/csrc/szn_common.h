// szn_common.h -- shared device/host helpers for libszn_hip.so (gfx950 / CDNA4 only).
//
// Conventions used by every kernel in this library:
//   * activations are NHWC ("pixel-major"): [B][H][W][C], C contiguous; the element type T is
//     float (parity path) or bf16 (throughput path); accumulation is always fp32.
//   * conv weights are OHWI: [Cout][KH][KW][Cin] (== torch channels_last of an (O,I,KH,KW) tensor).
//   * every launch goes to the caller's hipStream_t, no host synchronisation inside.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <math.h>
#include <type_traits>
#include "../../include/szn.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// ---- error plumbing -------------------------------------------------------------------------
void szn_set_error(const char* fmt, ...);
#define SZN_FAIL(code, ...) do { szn_set_error(__VA_ARGS__); return (code); } while (0)
void szn_note_kernel(const char* name);          /* thread-local: the kernel the dispatcher picked (szn_last_kernel) */
void szn_note_colsum_rows(int rows);             /* thread-local: partial rows the last call wrote into its colsum slab */
int szn_noted_colsum_rows(void);                /* (internal: read back inside the SAME entry point, published through its out-parameter) */
float szn_noted_work_fraction(void);
static inline void szn_publish_result(const szn_conv_desc_t* d) {
    if (d && d->result) { d->result->colsum_rows = szn_noted_colsum_rows(); d->result->work_fraction = szn_noted_work_fraction(); }
}
void szn_note_work_fraction(float f);
int szn_knob(const char* name, int dflt);        /* environment knob, registered in szn_runtime.hip's table (aborts on an unlisted name) */
int szn_knob_live(const char* name, int dflt);   /* the same, re-read on every call (the tests flip it inside one process) */            /* thread-local: fraction of the dense tiles the last conv call executed (constant-border hint) */
#define SZN_CHECK_LAUNCH(name) do { hipError_t e__ = hipGetLastError(); szn_note_kernel(name); \
    if (e__ != hipSuccess) SZN_FAIL(SZN_ERR_LAUNCH, "%s: %s", name, hipGetErrorString(e__)); } while (0)

// ---- Adam, one element (torch.optim.Adam's scalar chain; no contraction: -ffp-contract=off).  Shared by adam_kernel
//      (szn_optim.hip) and the epilogue of conv_wgrad_wide<T, true> (szn_conv2d_wgrad_adam): the same instructions on the same
//      values, so the fused and the separate update agree bit for bit. ----
__device__ __forceinline__ float adam_elem(float& pi, float gi, float& mi, float& vi, float b1, float b2, float eps, float wd,
                                           float step_size, float inv_bc2_sqrt, float gscale) {
    gi = gi * gscale;
    if (wd != 0.f) gi = fmaf(wd, pi, gi);
    mi = b1 * mi + (1.f - b1) * gi;
    vi = b2 * vi + (1.f - b2) * gi * gi;
    const float denom = sqrtf(vi) * inv_bc2_sqrt + eps;
    pi -= step_size * (mi / denom);
    return pi;
}
// host side of the same step: step_size = lr / (1 - beta1^t), inv_bc2_sqrt = 1 / sqrt(1 - beta2^t)
inline void szn_adam_scalars(float lr, float beta1, float beta2, int step, float* step_size, float* inv_bc2_sqrt) {
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    *step_size = (float)((double)lr / bc1);
    *inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
}

// ---- counter-based random bits: splitmix64 of (seed * 0xD1342543DE82EF95 + counter).  Shared by dropout_mask_kernel (szn_elementwise.hip)
//      and the noise of the visualisation panels (szn_viz.hip). ----
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- class sets ---------------------------------------------------------------------------
// class sets travel as kernel arguments (4 words = SZN_MAX_CLASSES bits).  Words are picked by selects, not by a dynamic index
// into the by-value struct (which would put it in scratch).
struct ClassBits {
    uint64_t w[4];
};
__device__ __forceinline__ uint64_t class_word(const ClassBits& s, int i) {
    return i == 0 ? s.w[0] : (i == 1 ? s.w[1] : (i == 2 ? s.w[2] : s.w[3]));
}
__device__ __forceinline__ bool in_set(const ClassBits& s, long k) {
    return k >= 0 && k < SZN_MAX_CLASSES && ((class_word(s, (int)(k >> 6)) >> (k & 63)) & 1ull);
}
inline ClassBits class_bits(const szn_class_set* s) {
    ClassBits b{};
    if (s) for (int i = 0; i < 4; ++i) b.w[i] = s->w[i];
    return b;
}
inline ClassBits class_bits64(uint64_t w0) {
    ClassBits b{};
    b.w[0] = w0;
    return b;
}
inline bool class_bits_any(const ClassBits& b) { return (b.w[0] | b.w[1] | b.w[2] | b.w[3]) != 0; }
inline bool class_bits_fit(const ClassBits& b, int K) {          // no member >= K
    for (int k = K < 0 ? 0 : K; k < SZN_MAX_CLASSES; ++k)
        if ((b.w[k >> 6] >> (k & 63)) & 1ull) return false;
    return true;
}

// ---- element type traits --------------------------------------------------------------------
struct bf16_raw { uint16_t v; };

__device__ __forceinline__ float bf16_bits_to_f32(uint16_t b) {
    return __uint_as_float(((uint32_t)b) << 16);
}
// round-to-nearest-even, NaN stays NaN (same rule as torch's float -> bfloat16 cast): gfx950 converts in hardware
// (v_cvt_pk_bf16_f32: one instruction per PAIR instead of ~7 VALU operations per element -- the conversions were a third of the
// VALU work of the 16-bit epilogues)
__device__ __forceinline__ uint16_t f32_to_bf16_bits(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }

// IEEE half as a 16-bit storage type (SZN_F16: BASELINE configs[4] "fp16 activations"); converted by the hardware's
// round-to-nearest-even v_cvt_f16_f32 / v_cvt_f32_f16
struct f16_raw { uint16_t v; };
__device__ __forceinline__ float f16_bits_to_f32(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
__device__ __forceinline__ uint16_t f32_to_f16_bits(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }

template <typename T> struct elem;
template <> struct elem<float> {
    static constexpr int kPer16B = 4;
    __device__ static __forceinline__ float ld(const float* p) { return *p; }
    __device__ static __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct elem<bf16_raw> {
    static constexpr int kPer16B = 8;
    __device__ static __forceinline__ float ld(const bf16_raw* p) { return bf16_bits_to_f32(p->v); }
    __device__ static __forceinline__ void st(bf16_raw* p, float v) { p->v = f32_to_bf16_bits(v); }
};

template <> struct elem<f16_raw> {
    static constexpr int kPer16B = 8;
    __device__ static __forceinline__ float ld(const f16_raw* p) { return f16_bits_to_f32(p->v); }
    __device__ static __forceinline__ void st(f16_raw* p, float v) { p->v = f32_to_f16_bits(v); }
};

// 16-bit kernels are templated on the storage type (bf16_raw | f16_raw): conversions and the MFMA opcode are the only
// differences, the LDS-DMA / fragment plumbing moves raw 16-bit patterns
// (primary templates = bf16, so that code shared with the float instantiation still compiles; f16_raw is specialised)
template <typename T> __device__ __forceinline__ uint16_t to_bits16(float f) { return f32_to_bf16_bits(f); }
template <> __device__ __forceinline__ uint16_t to_bits16<f16_raw>(float f) { return f32_to_f16_bits(f); }
template <typename T> __device__ __forceinline__ float from_bits16(uint16_t b) { return bf16_bits_to_f32(b); }
template <> __device__ __forceinline__ float from_bits16<f16_raw>(uint16_t b) { return f16_bits_to_f32(b); }
typedef __attribute__((ext_vector_type(2))) __bf16 szn_bf16x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 szn_f16x2_t;
typedef __attribute__((ext_vector_type(2))) float szn_f32x2_t;
template <typename T> __device__ __forceinline__ uint32_t pack2(float lo, float hi) {       // v_cvt_pk_bf16_f32
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((szn_f32x2_t){lo, hi}, szn_bf16x2_t));
}
template <> __device__ __forceinline__ uint32_t pack2<f16_raw>(float lo, float hi) {        // v_cvt_pk_f16_f32 (RNE)
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((szn_f32x2_t){lo, hi}, szn_f16x2_t));
}
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) uint32_t szn_u32x4_t;
// D += A(16 x 32) * B(32 x 16) with 8 consecutive k per lane in one 128-bit register group
template <typename T> __device__ __forceinline__ f32x4_t mfma16(szn_u32x4_t a, szn_u32x4_t b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4_t mfma16<f16_raw>(szn_u32x4_t a, szn_u32x4_t b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
static inline bool szn_is16(int dtype) { return dtype == SZN_BF16 || dtype == SZN_F16; }
// fp32 storage: SZN_F32, and SZN_BF16X3 (fp32 tensors, split-bf16 products inside the conv GEMMs; include/szn.h)
static inline bool szn_store_f32(int dtype) { return dtype == SZN_F32 || dtype == SZN_BF16X3; }
static inline size_t szn_esize(int dtype) { return szn_store_f32(dtype) ? 4 : 2; }

// ---- bf16x3 (SZN_BF16X3): the GEMM kernels' fp32 instantiations, with x = hi + lo split into two RNE bf16 values ----------------
// f32x3_t is the storage tag of those instantiations: 4 bytes, loaded and stored as float, so every fp32 address / byte computation
// and every epilogue is the fp32 one.  Only the fragment -> MFMA step differs.
struct f32x3_t { float v; };
template <> struct elem<f32x3_t> {
    static constexpr int kPer16B = 4;
    __device__ static __forceinline__ float ld(const f32x3_t* p) { return p->v; }
    __device__ static __forceinline__ void st(f32x3_t* p, float v) { p->v = v; }
};
// four fp32 K values of one lane -> [hi0 hi1 hi2 hi3 | lo0 lo1 lo2 lo3] as bf16 pairs; hi = rne(x), lo = rne(x - hi) (the
// subtraction is exact).  Done once per fragment, right after its LDS read.
__device__ __forceinline__ szn_u32x4_t x3_split(float x0, float x1, float x2, float x3) {
    const uint32_t h01 = pack2<bf16_raw>(x0, x1), h23 = pack2<bf16_raw>(x2, x3);
    const uint32_t l01 = pack2<bf16_raw>(x0 - __uint_as_float(h01 << 16), x1 - __uint_as_float(h01 & 0xffff0000u));
    const uint32_t l23 = pack2<bf16_raw>(x2 - __uint_as_float(h23 << 16), x3 - __uint_as_float(h23 & 0xffff0000u));
    return szn_u32x4_t{h01, h23, l01, l23};
}
__device__ __forceinline__ szn_u32x4_t x3_split(szn_u32x4_t f) {
    return x3_split(__uint_as_float(f.x), __uint_as_float(f.y), __uint_as_float(f.z), __uint_as_float(f.w));
}
// acc += A.B over the 4 K values of split fragments a = [a_hi | a_lo], b = [b_hi | b_lo] (same lane -> K mapping on both sides):
//   [a_hi | a_lo] . [b_hi | b_hi] = hi.hi + lo.hi,   [a_hi | a_lo] . [b_lo | 0] = hi.lo      (lo.lo dropped)
__device__ __forceinline__ f32x4_t x3_mma(szn_u32x4_t a, szn_u32x4_t b, f32x4_t c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                __builtin_bit_cast(bf16x8_t, (szn_u32x4_t{b.x, b.y, b.x, b.y})), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                   __builtin_bit_cast(bf16x8_t, (szn_u32x4_t{b.z, b.w, 0u, 0u})), c, 0, 0, 0);
}

// ---- wave helpers (wave = 64 lanes) ---------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

static inline int szn_div_up(long a, long b) { return (int)((a + b - 1) / b); }
// blocks of a grid-stride launch over n items: at least 1, at most cap
static inline int szn_grid_for(long n, int per_block = 256, int cap = 8192) {
    long b = (n + per_block - 1) / per_block;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// ---- streaming passes over a 4-byte-aligned fp32 pointer pair (szn_ema.hip, szn_accum.hip) ------
// the split of [0, n) into a scalar head, n4 whole 16-B vectors and a scalar tail; a pair whose addresses differ modulo 16 is all head
static inline void szn_split16(const void* a, const void* b, long n, long* head, long* n4) {
    if ((((uintptr_t)a ^ (uintptr_t)b) & 15) != 0) { *head = n; *n4 = 0; return; }
    long h = (long)(((16 - ((uintptr_t)a & 15)) & 15) >> 2);
    if (h > n) h = n;
    *head = h;
    *n4 = (n - h) >> 2;
}
// blocks of 256 lanes that take one pair of vectors (or one scalar element) each, at most cap
static inline int szn_stream_grid(long n, long n4, int cap) {
    const long per_thread = n4 > 0 ? (n4 + 1) / 2 : n;          // vector pairs, or scalar elements
    const long rest = n - n4 * 4;
    return szn_grid_for(per_thread > rest ? per_thread : rest, 256, cap);
}

// ---- dtype code -> storage tag ----------------------------------------------------------------
// Calls f with bf16_raw{} / f16_raw{} / float{} for SZN_BF16 / SZN_F16 / SZN_F32 (f: a generic lambda that launches the kernel instantiated
// on decltype of its argument).  Any other code: f is not called and the result is false -- the caller keeps its own error text.
template <typename F> static inline bool szn_by_dtype(int dtype, F&& f) {
    if (dtype == SZN_BF16) f(bf16_raw{});
    else if (dtype == SZN_F16) f(f16_raw{});
    else if (dtype == SZN_F32) f(float{});
    else return false;
    return true;
}
