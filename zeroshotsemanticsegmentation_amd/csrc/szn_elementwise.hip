// szn_elementwise.hip -- HBM-bound kernels around the MFMA convolutions: conv1_1 (Cin = 3), max-pool
// forward / backward(+ReLU gate), casts, Dropout2d factors, Adam / SGD-momentum steps, library info.
//
// Reference sites: models.py:43-47 (conv1_1, pools), models.py:86,91 (Dropout2d), train.py:126-133,174-175
// (torch.optim.SGD / Adam with two parameter groups).
#include "szn_common.h"
#include "szn_cb.h"
#include <algorithm>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;

// ---- error plumbing -----------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void szn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* szn_last_error(void) { return g_err; }
static thread_local const char* g_last_kernel = "";
static thread_local const char* g_prev_kernel = "";
void szn_note_kernel(const char* name) { g_prev_kernel = g_last_kernel; g_last_kernel = name; }
extern "C" const char* szn_last_kernel(void) { return g_last_kernel; }
extern "C" const char* szn_prev_kernel(void) { return g_prev_kernel; }
static thread_local int g_colsum_rows = 0;
void szn_note_colsum_rows(int rows) { g_colsum_rows = rows; }
int szn_noted_colsum_rows(void) { return g_colsum_rows; }
// ---- tuning / A-B knobs: ONE table.  szn_knob() refuses names that are not listed here, so a knob cannot exist without its line in
//      DESIGN.md section 4 and its case in tests/test_gpu_knobs.py (which runs a step under every non-default value below). ----
static const char* const g_knobs[] = {
    "SZN_REGW_MINTILES", "SZN_WIDE_MINTILES", "SZN_WGT_MINTILES", "SZN_WGW_MINTILES",     // dispatch thresholds (a huge value = kernel family off)
    "SZN_WIDE_8PH", "SZN_8PH_KORD", "SZN_WIDE_ROWS", "SZN_WIDE_DIRECT", "SZN_IGEMM_DIRECT",  // which forward / dgrad tile kernel, K order, epilogue form
    "SZN_CONST_BORDER", "SZN_DGRAD_BORDER", "SZN_WGT_CB",                                 // constant-border hints
    "SZN_WGW_HALF", "SZN_WGW_STAGGER", "SZN_WGH_STAGGER", "SZN_WGW_XCD",                  // fc6's weight gradient (+ Adam)
};
static bool knob_listed(const char* name) {
    for (const char* k : g_knobs)
        if (!strcmp(k, name)) return true;
    return false;
}
int szn_knob_live(const char* name, int dflt) {
    if (!knob_listed(name)) { fprintf(stderr, "libszn_hip: unregistered knob %s\n", name); abort(); }
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
int szn_knob(const char* name, int dflt) { return szn_knob_live(name, dflt); }   // (callers cache it in a function-local static: read once per process)
extern "C" int szn_knob_count(void) { return (int)(sizeof(g_knobs) / sizeof(g_knobs[0])); }
extern "C" const char* szn_knob_name(int i) { return (i >= 0 && i < szn_knob_count()) ? g_knobs[i] : nullptr; }
static thread_local float g_work_fraction = 1.f;
void szn_note_work_fraction(float f) { g_work_fraction = f; }
float szn_noted_work_fraction(void) { return g_work_fraction; }

extern "C" int szn_version(void) { return 106; /* 0.1.6: szn_calib_head */ }
extern "C" int szn_device_info(int device, szn_device_info_t* out) {
    if (!out) SZN_FAIL(SZN_ERR_ARG, "device_info: null output");
    hipDeviceProp_t p;
    hipError_t e = hipGetDeviceProperties(&p, device);
    if (e != hipSuccess) SZN_FAIL(SZN_ERR_LAUNCH, "device_info: %s", hipGetErrorString(e));
    memset(out, 0, sizeof(*out));
    strncpy(out->name, p.name, sizeof(out->name) - 1);
    strncpy(out->arch, p.gcnArchName, sizeof(out->arch) - 1);
    out->compute_units = p.multiProcessorCount;
    out->wavefront = p.warpSize;
    out->lds_bytes_per_block = (int)p.sharedMemPerBlock;
    out->hbm_bytes = (int64_t)p.totalGlobalMem;
    out->clock_mhz = p.clockRate / 1000;
    return SZN_OK;
}

// A stream whose kernels only run on the compute units of `mask` (bit i of word i / 32 = CU i; hipExtStreamCreateWithCUMask).  The
// engine confines the HBM-bound weight gradient + Adam step of fc6 in a ONE-image step to part of the chip with it, so that the few-tile
// dgrads of conv5_x .. conv3_x run beside it instead of queueing for its LDS (models._Engine._side_stream).
extern "C" int szn_stream_create_cu_mask(int n_words, const uint32_t* mask, szn_stream_t* out) {
    if (!out || !mask || n_words <= 0) SZN_FAIL(SZN_ERR_ARG, "stream_create_cu_mask: null / empty argument");
    bool any = false;
    for (int i = 0; i < n_words; ++i) any = any || mask[i] != 0u;
    if (!any) SZN_FAIL(SZN_ERR_ARG, "stream_create_cu_mask: the mask selects no compute unit");
    hipStream_t s = nullptr;
    hipError_t e = hipExtStreamCreateWithCUMask(&s, (uint32_t)n_words, mask);
    if (e != hipSuccess) SZN_FAIL(SZN_ERR_LAUNCH, "stream_create_cu_mask: %s", hipGetErrorString(e));
    *out = (szn_stream_t)s;
    return SZN_OK;
}
extern "C" int szn_stream_destroy(szn_stream_t stream) {
    if (!stream) SZN_FAIL(SZN_ERR_ARG, "stream_destroy: null stream");
    hipError_t e = hipStreamDestroy((hipStream_t)stream);
    if (e != hipSuccess) SZN_FAIL(SZN_ERR_LAUNCH, "stream_destroy: %s", hipGetErrorString(e));
    return SZN_OK;
}

namespace {

// ---- conv1_1: 3 -> 64, 3x3, pad P, reads NCHW f32, writes NHWC T ---------------------------------
// fp32 MFMA (v_mfma_f32_16x16x4_f32) on an im2col fragment gathered straight from the image: a wave owns segments of
// 16 consecutive output pixels of one row; K = 27 taps*channels padded to 28 = 7 MFMA steps, the lane (g, r16) loads
// tap t = 4 s + g of pixel r16 (64-B coalesced rows of the fp32 image, each im2col element loaded exactly once).  The
// 64 x 28 filter bank is 28 VGPRs of A fragments.  With pad = 100 almost half of the segments only see zero padding:
// those skip the loads and the MFMAs and store relu(bias).  Epilogue: v_permlane16_swap pairs two cout fragments so
// that a lane stores 8 consecutive couts of its pixel (one 16-B piece in bf16, 64 contiguous bytes per pixel per
// instruction) -- the kernel is bound by the 64-channel output write.
template <typename T>
__global__ __launch_bounds__(256) void conv1_1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, T* __restrict__ out, int B,
                                                          int H, int W, int pad, int Ho, int Wo) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int lane = threadIdx.x & 63, g = lane >> 4, r16 = lane & 15;
    float wa[7][4];
    int toff[7], tdhw[7];                                // image offset of tap t relative to (ci 0, ih0, iw0); kh << 8 | kw, -1 = pad tap
    const long plane = (long)H * W;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const int t = 4 * s + g;                         // (kh*3+kw)*3+ci, the OHWI order of w
        const int kh = t / 9, kw = (t / 3) % 3, ci = t % 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) wa[s][i] = t < 27 ? w[(16 * i + r16) * 27 + t] : 0.f;
        toff[s] = (int)(ci * plane + (long)kh * W + kw);
        tdhw[s] = t < 27 ? ((kh << 8) | kw) : -1;
    }
    float bv[2][8];
    int cst[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        cst[p] = 32 * p + (g & 1) * 16 + (g >> 1) * 8;   // first of the 8 consecutive couts this lane holds after the swap
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[p][e] = bias ? bias[cst[p] + e] : 0.f;
    }
    const int nsx = (Wo + 15) >> 4;
    const long nseg = (long)B * Ho * nsx;
    const long nwaves = (long)gridDim.x * 4;
    for (long seg = (long)blockIdx.x * 4 + (threadIdx.x >> 6); seg < nseg; seg += nwaves) {
        const int sx = (int)(seg % nsx);
        const long rowid = seg / nsx;
        const int oh = (int)(rowid % Ho), b = (int)(rowid / Ho);
        const int ih0 = oh - pad, iw0 = sx * 16 - pad;
        f32x4_t acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        const bool touches = (ih0 + 2 >= 0) && (ih0 < H) && (iw0 + 17 >= 0) && (iw0 < W);      // wave-uniform
        if (touches) {
            const float* xb = x + (long)b * 3 * plane + (long)ih0 * W + iw0 + r16;
            float xv[7];
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                const int ih = ih0 + (tdhw[s] >> 8), iw = iw0 + r16 + (tdhw[s] & 255);
                const bool ok = tdhw[s] >= 0 && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
                xv[s] = ok ? xb[toff[s]] : 0.f;
            }
#pragma unroll
            for (int s = 0; s < 7; ++s)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s][i], xv[s], acc[i], 0, 0, 0);
        }
        const int ow = sx * 16 + r16;
        if constexpr (sizeof(T) == 2) {
            // 16-bit rows are 128 B: lanes r16 < 8 and r16 >= 8 exchange one 16-B piece (row_ror:8), so that ONE store instruction
            // writes the whole 128-B line of pixels 0..7 (the other one of pixels 8..15) instead of two instructions writing a
            // 64-B half of every line each
            u32x4_t v2[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                float v[8];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * p][c]), __float_as_uint(acc[2 * p + 1][c]), false, false);
                    v[c] = fmaxf(__uint_as_float(r[0]) + bv[p][c], 0.f);
                    v[4 + c] = fmaxf(__uint_as_float(r[1]) + bv[p][4 + c], 0.f);
                }
                T* oe = (T*)&v2[p];
#pragma unroll
                for (int e = 0; e < 8; ++e) elem<T>::st(oe + e, v[e]);
            }
            const bool lo = r16 < 8;
            const u32x4_t send = lo ? v2[1] : v2[0];
            u32x4_t recv;
            recv.x = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.x, 0x128, 0xf, 0xf, false);
            recv.y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.y, 0x128, 0xf, 0xf, false);
            recv.z = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.z, 0x128, 0xf, 0xf, false);
            recv.w = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.w, 0x128, 0xf, 0xf, false);
            const u32x4_t va = lo ? v2[0] : recv, vb = lo ? recv : v2[1];
            const int owa = sx * 16 + (r16 & 7), cs = lo ? cst[0] : cst[1];
            T* op = out + (((long)b * Ho + oh) * Wo + owa) * 64 + cs;
            if (owa < Wo) *(u32x4_t*)op = va;
            if (owa + 8 < Wo) *(u32x4_t*)(op + 8 * 64) = vb;
        } else if (ow < Wo) {
            T* op = out + (((long)b * Ho + oh) * Wo + ow) * 64;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                float v[8];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * p][c]), __float_as_uint(acc[2 * p + 1][c]), false, false);
                    v[c] = fmaxf(__uint_as_float(r[0]) + bv[p][c], 0.f);
                    v[4 + c] = fmaxf(__uint_as_float(r[1]) + bv[p][4 + c], 0.f);
                }
                u32x4_t o4[2];
                T* oe = (T*)o4;
#pragma unroll
                for (int e = 0; e < 8; ++e) elem<T>::st(oe + e, v[e]);
                T* o = op + cst[p];
                *(u32x4_t*)o = o4[0];
                if (sizeof(T) == 4) *(u32x4_t*)(o + 4) = o4[1];
            }
        }   // (swap partners differ in g only: same pixel, same predicate)
    }
#endif
}

// 16-bit variant (round 3): the fp32 MFMA above needs 28 x 32 = 896 matrix-pipe cycles per 16-pixel segment and ran the layer at
// 0.19 ms for a 516 MB output that a plain fill writes in 0.08 ms (tools/probe_hbm.py: 6.8 TB/s).  Here the image values and the
// filter bank are rounded to the storage type -- what every other layer of the 16-bit path does with its operands, and what the
// fused conv1_1 wgrad already does with the image -- and K = 27 (padded to 32) is ONE v_mfma_f32_16x16x32 per cout fragment:
// lane (r16, g) supplies taps 8 g .. 8 g + 7 of pixel r16.  Segments whose nine taps are all inside the image (wave-uniform test)
// load without per-tap bounds checks; segments that only see padding store a constant computed once per wave.
template <typename T>
__global__ __launch_bounds__(256) void conv1_1_fwd16_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, T* __restrict__ out, int B,
                                                            int H, int W, int pad, int Ho, int Wo) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(sizeof(T) == 2, "16-bit storage only");
    const int lane = threadIdx.x & 63, g = lane >> 4, r16 = lane & 15;
    const long plane = (long)H * W;
    u32x4_t wa[4];                                       // A fragments: couts 16 i + r16, taps 8 g .. 8 g + 7 (t >= 27: zero)
    int toff[8], tdhw[8];                                // image offset of tap e relative to (ci 0, ih0, iw0); kh << 8 | kw, -1 = pad tap
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int t = 8 * g + e;                         // (kh*3+kw)*3+ci, the OHWI order of w
        const int tt = t < 27 ? t : 0;
        const int kh = tt / 9, kw = (tt / 3) % 3, ci = tt % 3;
        toff[e] = (int)(ci * plane + (long)kh * W + kw);
        tdhw[e] = t < 27 ? ((kh << 8) | kw) : -1;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float wv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) wv[e] = (8 * g + e < 27) ? w[(16 * i + r16) * 27 + 8 * g + e] : 0.f;
        wa[i] = u32x4_t{pack2<T>(wv[0], wv[1]), pack2<T>(wv[2], wv[3]), pack2<T>(wv[4], wv[5]), pack2<T>(wv[6], wv[7])};
    }
    float bv[2][8];
    int cst[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        cst[p] = 32 * p + (g & 1) * 16 + (g >> 1) * 8;   // first of the 8 consecutive couts this lane holds after the swap
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[p][e] = bias ? bias[cst[p] + e] : 0.f;
    }
    const bool lo = r16 < 8;
    // pieces of a padding-only segment: relu(bias) in the store layout (lanes r16 < 8 hold couts cst[0] .. + 7, the others cst[1] .. + 7)
    u32x4_t cpiece;
    {
        const int p = lo ? 0 : 1;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(lo ? bv[0][e] : bv[1][e], 0.f);
        (void)p;
        cpiece = u32x4_t{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7])};
    }
    // a wave takes runs of SEGS consecutive 16-pixel segments of one output row (2 KiB of output each): one division pair per run
    // (the per-segment 64-bit index arithmetic of the fp32 kernel cost more than its MFMAs), contiguous stores
    constexpr int SEGS = 8;
    const int nsx = (Wo + 15) >> 4, nch = (nsx + SEGS - 1) / SEGS;
    const int ntask = B * Ho * nch;
    const int nwaves = (int)gridDim.x * 4;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    for (int task = wave0; task < ntask; task += nwaves) {
      const int ch = task % nch, rowid = task / nch;
      const int oh = rowid % Ho, b = rowid / Ho;
      const int ih0 = oh - pad;
      const int sx_end = min(nsx, (ch + 1) * SEGS);
      const bool rowhit = (ih0 + 2 >= 0) && (ih0 < H);
      const float* xrow = x + (long)b * 3 * plane + (long)ih0 * W + r16;
      T* orow = out + (((long)b * Ho + oh) * Wo) * 64 + (lo ? cst[0] : cst[1]);
      // (two segments per iteration and the next segments' loads issued ahead of the stores were both measured: no change)
      for (int sx = ch * SEGS; sx < sx_end; ++sx) {
        const int iw0 = sx * 16 - pad;
        const int owa = sx * 16 + (r16 & 7);
        T* op = orow + (long)owa * 64;
        const bool touches = rowhit && (iw0 + 17 >= 0) && (iw0 < W);                            // wave-uniform
        if (!touches) {
            if (owa < Wo) *(u32x4_t*)op = cpiece;
            if (owa + 8 < Wo) *(u32x4_t*)(op + 8 * 64) = cpiece;
            continue;
        }
        const float* xb = xrow + iw0;
        float xv[8];
        const bool inner = ih0 >= 0 && ih0 + 2 < H && iw0 >= 0 && iw0 + 17 < W;                 // wave-uniform: every tap of every pixel inside
        if (inner) {
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[e] = xb[toff[e]];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int ih = ih0 + (tdhw[e] >> 8), iw = iw0 + r16 + (tdhw[e] & 255);
                const bool ok = tdhw[e] >= 0 && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
                xv[e] = ok ? xb[toff[e]] : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = tdhw[e] >= 0 ? xv[e] : 0.f;                         // lane-constant mask: taps 27 .. 31 are padding
        const u32x4_t xf = u32x4_t{pack2<T>(xv[0], xv[1]), pack2<T>(xv[2], xv[3]), pack2<T>(xv[4], xv[5]), pack2<T>(xv[6], xv[7])};
        f32x4_t acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = mfma16<T>(wa[i], xf, f32x4_t{0.f, 0.f, 0.f, 0.f});
        // 16-bit rows are 128 B: lanes r16 < 8 and r16 >= 8 exchange one 16-B piece (row_ror:8), so that ONE store instruction
        // writes the whole 128-B line of pixels 0..7 (the other one of pixels 8..15)
        u32x4_t v2[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * p][c]), __float_as_uint(acc[2 * p + 1][c]), false, false);
                v[c] = fmaxf(__uint_as_float(r[0]) + bv[p][c], 0.f);
                v[4 + c] = fmaxf(__uint_as_float(r[1]) + bv[p][4 + c], 0.f);
            }
            v2[p] = u32x4_t{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7])};
        }
        const u32x4_t send = lo ? v2[1] : v2[0];
        u32x4_t recv;
        recv.x = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.x, 0x128, 0xf, 0xf, false);
        recv.y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.y, 0x128, 0xf, 0xf, false);
        recv.z = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.z, 0x128, 0xf, 0xf, false);
        recv.w = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.w, 0x128, 0xf, 0xf, false);
        const u32x4_t va = lo ? v2[0] : recv, vb = lo ? recv : v2[1];
        if (owa < Wo) *(u32x4_t*)op = va;
        if (owa + 8 < Wo) *(u32x4_t*)(op + 8 * 64) = vb;
      }
    }
#endif
}

// Staged variant (end of round 3).  The kernel above gathers 8 taps per lane per 16-pixel segment straight from memory: every one of those
// load instructions touches 4-8 cache lines, and they share the CU's address path with the stores that are the layer's real work
// (0.153 ms against 0.08 ms for a plain fill of the 516 MB output).  Here a wave parks the 3 channels x 3 rows x 130 columns of the
// image that its run of 8 segments can see in a wave-private LDS patch -- 19 coalesced loads per lane (zero = padding, by the buffer
// bounds check), issued one run ahead -- and every segment reads its 8 taps from there.  Same values, same rounding, same MFMA: same bits.
constexpr int PSF = 132;                                 // floats per patch row (130 used)
constexpr int PATCHF = 9 * PSF;                          // floats per wave
template <typename T, bool AHEAD>      // AHEAD: the next run's image loads are issued before this run's segments (19 more live VGPRs)
__global__ __launch_bounds__(256) void conv1_1_fwd16s_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, T* __restrict__ out, int B,
                                                             int H, int W, int pad, int Ho, int Wo, unsigned x_bytes, BandCut cut) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(sizeof(T) == 2, "16-bit storage only");
    // cut (round 5): rows / columns of the OUTPUT that are not stored at all -- the constant band the engine removes in front of conv1_2
    // (szn_conv1_1_fwd_c); the output is then [B][Hc][Wc][64].  An empty cut (all zeros / ends) = the full map.
    const int Hc = Ho - (cut.ye - cut.ya) - (cut.ye2 - cut.ya2), Wc = Wo - (cut.xe - cut.xa) - (cut.xe2 - cut.xa2);
    __shared__ float spatch[4 * PATCHF];
    const int lane = threadIdx.x & 63, g = lane >> 4, r16 = lane & 15;
    float* const patch = spatch + (threadIdx.x >> 6) * PATCHF;
    const unsigned plane = (unsigned)(H * W);
    const auto rsX = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)x_bytes, 0x00020000);
    u32x4_t wa[4];                                       // A fragments: couts 16 i + r16, taps 8 g .. 8 g + 7 (t >= 27: zero)
    int tpo[8];                                          // patch word of tap e for segment 0, pixel 0; -1 = pad tap
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int t = 8 * g + e;                         // (kh*3+kw)*3+ci, the OHWI order of w
        const int tt = t < 27 ? t : 0;
        const int kh = tt / 9, kw = (tt / 3) % 3, ci = tt % 3;
        tpo[e] = t < 27 ? (ci * 3 + kh) * PSF + kw + r16 : -1;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float wv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) wv[e] = (8 * g + e < 27) ? w[(16 * i + r16) * 27 + 8 * g + e] : 0.f;
        wa[i] = u32x4_t{pack2<T>(wv[0], wv[1]), pack2<T>(wv[2], wv[3]), pack2<T>(wv[4], wv[5]), pack2<T>(wv[6], wv[7])};
    }
    float bv[2][8];
    int cst[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        cst[p] = 32 * p + (g & 1) * 16 + (g >> 1) * 8;   // first of the 8 consecutive couts this lane holds after the swap
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[p][e] = bias ? bias[cst[p] + e] : 0.f;
    }
    const bool lo = r16 < 8;
    u32x4_t cpiece;                                      // a padding-only segment: relu(bias) in the store layout
    {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(lo ? bv[0][e] : bv[1][e], 0.f);
        cpiece = u32x4_t{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7])};
    }
    constexpr int SEGS = 8, NLD = 19;                    // 19 x 64 >= 9 x 130 patch elements
    const int nsx = (Wo + 15) >> 4, nch = (nsx + SEGS - 1) / SEGS;
    const int ntask = B * Hc * nch;                      // (rows enumerated in cropped coordinates)
    const int nwaves = (int)gridDim.x * 4;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    // does the run see the image at all (wave-uniform)?
    auto run_touches = [&](int task) {
        const int ch = task % nch, oh = band_unmap((task / nch) % Hc, cut.ya, cut.ye, cut.ya2, cut.ye2);
        const int ih0 = oh - pad, iwA = ch * (SEGS * 16) - pad;
        return (ih0 + 2 >= 0) && (ih0 < H) && (iwA + SEGS * 16 + 1 >= 0) && (iwA < W);
    };
    float xr[NLD];
    auto stage_load = [&](int task) {
        const int ch = task % nch, rowid = task / nch;
        const int oh = band_unmap(rowid % Hc, cut.ya, cut.ye, cut.ya2, cut.ye2), b = rowid / Hc;
        const int ih0 = oh - pad, iwA = ch * (SEGS * 16) - pad;
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = lane + 64 * k;
            const int row = (idx * 2017) >> 18;                         // idx / 130 for idx < 1216
            const int c = idx - row * 130;
            const int ci = (row * 11) >> 5, kh = row - ci * 3;          // row / 3 for row < 10
            const int ih = ih0 + kh, iw = iwA + c;
            const bool ok = idx < 9 * 130 && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
            const unsigned off = ok ? (((unsigned)(b * 3 + ci)) * plane + (unsigned)(ih * W + iw)) * 4u : 0x80000000u;
            xr[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsX, off, 0, 0));
        }
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = lane + 64 * k;
            const int row = (idx * 2017) >> 18;
            if (idx < 9 * 130) patch[row * PSF + (idx - row * 130)] = xr[k];
        }
    };
    bool have = false;                                   // xr holds the image values of the current task
    if (AHEAD && wave0 < ntask && run_touches(wave0)) { stage_load(wave0); have = true; }
    for (int task = wave0; task < ntask; task += nwaves) {
      const int ch = task % nch, rowid = task / nch;
      const int ohc = rowid % Hc, b = rowid / Hc;
      const int oh = band_unmap(ohc, cut.ya, cut.ye, cut.ya2, cut.ye2);
      const int ih0 = oh - pad;
      const int sx0 = ch * SEGS, sx_end = min(nsx, sx0 + SEGS);
      const bool rowhit = (ih0 + 2 >= 0) && (ih0 < H);
      T* orow = out + (((long)b * Hc + ohc) * Wc) * 64 + (lo ? cst[0] : cst[1]);
      if constexpr (!AHEAD) {
          if (run_touches(task)) { stage_load(task); have = true; }
      }
      if (have) stage_store();                           // (waits for this run's loads; wave-private, LDS ops of a wave stay in order)
      have = false;
      if constexpr (AHEAD) {
          const int nxt = task + nwaves;
          if (nxt < ntask && run_touches(nxt)) { stage_load(nxt); have = true; }
      }
#pragma unroll 1
      for (int sx = sx0; sx < sx_end; ++sx) {
        const int iw0 = sx * 16 - pad;
        const int owa = sx * 16 + (r16 & 7);
        const int xca = owa < Wo ? band_map(owa, cut.xa, cut.xe, cut.xa2, cut.xe2) : -1;          // cropped columns of this lane's two pixels
        const int xcb = owa + 8 < Wo ? band_map(owa + 8, cut.xa, cut.xe, cut.xa2, cut.xe2) : -1;
        const bool touches = rowhit && (iw0 + 17 >= 0) && (iw0 < W);                            // wave-uniform
        if (!touches) {
            if (xca >= 0) *(u32x4_t*)(orow + (long)xca * 64) = cpiece;
            if (xcb >= 0) *(u32x4_t*)(orow + (long)xcb * 64) = cpiece;
            continue;
        }
        const float* pp = patch + (sx - sx0) * 16;
        float xv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = pp[tpo[e] < 0 ? 0 : tpo[e]];
            xv[e] = tpo[e] < 0 ? 0.f : v;
        }
        const u32x4_t xf = u32x4_t{pack2<T>(xv[0], xv[1]), pack2<T>(xv[2], xv[3]), pack2<T>(xv[4], xv[5]), pack2<T>(xv[6], xv[7])};
        f32x4_t acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = mfma16<T>(wa[i], xf, f32x4_t{0.f, 0.f, 0.f, 0.f});
        u32x4_t v2[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * p][c]), __float_as_uint(acc[2 * p + 1][c]), false, false);
                v[c] = fmaxf(__uint_as_float(r[0]) + bv[p][c], 0.f);
                v[4 + c] = fmaxf(__uint_as_float(r[1]) + bv[p][4 + c], 0.f);
            }
            v2[p] = u32x4_t{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7])};
        }
        const u32x4_t send = lo ? v2[1] : v2[0];
        u32x4_t recv;
        recv.x = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.x, 0x128, 0xf, 0xf, false);
        recv.y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.y, 0x128, 0xf, 0xf, false);
        recv.z = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.z, 0x128, 0xf, 0xf, false);
        recv.w = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.w, 0x128, 0xf, 0xf, false);
        const u32x4_t va = lo ? v2[0] : recv, vb = lo ? recv : v2[1];
        if (xca >= 0) *(u32x4_t*)(orow + (long)xca * 64) = va;
        if (xcb >= 0) *(u32x4_t*)(orow + (long)xcb * 64) = vb;
      }
    }
#endif
}

// conv1_1 wgrad = a 1x1-conv wgrad on the im2col image: xcol[m][t] = x[b][ci][oh+kh-pad][ow+kw-pad], t = (kh*3+kw)*3+ci
// (27 taps padded to 32 "channels"), so the MFMA wgrad kernel does the reduction over the B*Ho*Wo pixels.
template <typename T>
__global__ __launch_bounds__(256) void im2col_c3_kernel(const float* __restrict__ x, T* __restrict__ xcol, int B, int H,
                                                        int W, int pad, int Ho, int Wo) {
    constexpr int CH = elem<T>::kPer16B;
    constexpr int CPR = 32 / CH;                         // 16-B chunks per row (4 bf16 / 8 f32)
    const long total = (long)B * Ho * Wo * CPR;
    const long plane = (long)H * W;
    for (long gid = (long)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (long)gridDim.x * 256) {
        const int cc = (int)(gid % CPR);
        const long p = gid / CPR;
        const int ow = (int)(p % Wo);
        const long q = p / Wo;
        const int oh = (int)(q % Ho), b = (int)(q / Ho);
        u32x4_t o;
        T* oe = (T*)&o;
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            const int t = cc * CH + e;
            float v = 0.f;
            if (t < 27) {
                const int ci = t % 3, tap = t / 3, kh = tap / 3, kw = tap - kh * 3;
                const int ih = oh + kh - pad, iw = ow + kw - pad;
                if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) v = x[((long)b * 3 + ci) * plane + (long)ih * W + iw];
            }
            elem<T>::st(oe + e, v);
        }
        *(u32x4_t*)(xcol + p * 32 + cc * CH) = o;
    }
}

__global__ void unpack_dw32_kernel(const float* __restrict__ dw32, float* __restrict__ dw, int accumulate) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 64 * 27) return;
    const int co = i / 27, t = i - co * 27;
    const float v = dw32[co * 32 + t];
    dw[i] = accumulate ? dw[i] + v : v;
}

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

// ---- casts / dropout / optimizers -----------------------------------------------------------------
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

// Optimizer steps over the flat fp32 parameter / gradient / moment buffers: pure streaming (28-30 B per element), so each
// lane moves 16 B per access (four elements) and keeps two such groups in flight; the per-element arithmetic is the
// scalar chain of torch.optim (no contraction: -ffp-contract=off), identical for the vector body and the scalar tail.
// (adam_elem: szn_common.h -- shared with the weight-gradient kernel that applies the update in its epilogue)

#ifndef SZN_ADAM_NT
#define SZN_ADAM_NT 1      // non-temporal loads / stores of master, gradient and moments: 4 GB per step that nobody reads again before the next
#endif                     // optimizer pass stays out of the caches' way (0 = default policy: the NEXT step's first kernels pay for it -- the
                           // whole step 0.05 ms slower with fc6's update fused, 0.21 ms with the separate pass: profiles/r04_ablations.txt 18)
// the gradient as the optimizer kernels read it: fp32, or a 16-bit image (szn_*_step_g16: the summed wire buffer of the exchange)
template <typename G> struct grad_src {
    __device__ static __forceinline__ f32x4_t ld4(const void* g, long i) {
#if SZN_ADAM_NT
        return __builtin_nontemporal_load((const f32x4_t*)g + i);
#else
        return ((const f32x4_t*)g)[i];
#endif
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
                                                   const float* __restrict__ dyn) {
    if (dyn) {          // dynamic loss scaling: {scale S, found_inf, steps applied, ...}; see szn_adam_step_scaled
        if (dyn[1] != 0.f) return;                       // a non-finite gradient somewhere: the whole step is skipped
        gscale = gscale / dyn[0];
        const double step = (double)dyn[2] + 1.0;
        step_size = (float)((double)lr / (1.0 - pow((double)b1, step)));
        inv_bc2_sqrt = (float)(1.0 / sqrt(1.0 - pow((double)b2, step)));
    }
    const long n4 = vec ? (n >> 2) : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4_t gq = grad_src<G>::ld4(g, i);
#if SZN_ADAM_NT
        f32x4_t pq = __builtin_nontemporal_load((const f32x4_t*)p + i),
                mq = __builtin_nontemporal_load((const f32x4_t*)m + i), vq = __builtin_nontemporal_load((const f32x4_t*)v + i);
#else
        f32x4_t pq = ((const f32x4_t*)p)[i], mq = ((const f32x4_t*)m)[i], vq = ((const f32x4_t*)v)[i];
#endif
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pq[e], me = mq[e], ve = vq[e];
            adam_elem(pe, gq[e], me, ve, b1, b2, eps, wd, step_size, inv_bc2_sqrt, gscale);
            pq[e] = pe; mq[e] = me; vq[e] = ve;
        }
#if SZN_ADAM_NT
        __builtin_nontemporal_store(mq, (f32x4_t*)m + i); __builtin_nontemporal_store(vq, (f32x4_t*)v + i);
        __builtin_nontemporal_store(pq, (f32x4_t*)p + i);
#else
        ((f32x4_t*)m)[i] = mq; ((f32x4_t*)v)[i] = vq; ((f32x4_t*)p)[i] = pq;
#endif
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
                                                  const float* __restrict__ dyn) {
    if (dyn) {
        if (dyn[1] != 0.f) return;
        gscale = gscale / dyn[0];
        first = dyn[2] == 0.f;
    }
    const long n4 = vec ? (n >> 2) : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4_t gq = grad_src<G>::ld4(g, i);
#if SZN_ADAM_NT
        f32x4_t pq = __builtin_nontemporal_load((const f32x4_t*)p + i);
        f32x4_t bq = first ? f32x4_t{0.f, 0.f, 0.f, 0.f} : __builtin_nontemporal_load((const f32x4_t*)buf + i);
#else
        f32x4_t pq = ((const f32x4_t*)p)[i];
        f32x4_t bq = first ? f32x4_t{0.f, 0.f, 0.f, 0.f} : ((const f32x4_t*)buf)[i];
#endif
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pq[e], be = bq[e];
            sgd_elem(pe, gq[e], be, lr, mom, wd, first, gscale);
            pq[e] = pe; bq[e] = be;
        }
#if SZN_ADAM_NT
        __builtin_nontemporal_store(bq, (f32x4_t*)buf + i); __builtin_nontemporal_store(pq, (f32x4_t*)p + i);
#else
        ((f32x4_t*)buf)[i] = bq; ((f32x4_t*)p)[i] = pq;
#endif
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

inline int grid_for(long n, int per_block = 256, int cap = 8192) {
    long b = (n + per_block - 1) / per_block;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace

static bool c11_cut_ok(const int* c, int Ho, int Wo, BandCut& cut) {
    cut = BandCut{0, 0, Ho, Ho, 0, 0, Wo, Wo};
    if (!c) return true;
    cut = BandCut{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]};
    return 0 <= cut.ya && cut.ya <= cut.ye && cut.ye <= cut.ya2 && cut.ya2 <= cut.ye2 && cut.ye2 <= Ho &&
           0 <= cut.xa && cut.xa <= cut.xe && cut.xe <= cut.xa2 && cut.xa2 <= cut.xe2 && cut.xe2 <= Wo;
}

static int conv1_1_fwd_impl(int dtype, int B, int H, int W, int pad, const float* x, const float* w, const float* bias, void* out,
                            const int* cutv, szn_stream_t stream);

extern "C" int szn_conv1_1_fwd(int dtype, int B, int H, int W, int pad, const float* x, const float* w,
                               const float* bias, void* out, szn_stream_t stream) {
    return conv1_1_fwd_impl(dtype, B, H, W, pad, x, w, bias, out, nullptr, stream);
}

extern "C" int szn_conv1_1_fwd_c(int dtype, int B, int H, int W, int pad, const float* x, const float* w,
                                 const float* bias, void* out, const int cut[8], szn_stream_t stream) {
    if (!cut) SZN_FAIL(SZN_ERR_ARG, "conv1_1_fwd_c: cut is NULL");
    return conv1_1_fwd_impl(dtype, B, H, W, pad, x, w, bias, out, cut, stream);
}

static int conv1_1_fwd_impl(int dtype, int B, int H, int W, int pad, const float* x, const float* w, const float* bias, void* out,
                            const int* cutv, szn_stream_t stream) {
    if (!x || !w || !out || B <= 0 || H <= 0 || W <= 0 || pad < 0) SZN_FAIL(SZN_ERR_ARG, "conv1_1_fwd: bad argument");
    const int Ho = H + 2 * pad - 2, Wo = W + 2 * pad - 2;
    BandCut cut;
    if (!c11_cut_ok(cutv, Ho, Wo, cut)) SZN_FAIL(SZN_ERR_ARG, "conv1_1_fwd_c: cut intervals must be ordered and inside the map");
    if (Ho <= 0 || Wo <= 0) SZN_FAIL(SZN_ERR_ARG, "conv1_1_fwd: empty output");
    if ((long)3 * H * W >= (1L << 31)) SZN_FAIL(SZN_ERR_UNSUPPORTED, "conv1_1_fwd: image plane too large");
    const long nseg = (long)B * Ho * ((Wo + 15) / 16);     // 16-pixel segments, one wave each (grid-stride)
    long blocks = (nseg + 3) / 4;
    if (blocks > 256 * 32) blocks = 256 * 32;
    const int mm16 = 1;            // the 16-bit paths round image / filter operands to the compute dtype in registers (one 16x16x32 MFMA per fragment)
    const long ntask = (long)B * Ho * (((Wo + 15) / 16 + 7) / 8);       // runs of 8 segments, one wave each (grid-stride)
    long blocks16 = (ntask + 3) / 4;
    if (blocks16 > 256 * 16) blocks16 = 256 * 16;
    if (ntask >= (1L << 31)) SZN_FAIL(SZN_ERR_UNSUPPORTED, "conv1_1_fwd: output too large");
    const size_t x_bytes = (size_t)B * 3 * H * W * 4;
    const bool staged = x_bytes < 0x7fff0000ul;          // (larger images: taps gathered straight from memory, conv1_1_fwd16_kernel)
    const int ahead = 1, sblocks = 1024;
    // (sweep on MI355X, bf16, B = 8: gather 165 us; staged 142 / 134 us with 4096 / 1024 blocks; + loads one run ahead 125 / 118 us:
    //  a wave pays its filter / bias set-up once for ~8 runs instead of ~2)
    if (staged && sblocks > 0 && blocks16 > sblocks) blocks16 = sblocks;
    if (cutv && !(szn_is16(dtype) && mm16 && staged))
        SZN_FAIL(SZN_ERR_UNSUPPORTED, "conv1_1_fwd_c: only the staged 16-bit kernel writes a cropped map");
    if (dtype == SZN_BF16 && mm16 && staged && ahead)
        hipLaunchKernelGGL((conv1_1_fwd16s_kernel<bf16_raw, true>), dim3((unsigned)blocks16), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                           (bf16_raw*)out, B, H, W, pad, Ho, Wo, (unsigned)x_bytes, cut);
    else if (dtype == SZN_BF16 && mm16 && staged)
        hipLaunchKernelGGL((conv1_1_fwd16s_kernel<bf16_raw, false>), dim3((unsigned)blocks16), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                           (bf16_raw*)out, B, H, W, pad, Ho, Wo, (unsigned)x_bytes, cut);
    else if (dtype == SZN_F16 && mm16 && staged && ahead)
        hipLaunchKernelGGL((conv1_1_fwd16s_kernel<f16_raw, true>), dim3((unsigned)blocks16), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                           (f16_raw*)out, B, H, W, pad, Ho, Wo, (unsigned)x_bytes, cut);
    else if (dtype == SZN_F16 && mm16 && staged)
        hipLaunchKernelGGL((conv1_1_fwd16s_kernel<f16_raw, false>), dim3((unsigned)blocks16), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                           (f16_raw*)out, B, H, W, pad, Ho, Wo, (unsigned)x_bytes, cut);
    else if (dtype == SZN_BF16 && mm16)
        hipLaunchKernelGGL(conv1_1_fwd16_kernel<bf16_raw>, dim3((unsigned)blocks16), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                           (bf16_raw*)out, B, H, W, pad, Ho, Wo);
    else if (dtype == SZN_F16 && mm16)
        hipLaunchKernelGGL(conv1_1_fwd16_kernel<f16_raw>, dim3((unsigned)blocks16), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                           (f16_raw*)out, B, H, W, pad, Ho, Wo);
    else if (dtype == SZN_BF16)
        hipLaunchKernelGGL(conv1_1_fwd_kernel<bf16_raw>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                           (bf16_raw*)out, B, H, W, pad, Ho, Wo);
    else if (dtype == SZN_F16)
        hipLaunchKernelGGL(conv1_1_fwd_kernel<f16_raw>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                           (f16_raw*)out, B, H, W, pad, Ho, Wo);
    else if (dtype == SZN_F32)
        hipLaunchKernelGGL(conv1_1_fwd_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                           (float*)out, B, H, W, pad, Ho, Wo);
    else
        SZN_FAIL(SZN_ERR_ARG, "conv1_1_fwd: bad dtype %d", dtype);
    SZN_CHECK_LAUNCH("conv1_1_fwd_kernel");
    return SZN_OK;
}

int szn_conv1_1_wgrad_fused_try(int dtype, int B, int H, int W, int pad, const float* x, const void* dout, float* dw, int accumulate,
                                void* workspace, size_t workspace_bytes, szn_stream_t stream, const int* cut = nullptr);

static constexpr size_t kC11SlabBytes = (size_t)32 << 20;
extern "C" size_t szn_conv1_1_wgrad_workspace_bytes(int dtype, int B, int H, int W, int pad) {
    if (B <= 0 || H <= 0 || W <= 0 || pad < 0) return 0;
    const size_t Ho = H + 2 * pad - 2, Wo = W + 2 * pad - 2;
    // im2col image + the [64][32] fp32 result + room for the fixed-order pixel-split slabs of the GEMM behind it (8 KiB per split)
    return (size_t)B * Ho * Wo * 32 * szn_esize(dtype) + 64 * 32 * sizeof(float) + kC11SlabBytes;
}

// dout given as the CROPPED map [B][Hc][Wc][64] that szn_conv1_1_fwd_c wrote the activations of (same cut): the removed rows / columns hold no
// image pixel in their windows, so they contribute nothing to dw.  16-bit fused kernel only; db must be NULL (it comes from column sums).
extern "C" int szn_conv1_1_wgrad_c(int dtype, int B, int H, int W, int pad, const float* x, const void* dout, float* dw,
                                   int accumulate, void* workspace, const int cut[8], szn_stream_t stream) {
    if (!x || !dout || !dw || !workspace || !cut || B <= 0 || H <= 0 || W <= 0 || pad < 0)
        SZN_FAIL(SZN_ERR_ARG, "conv1_1_wgrad_c: bad argument");
    if ((uintptr_t)workspace & 15) SZN_FAIL(SZN_ERR_ARG, "conv1_1_wgrad_c: workspace must be 16-B aligned");
    BandCut bc;
    if (!c11_cut_ok(cut, H + 2 * pad - 2, W + 2 * pad - 2, bc)) SZN_FAIL(SZN_ERR_ARG, "conv1_1_wgrad_c: bad cut");
    if (!szn_is16(dtype)) SZN_FAIL(SZN_ERR_UNSUPPORTED, "conv1_1_wgrad_c: 16-bit gradients only");
    const int rc = szn_conv1_1_wgrad_fused_try(dtype, B, H, W, pad, x, dout, dw, accumulate, workspace,
                                               szn_conv1_1_wgrad_workspace_bytes(dtype, B, H, W, pad), stream, cut);
    if (rc > 0) SZN_FAIL(SZN_ERR_UNSUPPORTED, "conv1_1_wgrad_c: the fused kernel declined this shape");
    return rc;
}

extern "C" int szn_conv1_1_wgrad(int dtype, int B, int H, int W, int pad, const float* x, const void* dout, float* dw,
                                 float* db, int accumulate, void* workspace, szn_stream_t stream) {
    if (!x || !dout || !dw || !workspace || B <= 0 || H <= 0 || W <= 0 || pad < 0)
        SZN_FAIL(SZN_ERR_ARG, "conv1_1_wgrad: bad argument");
    if ((uintptr_t)workspace & 15) SZN_FAIL(SZN_ERR_ARG, "conv1_1_wgrad: workspace must be 16-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const int Ho = H + 2 * pad - 2, Wo = W + 2 * pad - 2;
    const long M = (long)B * Ho * Wo;
    if (M >= (1L << 31)) SZN_FAIL(SZN_ERR_UNSUPPORTED, "conv1_1_wgrad: more than 2^31 pixels");
    const size_t es = szn_esize(dtype);
    if (szn_is16(dtype)) {          // fused kernel: no im2col image, padding-only pixels skipped (szn_conv1_1_wgrad.hip)
        const int rc = szn_conv1_1_wgrad_fused_try(dtype, B, H, W, pad, x, dout, dw, accumulate, workspace,
                                                   szn_conv1_1_wgrad_workspace_bytes(dtype, B, H, W, pad), stream);
        if (rc < 0) return rc;
        if (rc == 0) return db ? szn_bias_grad(dtype, M, 64, 64, dout, db, accumulate, stream) : SZN_OK;
        // The im2col path below reads ALL of dout.  szn_conv1_1_wgrad_reads() lets the producer of dout (conv1_2's dgrad under the
        // constant-border hint) leave everything outside the reported rectangle unwritten: if it promised a sub-rectangle for these
        // arguments, falling back here would sum uninitialised memory into dw -- fail instead of returning a silent wrong gradient.
        int rect[4];
        if (szn_conv1_1_wgrad_reads(dtype, B, H, W, pad, rect) == 1)
            SZN_FAIL(SZN_ERR_UNSUPPORTED, "conv1_1_wgrad: the fused kernel declined a shape for which szn_conv1_1_wgrad_reads() "
                     "reports the sub-rectangle [%d,%d) x [%d,%d): dout may be undefined outside it", rect[0], rect[1], rect[2], rect[3]);
    }
    float* dw32 = (float*)workspace;                              // [64][32]
    char* xcol = (char*)workspace + 64 * 32 * sizeof(float);      // [M][32] of dtype
    const long chunks = M * (32 / (16 / es));
    long blocks = (chunks + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    if (dtype == SZN_BF16)
        hipLaunchKernelGGL(im2col_c3_kernel<bf16_raw>, dim3((unsigned)blocks), dim3(256), 0, st, x, (bf16_raw*)xcol, B, H, W,
                           pad, Ho, Wo);
    else if (dtype == SZN_F16)
        hipLaunchKernelGGL(im2col_c3_kernel<f16_raw>, dim3((unsigned)blocks), dim3(256), 0, st, x, (f16_raw*)xcol, B, H, W,
                           pad, Ho, Wo);
    else if (dtype == SZN_F32)
        hipLaunchKernelGGL(im2col_c3_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, x, (float*)xcol, B, H, W, pad, Ho,
                           Wo);
    else
        SZN_FAIL(SZN_ERR_ARG, "conv1_1_wgrad: bad dtype %d", dtype);
    SZN_CHECK_LAUNCH("im2col_c3_kernel");
    // 1x1 "conv" over M rows: in = xcol [M][32], dout [M][64] -> dw32 [64][1][1][32]
    szn_conv_desc_t d = {dtype, 1, 1, (int)M, 32, 1, (int)M, 64, 1, 1, 0, 32, 64, 0, 0, 0};
    {   // slabs of the pixel splits (deterministic reduction) behind the im2col image, 256-B aligned
        const size_t off = ((size_t)64 * 32 * sizeof(float) + (size_t)M * 32 * es + 255) & ~(size_t)255;
        d.workspace = (char*)workspace + off;
        d.workspace_bytes = kC11SlabBytes - 256;
    }
    int rc = szn_conv2d_wgrad(&d, xcol, dout, dw32, 0, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(unpack_dw32_kernel, dim3((64 * 27 + 255) / 256), dim3(256), 0, st, (const float*)dw32, dw, accumulate);
    SZN_CHECK_LAUNCH("unpack_dw32_kernel");
    if (db) return szn_bias_grad(dtype, M, 64, 64, dout, db, accumulate, stream);
    return SZN_OK;
}

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
    if (dtype == SZN_BF16)
        hipLaunchKernelGGL(maxpool_fwd_kernel<bf16_raw>, dim3(grid_for(total, 256, 65536)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_raw*)in, (bf16_raw*)out, B, Hi, Wi, C, Ho, Wo, (uint8_t*)code);
    else if (dtype == SZN_F16)
        hipLaunchKernelGGL(maxpool_fwd_kernel<f16_raw>, dim3(grid_for(total, 256, 65536)), dim3(256), 0, (hipStream_t)stream,
                           (const f16_raw*)in, (f16_raw*)out, B, Hi, Wi, C, Ho, Wo, (uint8_t*)code);
    else if (dtype == SZN_F32)
        hipLaunchKernelGGL(maxpool_fwd_kernel<float>, dim3(grid_for(total, 256, 65536)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)in, (float*)out, B, Hi, Wi, C, Ho, Wo, (uint8_t*)code);
    else
        SZN_FAIL(SZN_ERR_ARG, "maxpool_fwd: bad dtype %d", dtype);
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
    const int grid = grid_for(total, 256, colsum ? 512 : 65536);
    float* cslab = colsum ? colsum_slab : nullptr;
    if (cslab && colsum_slab_rows < grid)
        SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd: colsum_slab holds %d rows, %d needed", colsum_slab_rows, grid);
    szn_note_colsum_rows(cslab ? grid : 0);
    if (colsum_rows_out) *colsum_rows_out = cslab ? grid : 0;
    if (dtype == SZN_BF16)
        hipLaunchKernelGGL(maxpool_bwd_kernel<bf16_raw>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_raw*)in, (const bf16_raw*)out, (const bf16_raw*)dout, (bf16_raw*)din, B, Hi, Wi, C,
                           Ho, Wo, colsum, cslab);
    else if (dtype == SZN_F16)
        hipLaunchKernelGGL(maxpool_bwd_kernel<f16_raw>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                           (const f16_raw*)in, (const f16_raw*)out, (const f16_raw*)dout, (f16_raw*)din, B, Hi, Wi, C,
                           Ho, Wo, colsum, cslab);
    else if (dtype == SZN_F32)
        hipLaunchKernelGGL(maxpool_bwd_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                           (const float*)in, (const float*)out, (const float*)dout, (float*)din, B, Hi, Wi, C, Ho, Wo, colsum, cslab);
    else
        SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd: bad dtype %d", dtype);
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
    const int grid = grid_for(total, 256, sums ? 512 : 65536);      // (512: see szn_maxpool2x2_ceil_bwd)
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
#define SZN_POOLBWD_LAUNCH(TT, SK)                                                                                                      \
    hipLaunchKernelGGL((maxpool_bwd_code_kernel<TT, SK>), dim3(grid), dim3(256), 0, st, (const uint8_t*)code, (const TT*)dout, (TT*)din, B, \
                       Hi, Wi, C, Ho, Wo, colsum, cslab, sk, sk2, skip_slab, PoolGather{})
#define SZN_POOLBWD_BY_SKIP(TT) do { if (gather) hipLaunchKernelGGL((maxpool_bwd_code_kernel<TT, 0, true>), dim3(grid), dim3(256), 0, st, (const uint8_t*)code, (const TT*)dout, (TT*)din, B, Hi, Wi, C, Ho, Wo, colsum, cslab, sk, sk2, skip_slab, *gather); \
    else if (nsk == 2) SZN_POOLBWD_LAUNCH(TT, 2); else if (nsk == 1) SZN_POOLBWD_LAUNCH(TT, 1); else SZN_POOLBWD_LAUNCH(TT, 0); } while (0)
    if (dtype == SZN_BF16) SZN_POOLBWD_BY_SKIP(bf16_raw);
    else if (dtype == SZN_F16) SZN_POOLBWD_BY_SKIP(f16_raw);
    else if (dtype == SZN_F32) SZN_POOLBWD_BY_SKIP(float);
    else SZN_FAIL(SZN_ERR_ARG, "maxpool_bwd_code: bad dtype %d", dtype);
#undef SZN_POOLBWD_BY_SKIP
#undef SZN_POOLBWD_LAUNCH
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

extern "C" int szn_cast(int src_dtype, int dst_dtype, long n, const void* src, void* dst, szn_stream_t stream) {
    if (!src || !dst || n < 0) SZN_FAIL(SZN_ERR_ARG, "cast: bad argument");
    if (n == 0) return SZN_OK;
    hipStream_t st = (hipStream_t)stream;
    const int grid = grid_for(n);
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

template <typename G>
static void adam_launch(dim3 grid, hipStream_t st, int lp_f16, float* param, const void* grad, float* exp_avg, float* exp_avg_sq, long n,
                        float lr, float beta1, float beta2, float eps, float wd, float step_size, float inv_bc2_sqrt, float gs,
                        uint16_t* w_lp, int vec, const float* dyn) {
    if (lp_f16)
        hipLaunchKernelGGL((adam_kernel<f16_raw, G>), grid, dim3(256), 0, st, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, wd,
                           step_size, inv_bc2_sqrt, gs, w_lp, vec, dyn);
    else
        hipLaunchKernelGGL((adam_kernel<bf16_raw, G>), grid, dim3(256), 0, st, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, wd,
                           step_size, inv_bc2_sqrt, gs, w_lp, vec, dyn);
}

static int adam_impl(long n, float* param, const void* grad, int grad_dtype, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int step, float grad_scale, void* w_lp, int w_lp_dtype,
                     const float* dyn, szn_stream_t stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step < 1) SZN_FAIL(SZN_ERR_ARG, "adam_step: bad argument");
    if (w_lp && !szn_is16(w_lp_dtype)) SZN_FAIL(SZN_ERR_ARG, "adam_step: the weight image must be SZN_BF16 or SZN_F16");
    if (grad_dtype != SZN_F32 && !szn_is16(grad_dtype)) SZN_FAIL(SZN_ERR_ARG, "adam_step: the gradient must be SZN_F32, SZN_BF16 or SZN_F16");
    float step_size, inv_bc2_sqrt;
    szn_adam_scalars(lr, beta1, beta2, step, &step_size, &inv_bc2_sqrt);
    const uintptr_t galign = grad_dtype == SZN_F32 ? 15 : 7;
    const int vec = ((((uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0 && ((uintptr_t)grad & galign) == 0 &&
                     (((uintptr_t)w_lp) & 7) == 0) ? 1 : 0;
    // one 16-B group per thread, no grid-stride loop: measured 6.1 TB/s on the 135 M-element buffer vs 5.6 with 16 Ki blocks
    const dim3 grid(grid_for(vec ? (n + 3) / 4 : n, 256, 1 << 24));
    const int lp16 = (w_lp && w_lp_dtype == SZN_F16) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    if (grad_dtype == SZN_BF16)
        adam_launch<bf16_raw>(grid, st, lp16, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step_size, inv_bc2_sqrt,
                              grad_scale, (uint16_t*)w_lp, vec, dyn);
    else if (grad_dtype == SZN_F16)
        adam_launch<f16_raw>(grid, st, lp16, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step_size, inv_bc2_sqrt,
                             grad_scale, (uint16_t*)w_lp, vec, dyn);
    else
        adam_launch<float>(grid, st, lp16, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step_size, inv_bc2_sqrt,
                           grad_scale, (uint16_t*)w_lp, vec, dyn);
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

template <typename G>
static void sgd_launch(dim3 grid, hipStream_t st, int lp_f16, float* param, const void* grad, float* buf, long n, float lr, float mom,
                       float wd, int first, float gs, uint16_t* w_lp, int vec, const float* dyn) {
    if (lp_f16)
        hipLaunchKernelGGL((sgd_kernel<f16_raw, G>), grid, dim3(256), 0, st, param, grad, buf, n, lr, mom, wd, first, gs, w_lp, vec, dyn);
    else
        hipLaunchKernelGGL((sgd_kernel<bf16_raw, G>), grid, dim3(256), 0, st, param, grad, buf, n, lr, mom, wd, first, gs, w_lp, vec, dyn);
}

static int sgd_impl(long n, float* param, const void* grad, int grad_dtype, float* momentum_buf, float lr, float momentum,
                    float weight_decay, int first_step, float grad_scale, void* w_lp, int w_lp_dtype, const float* dyn,
                    szn_stream_t stream) {
    if (!param || !grad || !momentum_buf || n <= 0) SZN_FAIL(SZN_ERR_ARG, "sgd_momentum_step: bad argument");
    if (w_lp && !szn_is16(w_lp_dtype)) SZN_FAIL(SZN_ERR_ARG, "sgd_momentum_step: the weight image must be SZN_BF16 or SZN_F16");
    if (grad_dtype != SZN_F32 && !szn_is16(grad_dtype)) SZN_FAIL(SZN_ERR_ARG, "sgd_momentum_step: the gradient must be SZN_F32, SZN_BF16 or SZN_F16");
    const uintptr_t galign = grad_dtype == SZN_F32 ? 15 : 7;
    const int vec = ((((uintptr_t)param | (uintptr_t)momentum_buf) & 15) == 0 && ((uintptr_t)grad & galign) == 0 &&
                     (((uintptr_t)w_lp) & 7) == 0) ? 1 : 0;
    const dim3 grid(grid_for(vec ? (n + 3) / 4 : n, 256, 1 << 24));
    const int lp16 = (w_lp && w_lp_dtype == SZN_F16) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    if (grad_dtype == SZN_BF16)
        sgd_launch<bf16_raw>(grid, st, lp16, param, grad, momentum_buf, n, lr, momentum, weight_decay, first_step, grad_scale, (uint16_t*)w_lp, vec, dyn);
    else if (grad_dtype == SZN_F16)
        sgd_launch<f16_raw>(grid, st, lp16, param, grad, momentum_buf, n, lr, momentum, weight_decay, first_step, grad_scale, (uint16_t*)w_lp, vec, dyn);
    else
        sgd_launch<float>(grid, st, lp16, param, grad, momentum_buf, n, lr, momentum, weight_decay, first_step, grad_scale, (uint16_t*)w_lp, vec, dyn);
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
    hipLaunchKernelGGL(grad_finite_kernel, dim3(grid_for(vec ? (n + 3) / 4 : n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, grad,
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
