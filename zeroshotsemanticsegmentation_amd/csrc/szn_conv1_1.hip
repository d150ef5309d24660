// szn_conv1_1.hip -- conv1_1 (3 -> 64, 3x3, pad P; reads the NCHW fp32 image, writes NHWC T): forward, and the im2col fallback of its
// weight gradient (the fused weight-gradient kernel: szn_conv1_1_wgrad.hip).
//
// Reference sites: models.py:43-47 (conv1_1).
#include "szn_common.h"
#include "szn_cb.h"

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;

namespace {

// ---- conv1_1: 3 -> 64, 3x3, pad P, reads NCHW f32, writes NHWC T ---------------------------------
// What the three forward kernels below share.  lane = (g, r16): r16 = pixel of the 16-pixel segment (B operand) / cout within a 16-cout
// fragment (A operand), g = which group of K values.

struct C11Tap { int kh, kw, ci; };
__device__ __forceinline__ C11Tap c11_tap(int t) {       // t = (kh*3+kw)*3+ci, the OHWI order of w
    return C11Tap{t / 9, (t / 3) % 3, t % 3};
}

template <typename T> __device__ __forceinline__ u32x4_t c11_pack8(const float (&v)[8]) {
    return u32x4_t{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7])};
}

// 16-bit A fragments: couts 16 i + r16, taps 8 g .. 8 g + 7 (t >= 27: zero)
template <typename T> __device__ __forceinline__ void c11_filter16(const float* w, int g, int r16, u32x4_t (&wa)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float wv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) wv[e] = (8 * g + e < 27) ? w[(16 * i + r16) * 27 + 8 * g + e] : 0.f;
        wa[i] = c11_pack8<T>(wv);
    }
}

// the first of the 8 consecutive couts this lane holds after the swap of fragments 2 p, 2 p + 1; bv: their bias
__device__ __forceinline__ int c11_bias(const float* bias, int g, int p, float (&bv)[8]) {
    const int cst = 32 * p + (g & 1) * 16 + (g >> 1) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = bias ? bias[cst + e] : 0.f;
    return cst;
}

// a padding-only segment: relu(bias) in the 16-bit store layout (lanes r16 < 8 hold couts cst[0] .. + 7, the others cst[1] .. + 7)
template <typename T> __device__ __forceinline__ u32x4_t c11_cpiece(const float (&bv)[2][8], bool lo) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = fmaxf(lo ? bv[0][e] : bv[1][e], 0.f);
    return c11_pack8<T>(v);
}

// v_permlane16_swap pairs cout fragments 2 p and 2 p + 1 so that a lane holds 8 consecutive couts of its pixel; + bias, ReLU
__device__ __forceinline__ void c11_pair_bias_relu(const f32x4_t (&acc)[4], const float (&bv)[2][8], int p, float (&v)[8]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * p][c]), __float_as_uint(acc[2 * p + 1][c]), false, false);
        v[c] = fmaxf(__uint_as_float(r[0]) + bv[p][c], 0.f);
        v[4 + c] = fmaxf(__uint_as_float(r[1]) + bv[p][4 + c], 0.f);
    }
}

// 16-bit epilogue up to the two 16-B pieces a lane stores.  16-bit rows are 128 B: lanes r16 < 8 and r16 >= 8 exchange one piece
// (row_ror:8), so that ONE store instruction writes the whole 128-B line of pixels 0..7 (the other one of pixels 8..15) instead of two
// instructions writing a 64-B half of every line each.  va: pixel r16 & 7, vb: pixel (r16 & 7) + 8; couts cst[lo ? 0 : 1] .. + 7.
template <typename T>
__device__ __forceinline__ void c11_epilogue16(const f32x4_t (&acc)[4], const float (&bv)[2][8], bool lo, u32x4_t& va, u32x4_t& vb) {
    u32x4_t v2[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        float v[8];
        c11_pair_bias_relu(acc, bv, p, v);
        v2[p] = c11_pack8<T>(v);
    }
    const u32x4_t send = lo ? v2[1] : v2[0];
    u32x4_t recv;
    recv.x = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.x, 0x128, 0xf, 0xf, false);
    recv.y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.y, 0x128, 0xf, 0xf, false);
    recv.z = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.z, 0x128, 0xf, 0xf, false);
    recv.w = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.w, 0x128, 0xf, 0xf, false);
    va = lo ? v2[0] : recv;
    vb = lo ? recv : v2[1];
}

// fp32 storage.  fp32 MFMA (v_mfma_f32_16x16x4_f32) on an im2col fragment gathered straight from the image: a wave owns segments of
// 16 consecutive output pixels of one row; K = 27 taps*channels padded to 28 = 7 MFMA steps, the lane (g, r16) loads
// tap t = 4 s + g of pixel r16 (64-B coalesced rows of the fp32 image, each im2col element loaded exactly once).  The
// 64 x 28 filter bank is 28 VGPRs of A fragments.  With pad = 100 almost half of the segments only see zero padding:
// those skip the loads and the MFMAs and store relu(bias).  A lane stores 8 consecutive couts of its pixel as two 16-B pieces.
template <typename T>                                    // (float only; a template so that the kernel keeps its symbol)
__global__ __launch_bounds__(256) void conv1_1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, T* __restrict__ out, int B,
                                                          int H, int W, int pad, int Ho, int Wo) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(std::is_same<T, float>::value, "fp32 storage only");
    const int lane = threadIdx.x & 63, g = lane >> 4, r16 = lane & 15;
    float wa[7][4];
    int toff[7], tdhw[7];                                // image offset of tap t relative to (ci 0, ih0, iw0); kh << 8 | kw, -1 = pad tap
    const long plane = (long)H * W;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const int t = 4 * s + g;
        const C11Tap tp = c11_tap(t);
#pragma unroll
        for (int i = 0; i < 4; ++i) wa[s][i] = t < 27 ? w[(16 * i + r16) * 27 + t] : 0.f;
        toff[s] = (int)(tp.ci * plane + (long)tp.kh * W + tp.kw);
        tdhw[s] = t < 27 ? ((tp.kh << 8) | tp.kw) : -1;
    }
    float bv[2][8];
    int cst[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) cst[p] = c11_bias(bias, g, p, bv[p]);
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
        if (ow < Wo) {                                   // (swap partners differ in g only: same pixel, same predicate)
            T* op = out + (((long)b * Ho + oh) * Wo + ow) * 64;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                float v[8];
                c11_pair_bias_relu(acc, bv, p, v);
                T* o = op + cst[p];
                *(f32x4_t*)o = f32x4_t{v[0], v[1], v[2], v[3]};
                *(f32x4_t*)(o + 4) = f32x4_t{v[4], v[5], v[6], v[7]};
            }
        }
    }
#endif
}

// 16-bit storage, taps gathered straight from memory: the only path for an image of 2 GiB or more, which the buffer resource of the staged
// kernel below cannot address.  The image values and the filter bank are rounded to the storage type -- what every other layer of the
// 16-bit path does with its operands, and what the fused conv1_1 wgrad already does with the image -- and K = 27 (padded to 32) is ONE
// v_mfma_f32_16x16x32 per cout fragment (the fp32 MFMA above needs 28 x 32 = 896 matrix-pipe cycles per 16-pixel segment): lane (r16, g)
// supplies taps 8 g .. 8 g + 7 of pixel r16.  Segments whose nine taps are all inside the image (wave-uniform test) load without per-tap
// bounds checks; segments that only see padding store a constant computed once per wave.
template <typename T>
__global__ __launch_bounds__(256) void conv1_1_fwd16_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, T* __restrict__ out, int B,
                                                            int H, int W, int pad, int Ho, int Wo) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(sizeof(T) == 2, "16-bit storage only");
    const int lane = threadIdx.x & 63, g = lane >> 4, r16 = lane & 15;
    const long plane = (long)H * W;
    u32x4_t wa[4];
    int toff[8], tdhw[8];                                // image offset of tap e relative to (ci 0, ih0, iw0); kh << 8 | kw, -1 = pad tap
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int t = 8 * g + e;
        const C11Tap tp = c11_tap(t < 27 ? t : 0);
        toff[e] = (int)(tp.ci * plane + (long)tp.kh * W + tp.kw);
        tdhw[e] = t < 27 ? ((tp.kh << 8) | tp.kw) : -1;
    }
    c11_filter16<T>(w, g, r16, wa);
    float bv[2][8];
    int cst[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) cst[p] = c11_bias(bias, g, p, bv[p]);
    const bool lo = r16 < 8;
    const u32x4_t cpiece = c11_cpiece<T>(bv, lo);
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
        const u32x4_t xf = c11_pack8<T>(xv);
        f32x4_t acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = mfma16<T>(wa[i], xf, f32x4_t{0.f, 0.f, 0.f, 0.f});
        u32x4_t va, vb;
        c11_epilogue16<T>(acc, bv, lo, va, vb);
        if (owa < Wo) *(u32x4_t*)op = va;
        if (owa + 8 < Wo) *(u32x4_t*)(op + 8 * 64) = vb;
      }
    }
#endif
}

// 16-bit storage, staged: the kernel every 16-bit step runs.  The kernel above gathers 8 taps per lane per 16-pixel segment straight from
// memory: every one of those load instructions touches 4-8 cache lines, and they share the CU's address path with the stores that are the
// layer's real work (0.153 ms against 0.08 ms for a plain fill of the 516 MB output; tools/probe_hbm.py: 6.8 TB/s).  Here a wave parks the
// 3 channels x 3 rows x 130 columns of the image that its run of 8 segments can see in a wave-private LDS patch -- 19 coalesced loads per
// lane (zero = padding, by the buffer bounds check), issued one run ahead (19 more live VGPRs) -- and every segment reads its 8 taps from
// there.  Same values, same rounding, same MFMA: same bits.
constexpr int PSF = 132;                                 // floats per patch row (130 used)
constexpr int PATCHF = 9 * PSF;                          // floats per wave
template <typename T>
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
    u32x4_t wa[4];
    int tpo[8];                                          // patch word of tap e for segment 0, pixel 0; -1 = pad tap
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int t = 8 * g + e;
        const C11Tap tp = c11_tap(t < 27 ? t : 0);
        tpo[e] = t < 27 ? (tp.ci * 3 + tp.kh) * PSF + tp.kw + r16 : -1;
    }
    c11_filter16<T>(w, g, r16, wa);
    float bv[2][8];
    int cst[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) cst[p] = c11_bias(bias, g, p, bv[p]);
    const bool lo = r16 < 8;
    const u32x4_t cpiece = c11_cpiece<T>(bv, lo);
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
    if (wave0 < ntask && run_touches(wave0)) { stage_load(wave0); have = true; }
    for (int task = wave0; task < ntask; task += nwaves) {
      const int ch = task % nch, rowid = task / nch;
      const int ohc = rowid % Hc, b = rowid / Hc;
      const int oh = band_unmap(ohc, cut.ya, cut.ye, cut.ya2, cut.ye2);
      const int ih0 = oh - pad;
      const int sx0 = ch * SEGS, sx_end = min(nsx, sx0 + SEGS);
      const bool rowhit = (ih0 + 2 >= 0) && (ih0 < H);
      T* orow = out + (((long)b * Hc + ohc) * Wc) * 64 + (lo ? cst[0] : cst[1]);
      if (have) stage_store();                           // (waits for this run's loads; wave-private, LDS ops of a wave stay in order)
      have = false;
      const int nxt = task + nwaves;                     // the next run's image loads are issued before this run's segments
      if (nxt < ntask && run_touches(nxt)) { stage_load(nxt); have = true; }
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
        const u32x4_t xf = c11_pack8<T>(xv);
        f32x4_t acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = mfma16<T>(wa[i], xf, f32x4_t{0.f, 0.f, 0.f, 0.f});
        u32x4_t va, vb;
        c11_epilogue16<T>(acc, bv, lo, va, vb);
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

}  // namespace

static bool c11_cut_ok(const int* c, int Ho, int Wo, BandCut& cut) {
    cut = BandCut{0, 0, Ho, Ho, 0, 0, Wo, Wo};
    if (!c) return true;
    cut = BandCut{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]};
    return 0 <= cut.ya && cut.ya <= cut.ye && cut.ye <= cut.ya2 && cut.ya2 <= cut.ye2 && cut.ye2 <= Ho &&
           0 <= cut.xa && cut.xa <= cut.xe && cut.xe <= cut.xa2 && cut.xa2 <= cut.xe2 && cut.xe2 <= Wo;
}

// The staged 16-bit kernel runs at most this many blocks (sweep on MI355X, bf16, B = 8: gather 165 us; staged 142 / 134 us with 4096 / 1024
// blocks; + loads one run ahead 125 / 118 us: a wave pays its filter / bias set-up once for ~8 runs instead of ~2)
constexpr int kC11StagedBlocks = 1024;

static int conv1_1_fwd_impl(int dtype, int B, int H, int W, int pad, const float* x, const float* w, const float* bias, void* out,
                            const int* cutv, szn_stream_t stream) {
    if (!x || !w || !out || B <= 0 || H <= 0 || W <= 0 || pad < 0) SZN_FAIL(SZN_ERR_ARG, "conv1_1_fwd: bad argument");
    const int Ho = H + 2 * pad - 2, Wo = W + 2 * pad - 2;
    BandCut cut;
    if (!c11_cut_ok(cutv, Ho, Wo, cut)) SZN_FAIL(SZN_ERR_ARG, "conv1_1_fwd_c: cut intervals must be ordered and inside the map");
    if (Ho <= 0 || Wo <= 0) SZN_FAIL(SZN_ERR_ARG, "conv1_1_fwd: empty output");
    if ((long)3 * H * W >= (1L << 31)) SZN_FAIL(SZN_ERR_UNSUPPORTED, "conv1_1_fwd: image plane too large");
    const int nsx = (Wo + 15) / 16;
    const long nseg = (long)B * Ho * nsx;                  // fp32: 16-pixel segments, one wave each (grid-stride)
    const long ntask = (long)B * Ho * ((nsx + 7) / 8);     // 16-bit: runs of 8 segments, one wave each (grid-stride)
    if (ntask >= (1L << 31)) SZN_FAIL(SZN_ERR_UNSUPPORTED, "conv1_1_fwd: output too large");
    const size_t x_bytes = (size_t)B * 3 * H * W * 4;
    const bool staged = x_bytes < 0x7fff0000ul;          // (larger images: taps gathered straight from memory, conv1_1_fwd16_kernel)
    if (cutv && !(szn_is16(dtype) && staged))
        SZN_FAIL(SZN_ERR_UNSUPPORTED, "conv1_1_fwd_c: only the staged 16-bit kernel writes a cropped map");
    hipStream_t st = (hipStream_t)stream;
    const bool known = szn_by_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        if constexpr (sizeof(T) == 4)
            hipLaunchKernelGGL(conv1_1_fwd_kernel<T>, dim3(szn_grid_for(nseg, 4, 256 * 32)), dim3(256), 0, st, x, w, bias, (T*)out, B, H, W,
                               pad, Ho, Wo);
        else if (staged)
            hipLaunchKernelGGL(conv1_1_fwd16s_kernel<T>, dim3(szn_grid_for(ntask, 4, kC11StagedBlocks)), dim3(256), 0, st, x, w, bias, (T*)out,
                               B, H, W, pad, Ho, Wo, (unsigned)x_bytes, cut);
        else
            hipLaunchKernelGGL(conv1_1_fwd16_kernel<T>, dim3(szn_grid_for(ntask, 4, 256 * 16)), dim3(256), 0, st, x, w, bias, (T*)out, B, H,
                               W, pad, Ho, Wo);
    });
    if (!known) SZN_FAIL(SZN_ERR_ARG, "conv1_1_fwd: bad dtype %d", dtype);
    SZN_CHECK_LAUNCH("conv1_1_fwd_kernel");
    return SZN_OK;
}

extern "C" int szn_conv1_1_fwd(int dtype, int B, int H, int W, int pad, const float* x, const float* w,
                               const float* bias, void* out, szn_stream_t stream) {
    return conv1_1_fwd_impl(dtype, B, H, W, pad, x, w, bias, out, nullptr, stream);
}

extern "C" int szn_conv1_1_fwd_c(int dtype, int B, int H, int W, int pad, const float* x, const float* w,
                                 const float* bias, void* out, const int cut[8], szn_stream_t stream) {
    if (!cut) SZN_FAIL(SZN_ERR_ARG, "conv1_1_fwd_c: cut is NULL");
    return conv1_1_fwd_impl(dtype, B, H, W, pad, x, w, bias, out, cut, stream);
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
    const bool known = szn_by_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(im2col_c3_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, x, (T*)xcol, B, H, W, pad, Ho, Wo);
    });
    if (!known) SZN_FAIL(SZN_ERR_ARG, "conv1_1_wgrad: bad dtype %d", dtype);
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
