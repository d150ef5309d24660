// szn_viz.hip -- validation visualisations (vis_utils.py:4-109 of the reference): the uint8 RGB panels of a batch, written by one kernel.
//
// Integer-exact (the contract is stated in include/szn.h).  One thread owns a run of 4 horizontally adjacent source pixels: it loads
// their image values and labels once and writes that run into every panel of the layout.  Both layouts place cell i at panel row
// i / n_col and panel column i % n_col; they differ only in what a cell holds (viz_cell).
#include "szn_common.h"

namespace {

enum { VIZ_SEGMENTATION = 0, VIZ_SEENMASK = 1 };
constexpr int kVizMaxCells = 8;              // 2 rows x 4 columns

struct VizArgs {
    const void* img;
    const int64_t* lbl_true;                 // NULL: segmentation without the truth row
    const int64_t* lbl_pred;
    uint8_t* out;
    long row_bytes, image_bytes;
    double mean[3];                          // BGR, image kind 1 only
    uint64_t seed_mul;                       // seed * 0xD1342543DE82EF95
    ClassBits unseen;
    int B, H, W, K, img_kind, layout, n_col, n_cells;
};

__device__ __forceinline__ uint32_t pack_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

// PASCAL bit-shuffle colour of class k
__device__ __forceinline__ uint32_t class_colour(uint32_t k) {
    uint32_t r = 0, g = 0, b = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        r |= (k & 1u) << (7 - j);
        g |= ((k >> 1) & 1u) << (7 - j);
        b |= ((k >> 2) & 1u) << (7 - j);
        k >>= 3;
    }
    return pack_rgb(r, g, b);
}

__device__ __forceinline__ uint32_t unbias_u8(float x, double mean) {
    const double t = floor((double)x + mean + 0.5);
    return t < 0.0 ? 0u : (t > 255.0 ? 255u : (uint32_t)(int)t);
}

// the source pixel as packed RGB
__device__ __forceinline__ uint32_t load_rgb(const VizArgs& a, long px, long b, long hw) {
    if (a.img_kind == 0) {
        const uint8_t* p = (const uint8_t*)a.img + px * 3;
        return pack_rgb(p[0], p[1], p[2]);
    }
    const float* p = (const float*)a.img + b * 3 * hw + (px - b * hw);
    return pack_rgb(unbias_u8(p[2 * hw], a.mean[2]), unbias_u8(p[hw], a.mean[1]), unbias_u8(p[0], a.mean[0]));
}

__device__ __forceinline__ uint32_t noise_rgb(uint64_t seed_mul, long px) {
    uint32_t c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = (uint32_t)(((splitmix64(seed_mul + 3ull * (uint64_t)px + (uint64_t)i) >> 40) * 255ull) >> 24);
    return pack_rgb(c[0], c[1], c[2]);
}

struct VizPixel {
    uint32_t rgb, grey, noise;
    long lt, lp;
    bool unlabelled;
};

__device__ __forceinline__ VizPixel viz_load(const VizArgs& a, long px, long b, long hw) {
    VizPixel p;
    p.rgb = load_rgb(a, px, b, hw);
    p.grey = (19595u * (p.rgb & 255u) + 38470u * ((p.rgb >> 8) & 255u) + 7471u * (p.rgb >> 16) + 32768u) >> 16;
    p.lt = a.lbl_true ? (long)a.lbl_true[px] : 0;
    p.lp = (long)a.lbl_pred[px];
    p.unlabelled = a.lbl_true && (p.lt < 0 || (a.layout == VIZ_SEGMENTATION && p.lt >= a.K));
    p.noise = p.unlabelled ? noise_rgb(a.seed_mul, px) : 0u;
    return p;
}

// what cell i shows at this pixel.  Segmentation: rows {truth, prediction} (prediction only without lbl_true) x columns {image, colour,
// overlay, mask}; seen-mask: image, 255 * (lbl_true == 1), 255 * (lbl_pred == 1).
__device__ __forceinline__ uint32_t viz_cell(const VizArgs& a, int i, const VizPixel& p) {
    const int r = i / a.n_col, c = i - r * a.n_col;
    if (c == 0) return p.rgb;
    if (p.unlabelled) return p.noise;
    if (a.layout == VIZ_SEENMASK) return (c == 1 ? p.lt : p.lp) == 1 ? 0xffffffu : 0u;
    const long l = (a.lbl_true && r == 0) ? p.lt : p.lp;
    const bool valid = l >= 0 && l < a.K;
    if (c == 3) return (valid && !in_set(a.unseen, l)) ? 0xffffffu : 0u;
    const uint32_t col = valid ? class_colour((uint32_t)l) : 0u;
    if (c == 1) return col;
    return pack_rgb(((col & 255u) + p.grey) >> 1, (((col >> 8) & 255u) + p.grey) >> 1, ((col >> 16) + p.grey) >> 1);
}

template <bool V4>
__device__ __forceinline__ void viz_panels_body(const VizArgs& a) {
    const long w4 = (a.W + 3) / 4, hw = (long)a.H * a.W;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)a.B * a.H * w4) return;
    const long by = g / w4, x0 = (g - by * w4) * 4;
    const long b = by / a.H, y = by - b * a.H;
    const int n = V4 ? 4 : (int)(a.W - x0 < 4 ? a.W - x0 : 4);
    VizPixel p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < n) p[j] = viz_load(a, by * a.W + x0 + j, b, hw);
    uint8_t* img_out = a.out + b * a.image_bytes;
#pragma unroll
    for (int i = 0; i < kVizMaxCells; ++i) {
        if (i >= a.n_cells) continue;
        const int r = i / a.n_col, c = i - r * a.n_col;
        uint8_t* o = img_out + (r * (long)a.H + y) * a.row_bytes + ((long)c * a.W + x0) * 3;
        if (V4) {
            const uint32_t c0 = viz_cell(a, i, p[0]), c1 = viz_cell(a, i, p[1]), c2 = viz_cell(a, i, p[2]), c3 = viz_cell(a, i, p[3]);
            uint32_t* o4 = (uint32_t*)o;                     // 12 bytes, 4-B aligned (the dispatcher checked)
            o4[0] = c0 | (c1 << 24);
            o4[1] = (c1 >> 8) | (c2 << 16);
            o4[2] = (c2 >> 16) | (c3 << 8);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) {
                    const uint32_t v = viz_cell(a, i, p[j]);
                    o[3 * j] = (uint8_t)v;
                    o[3 * j + 1] = (uint8_t)(v >> 8);
                    o[3 * j + 2] = (uint8_t)(v >> 16);
                }
        }
    }
}

__global__ __launch_bounds__(256) void viz_panels_kernel(const VizArgs a) { viz_panels_body<false>(a); }
__global__ __launch_bounds__(256) void viz_panels_kernel_v4(const VizArgs a) { viz_panels_body<true>(a); }

int viz_launch(const char* who, int layout, int B, int H, int W, const void* img, int img_kind, const double* mean_bgr,
               const int64_t* lbl_true, const int64_t* lbl_pred, int K, const szn_class_set* unseen, uint64_t seed, uint8_t* out,
               long out_row_bytes, long out_image_bytes, szn_stream_t stream) {
    if (!img || !lbl_pred || !out) SZN_FAIL(SZN_ERR_ARG, "%s: img, lbl_pred and out are required", who);
    if (B <= 0 || H <= 0 || W <= 0) SZN_FAIL(SZN_ERR_ARG, "%s: empty batch or image (B %d, H %d, W %d)", who, B, H, W);
    if (img_kind != 0 && img_kind != 1) SZN_FAIL(SZN_ERR_ARG, "%s: img_kind %d (0 = uint8 RGB HWC, 1 = f32 BGR - mean NCHW)", who, img_kind);
    if (img_kind == 1 && !mean_bgr) SZN_FAIL(SZN_ERR_ARG, "%s: img_kind 1 needs mean_bgr", who);
    if (K < 1 || K > SZN_MAX_CLASSES) SZN_FAIL(SZN_ERR_ARG, "%s: K %d outside [1, %d]", who, K, SZN_MAX_CLASSES);
    VizArgs a{};
    a.unseen = class_bits(unseen);
    if (!class_bits_fit(a.unseen, K)) SZN_FAIL(SZN_ERR_ARG, "%s: the unseen set names a class >= K (%d)", who, K);
    a.layout = layout;
    a.n_col = (layout == VIZ_SEGMENTATION && unseen) ? 4 : 3;
    const int rows = (layout == VIZ_SEGMENTATION && lbl_true) ? 2 : 1;
    a.n_cells = rows * a.n_col;
    const long panel_row = 3L * a.n_col * W;
    if (out_row_bytes < panel_row) SZN_FAIL(SZN_ERR_ARG, "%s: out_row_bytes %ld below a panel row (%ld)", who, out_row_bytes, panel_row);
    const long need = ((long)rows * H - 1) * out_row_bytes + panel_row;
    if (out_image_bytes < need) SZN_FAIL(SZN_ERR_ARG, "%s: out_image_bytes %ld below a rendered image (%ld)", who, out_image_bytes, need);
    a.img = img; a.lbl_true = lbl_true; a.lbl_pred = lbl_pred; a.out = out;
    a.row_bytes = out_row_bytes; a.image_bytes = out_image_bytes;
    for (int c = 0; c < 3; ++c) a.mean[c] = mean_bgr ? mean_bgr[c] : 0.0;
    a.seed_mul = seed * 0xD1342543DE82EF95ull;
    a.B = B; a.H = H; a.W = W; a.K = K; a.img_kind = img_kind;
    const long groups = (long)B * H * ((W + 3) / 4);
    if ((groups + 255) / 256 > 0x7fffffffL) SZN_FAIL(SZN_ERR_ARG, "%s: batch too large", who);
    const dim3 grid((unsigned)((groups + 255) / 256));
    // every panel row segment of a thread is 12 bytes at a multiple of 4: three dword stores
    const bool v4 = W % 4 == 0 && out_row_bytes % 4 == 0 && out_image_bytes % 4 == 0 && ((uintptr_t)out & 3) == 0;
    if (v4) {
        hipLaunchKernelGGL(viz_panels_kernel_v4, grid, dim3(256), 0, (hipStream_t)stream, a);
        SZN_CHECK_LAUNCH("viz_panels_kernel_v4");
    } else {
        hipLaunchKernelGGL(viz_panels_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
        SZN_CHECK_LAUNCH("viz_panels_kernel");
    }
    return SZN_OK;
}

}  // namespace

extern "C" int szn_viz_segmentation(int B, int H, int W, const void* img, int img_kind, const double* mean_bgr, const int64_t* lbl_true,
                                    const int64_t* lbl_pred, int K, const szn_class_set* unseen, uint64_t seed, uint8_t* out,
                                    long out_row_bytes, long out_image_bytes, szn_stream_t stream) {
    return viz_launch("viz_segmentation", VIZ_SEGMENTATION, B, H, W, img, img_kind, mean_bgr, lbl_true, lbl_pred, K, unseen, seed, out,
                      out_row_bytes, out_image_bytes, stream);
}

extern "C" int szn_viz_seenmask(int B, int H, int W, const void* img, int img_kind, const double* mean_bgr, const int64_t* lbl_true,
                                const int64_t* lbl_pred, uint64_t seed, uint8_t* out, long out_row_bytes, long out_image_bytes,
                                szn_stream_t stream) {
    if (!lbl_true) SZN_FAIL(SZN_ERR_ARG, "viz_seenmask: lbl_true is required");
    return viz_launch("viz_seenmask", VIZ_SEENMASK, B, H, W, img, img_kind, mean_bgr, lbl_true, lbl_pred, 2, nullptr, seed, out,
                      out_row_bytes, out_image_bytes, stream);
}
