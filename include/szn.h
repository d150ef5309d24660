/* szn.h -- C-ABI of libszn_hip.so: the MI355X (gfx950) kernels underneath the SZN pixel-embedding
 * training path.
 *
 * The reference (RohanDoshi2018/ZeroshotSemanticSegmentation) has no FFI of its own: its "operator
 * interface" for this path is the set of torch calls made by models.py / utils.py / train.py.  Each
 * entry point below names the reference call site (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  Every pointer is a CALLER-OWNED DEVICE pointer
 *     (the library never allocates, frees or retains them) unless the comment says "host".
 *   - every function returns int: 0 = SZN_OK, <0 = error; szn_last_error() gives the text
 *     (thread-local).  No host synchronisation happens inside any entry point; every launch goes
 *     to the hipStream_t passed as `stream` (pass torch.cuda.current_stream().cuda_stream).
 *   - activations are NHWC [B][H][W][C] ("pixel-major"), conv weights OHWI [Cout][KH][KW][Cin]
 *     (== torch channels_last storage of an (O,I,KH,KW) tensor), element type given by `dtype`
 *     (SZN_F32 parity path / SZN_BF16 throughput path / SZN_F16 IEEE-half variant); accumulation is always fp32.
 *   - the network-boundary tensors keep the reference's layout: input image (B,3,H,W) NCHW f32,
 *     score (B,E,H,W) NCHW f32, labels (B,H,W) int64 with -1 = ignore.
 */
#ifndef SZN_H_
#define SZN_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* szn_stream_t; /* hipStream_t */

enum { SZN_OK = 0, SZN_ERR_ARG = -1, SZN_ERR_LAUNCH = -2, SZN_ERR_UNSUPPORTED = -3 };
enum { SZN_F32 = 0, SZN_BF16 = 1, SZN_F16 = 2, SZN_BF16X3 = 3 };   /* SZN_F16: IEEE half activations / weight images (BASELINE configs[4]) */
/* SZN_BF16X3: fp32-accurate GEMMs on the bf16 matrix cores.  Tensors are fp32 exactly as for SZN_F32 (same layouts, strides, sizes,
 * workspaces); only the products inside the conv GEMMs change.  Arithmetic contract:
 *   hi = bf16_rne(x), lo = bf16_rne(x - float(hi))   (the subtraction is exact in fp32), for every operand element x;
 *   each product a.b is computed as a_hi.b_hi + a_hi.b_lo + a_lo.b_hi (lo.lo dropped), accumulated in fp32 by the bf16 MFMA;
 *   every epilogue (bias, ReLU, gate, Dropout2d factor, split-K slabs, column sums) is the SZN_F32 one, unchanged.
 * Error per product <= ~3 * 2^-18 relative (about 1e-5), against ~4e-3 for plain bf16 operands.  A non-finite input may give NaN where
 * fp32 gives +-Inf (x - hi = Inf - Inf).
 * Taken by szn_conv2d_fwd / _dgrad / _wgrad, szn_conv2d_dgrad_gemm and szn_gemm_proj_*; the helpers the fp32 path calls around
 * them (szn_pack_weight_dgrad, szn_conv2d_dgrad_gemm_native_supported, szn_conv2d_wgrad_adam_supported, szn_conv2d_dgrad_border_region,
 * szn_conv2d_wgrad_cb_region) treat it as SZN_F32.  Every other entry point rejects it (SZN_ERR_ARG).  szn_last_kernel() names the
 * split variants with a "+bf16x3" suffix (e.g. "conv_igemm_v2+bf16x3").                                                            */

/* a set of class indices below SZN_MAX_CLASSES: bit (k % 64) of w[k / 64] = class k.  Passed by HOST pointer, read during the
 * call (NULL = the empty set); used by the *_k entry points (more than 64 classes).                                                                                        */
#define SZN_MAX_CLASSES 256
typedef struct szn_class_set {
    uint64_t w[4];
} szn_class_set;

/* ---- library -------------------------------------------------------------------------------- */
const char* szn_last_error(void);
/* Name of the kernel most recently launched by this thread's last call (e.g. "conv3x3_regw", "conv_igemm_wide",
 * "wgrad_taps_reduce"): which specialised path the dispatcher took.  Test / profiling aid -- the parity tests assert it
 * so that a specialised kernel cannot silently fall back to the generic one. */
const char* szn_last_kernel(void);
const char* szn_prev_kernel(void);   /* the launch before it (e.g. the GEMM kernel in front of a split-K epilogue) */
int szn_version(void); /* major*10000 + minor*100 + patch */
/* The environment knobs this build reads (A/B switches and dispatch thresholds; defaults = the shipped behaviour): szn_knob_count() names,
 * szn_knob_name(i) for 0 <= i < count (NULL outside).  The library refuses to read a variable that is not in this list, and
 * tests/test_gpu_knobs.py runs a training step under a non-default value of every one of them.                                              */
int szn_knob_count(void);
const char* szn_knob_name(int i);
typedef struct {
    char name[128];
    char arch[32];
    int compute_units;
    int wavefront;
    int lds_bytes_per_block;
    int64_t hbm_bytes;
    int clock_mhz;
} szn_device_info_t;
int szn_device_info(int device, szn_device_info_t* out /* host */);
/* A stream confined to the compute units of `mask` (bit i of word i / 32 = CU i; n_words x 32 bits) -- what
 * torch.cuda.Stream() would be for the reference if it split its one-image step (train.py:82-84) over two queues: the engine
 * runs fc6's HBM-bound weight gradient + Adam step there while the few-tile dgrads of conv5_x .. conv3_x use the other CUs.
 * The handle is a hipStream_t: wrap it (torch.cuda.ExternalStream) or pass it as `stream` to any entry point. */
int szn_stream_create_cu_mask(int n_words, const uint32_t* mask /* host */, szn_stream_t* out /* host */);
int szn_stream_destroy(szn_stream_t stream);

/* ---- stride-1 convolution as implicit GEMM on MFMA --------------------------------------------
 * Replaces nn.Conv2d forward/backward for conv1_2..conv5_3 (3x3 pad 1), fc6 (7x7 valid), fc7 and
 * score_fr || seenmask_score (1x1): models.py:45-97 (construction), models.py:117-149 (forward),
 * and their autograd backward triggered by trainer_fcn.py:157 / trainer_seenmask.py:81.
 * Ci must be a multiple of 64 (bf16) / 32 (f32); Co is arbitrary.                               */
/* What a call decided that its caller has to know afterwards (HOST memory, optional): filled before the entry point returns.
 * colsum_rows   = the partial rows the call wrote into its colsum slab (0: it used no slab) -- a function of the kernel the dispatcher picked;
 *                 szn_colsum_reduce_batch takes it.
 * work_fraction = 1.0, or the fraction of the dense tiles the call executed under the constant-border hint (cb_on).                        */
typedef struct szn_call_result {
    int colsum_rows;
    float work_fraction;
} szn_call_result_t;

typedef struct {
    int dtype;        /* SZN_F32 | SZN_BF16 | SZN_F16 | SZN_BF16X3 (fp32 tensors): element type of in / w / gate / out */
    int B, Hi, Wi, Ci; /* input  [B][Hi][Wi][Ci], pixel stride ldi >= Ci elements                 */
    int Ho, Wo, Co;   /* output [B][Ho][Wo][Co], pixel stride ldo >= Co; Ho = Hi + 2*pad - KH + 1 */
    int KH, KW, pad;
    int ldi, ldo, ldg; /* pixel strides (elements) of in / out / gate                            */
    int relu;         /* epilogue max(v,0)  (nn.ReLU, models.py:44..90)                           */
    int out_f32;      /* store out as float even when dtype == SZN_BF16                           */
    void* workspace;  /* optional device scratch for split-K (few output tiles, long K: fc6/fc7); */
    size_t workspace_bytes; /* used when >= B*Ho*Wo*Co*4 bytes (dgrad: B*Hi*Wi*Ci*4); NULL = never split */
    float* colsum;    /* optional f32 [Co] (dgrad: [Ci]): += column sums of the tensor being written, i.e. the
                         bias gradient of the layer that produced the gated input (saves a pass over it)  */
    void* pool_out;   /* szn_conv2d_fwd only, optional: ALSO write MaxPool2d(2, 2, ceil_mode=True) of the output
                         (models.py:47,54,63,72,81 follow a ReLU'd conv): [B][ceil(Ho/2)][ceil(Wo/2)][Co], same element
                         type as out, dense (needs ldo == Co, relu != 0).  Fused into the conv epilogue where the
                         kernel supports it (the 710^2 / 355^2 layers), else szn_maxpool2x2_ceil_fwd runs behind it */
    float* colsum_slab; /* optional fp32 workspace [colsum_slab_rows][Co] (dgrad: [..][Ci]), 16-B aligned, declared at the END of
                         the struct.  With it the kernel does NOT touch colsum: every pixel tile / persistent block writes its
                         partial column sums into its own row (result->colsum_rows rows, a function of the kernel the
                         dispatcher picked) and the caller adds them with szn_colsum_reduce_batch in a fixed order --
                         bit-reproducible bias gradients.  Without it the partials are added to colsum with fp32 atomics
                         (same value up to the order of the additions).                                            */
    int colsum_slab_rows; /* rows the slab can hold; an error is returned if the kernel needs more                  */
    void* pool_code;    /* optional, with pool_out: one byte per pooled element [B][ceil(Ho/2)][ceil(Wo/2)][Co] = position 2 dy + dx
                         of the FIRST maximum of its window (torch's scan order), or 4 when that maximum is not positive (the
                         ReLU gate): everything szn_maxpool2x2_ceil_bwd_code needs.  8-B aligned.                            */
    int pool_only;      /* with pool_out: the caller does not need the un-pooled tensor (in training it is read once, by the pool's
                         backward pass, which takes pool_code instead: 516 + 258 MB per step that are neither written nor read back);
                         `out` must still be valid memory, a kernel that fuses the pool MAY leave it unwritten             */
    int cb_on;          /* constant-border hint (optional; a kernel that does not take it computes everything).  models.py:43 pads conv1_1
                         by 100, so on the 710^2 / 355^2 maps most pixels outside the image's reach hold ONE value per channel (conv1_1
                         writes relu(bias) there) and stay that way through conv1_2 .. conv2_2 away from the tensor edge.
                         szn_conv2d_fwd: cb_rect = output rows [r0, r1) x columns [c0, c1) the image can influence; cb_const = output
                         rows / columns [r0, r1) x [c0, c1) outside of which the zero padding of the layers so far is felt.  The caller
                         asserts that the INPUT is constant accordingly, so output pixels inside cb_const and outside cb_rect are all
                         equal: a kernel that takes the hint (conv3x3_regw) runs its tiles over cb_rect and the edge frame only, and
                         broadcasts one computed pixel to the rest (out / pool_out / pool_code alike).  Same bits as the dense
                         computation.  result->work_fraction = the fraction of the dense tiles the call executed.
                         szn_conv2d_dgrad with a gate (coordinates of DIN): cb_rect = the rows x columns outside of which every pixel of
                         the gate tensor equals gate pixel (row r0 - 1, column c0) of image 0 (needs r0 >= 1) -- the kernel may read that
                         pixel instead; cb_const = the rows x columns of DIN the caller is going to read -- stores outside may be
                         skipped (DIN is undefined there; colsum still covers every pixel).  conv1_2's dgrad: its output feeds only
                         szn_conv1_1_wgrad, whose read set szn_conv1_1_wgrad_reads() reports.
                         szn_conv2d_wgrad (coordinates of the INPUT x): cb_rect = the rows x columns the image can influence, cb_const =
                         the rows x columns outside of which zero padding is felt; the caller asserts that every pixel of x inside
                         cb_const and outside cb_rect holds the same value per channel.  conv_wgrad_taps then runs only the 16 x 16
                         output tiles whose input patch is not constant; the others contribute (their column sum of dout) x (that
                         pixel) to all nine taps -- the same sum in a different order (fp32; <= 1e-5 relative against the dense
                         result, tests/test_gpu_conv.py), ignored with accumulate != 0.  result->work_fraction reports it.
                         `colsum` (otherwise unused by szn_conv2d_wgrad) may then hold that column sum [Co], computed by the producer
                         of dout over the region szn_conv2d_wgrad_cb_region() names (szn_maxpool2x2_ceil_bwd_code_cb); NULL = the
                         call sums them itself.                                                                                   */
    int cb_rect[4];
    int cb_const[4];
    int reserved_cus;   /* optional (0 = none): compute units the persistent one-block-per-CU kernels (conv3x3_regw, conv_wgrad_taps)
                         leave idle for another queue -- under data parallelism the RCCL all-reduce of the gradient buckets runs on
                         its own stream while dgrad / wgrad continue (engine.GradBuckets; train.py has no counterpart: the reference
                         is single-GPU).  Tiled kernels ignore it (their blocks come and go; the hardware interleaves the queues).  */
    void* dw_lp;        /* szn_conv2d_wgrad only, optional: deliver the weight gradient as a 16-bit image (dw_lp_dtype = SZN_BF16 |
                         SZN_F16, OHWI like dw, 8-B aligned) -- the wire format of the data-parallel gradient exchange
                         (engine.GradBuckets, SZN_GRAD_COMM=bf16; the reference is single-GPU: trainer_fcn.py:157-158 call
                         loss.backward(); optim.step() back to back).  The kernels that own the final store of a gradient element
                         (wgrad_taps_reduce, conv_wgrad_wide's epilogue, wgrad_slab_reduce) round it once from the fp32 sum and write
                         2 B instead of 4; dw must still be valid fp32 memory of the full size (scratch for the paths that finish in
                         fp32 and convert), its content is UNDEFINED afterwards.  Ignored with accumulate != 0 (error).          */
    int dw_lp_dtype;
    szn_call_result_t* result; /* optional HOST pointer: szn_conv2d_fwd / _dgrad / _wgrad / _wgrad_adam report through it (no "last call" state) */
} szn_conv_desc_t;

/* out[m][n] = epi( sum_k in(m,k) * w[n][k] + bias[n] )
 * epi(v):  relu -> (gate ? (gate[m][n] > 0 ? v : 0) : v) -> (chan_scale ? v*chan_scale[b][n] : v)
 * bias, gate, chan_scale may be NULL.  chan_scale is the Dropout2d factor per (image, channel)
 * (models.py:86,91: 0 or 1/(1-p)).                                                               */
int szn_conv2d_fwd(const szn_conv_desc_t* d, const void* in, const void* w, const float* bias,
                   const void* gate, const float* chan_scale, void* out, szn_stream_t stream);

/* wT[ci][KH-1-kh][KW-1-kw][co] = w[co][kh][kw][ci]: the weight image szn_conv2d_dgrad consumes.  */
int szn_pack_weight_dgrad(int dtype, int Co, int KH, int KW, int Ci, const void* w, void* wT,
                          szn_stream_t stream);
/* the same for n layers in ONE launch (the per-step refresh after the optimizer, train.py:126-133: most layers are a few
 * tiles and would each pay a dispatch): 16-bit images, square K x K filters, Co and Ci multiples of 64, n <= 24.          */
int szn_pack_weight_dgrad_batch(int dtype, int n, const void* const* w, void* const* wT, const int* Co, const int* K,
                                const int* Ci, szn_stream_t stream);

/* d (forward geometry) -> din[B][Hi][Wi][Ci] = conv(dout, wT) with pad' = KH-1-pad; epilogue as
 * above with gate = the forward INPUT activation (ReLU backward) and chan_scale = the dropout
 * factors that were applied to that input.  d->ldo is the pixel stride of DOUT, d->ldi of DIN.   */
int szn_conv2d_dgrad(const szn_conv_desc_t* d, const void* dout, const void* wT, const void* gate,
                     const float* chan_scale, void* din, szn_stream_t stream);
/* cb_on == 2 on a gated szn_conv2d_dgrad with colsum (conv1_2's dgrad: din feeds only szn_conv1_1_wgrad and conv1_1's bias gradient): the
 * tiles that neither store anything (outside cb_const) nor see a varying gate (outside cb_rect) are not run; colsum then covers the
 * tiles that ran, and szn_conv2d_dgrad_border_finish adds the rest from region sums of dout -- it is linear in dout there (one gate value
 * per channel), so it needs skip_sum [Co] = sum of dout over the map outside szn_conv2d_dgrad_border_region()'s inner rectangle (from the
 * producer of dout: szn_maxpool2x2_ceil_bwd_code_cb) and 1-pixel strips it reads itself.  Same value up to fp32 summation order.
 * The caller checks result->work_fraction < 1 after the dgrad call before it calls finish (a kernel that ignores the hint computes the
 * complete column sums).  workspace: 2 * 24 * B * Co floats, 16-B aligned.                                                                */
int szn_conv2d_dgrad_border_region(const szn_conv_desc_t* d, int region[8]);
int szn_conv2d_dgrad_border_finish(const szn_conv_desc_t* d, const void* dout, const void* wT, const void* gate,
                                   const float* skip_sum, float* colsum, void* workspace, szn_stream_t stream);

/* dgrad of a large-window convolution (models.py:84 fc6 = Conv2d(512, 4096, 7) backward) as GEMM + col2im: as a
 * convolution over the padded dout map szn_conv2d_dgrad executes 1.83x the algorithmic FLOPs of fc6's dgrad (most taps
 * of the border pixels are padding); here
 *   Y[(b,oh,ow)][(kh,kw,ci)] = sum_co dout[(b,oh,ow)][co] * w[co][kh][kw][ci]   (fp32, in d->workspace)
 *   din[b][ih][iw][ci]       = sum_{kh,kw} Y[(b, ih+pad-kh, iw+pad-kw)][(kh,kw,ci)]
 * wG = the plain transpose [KH*KW*Ci][Co] of the OHWI filter bank, i.e. szn_pack_weight_dgrad(dtype, Co, 1, 1,
 * KH*KW*Ci, w, wG).  d = forward geometry (d->ldo = pixel stride of dout, d->ldi of din); d->workspace must hold
 * szn_conv2d_dgrad_gemm_workspace_bytes(d) = B*Ho*Wo*KH*KW*Ci*4 bytes.  Co must be a multiple of 64 (bf16) / 32
 * (f32) like every reduction dimension of szn_conv2d_*; Ci a multiple of 4.  No gate / chan_scale / colsum epilogue
 * (fc6's input is a pooled map: the ReLU gate is applied by szn_maxpool2x2_ceil_bwd).                          */
size_t szn_conv2d_dgrad_gemm_workspace_bytes(const szn_conv_desc_t* d);
int szn_conv2d_dgrad_gemm(const szn_conv_desc_t* d, const void* dout, const void* wG, void* din,
                          szn_stream_t stream);
/* The same dgrad on the filter bank in its FORWARD layout w [Co][KH][KW][Ci] (no transposed copy per optimizer step: for fc6 that copy
 * is 205 MB in + 205 MB out): Y = dout x w runs on the two-K-major-operand kernel of the wide weight gradient with A = dout^T (only the
 * small dout is transposed, into the workspace).  16-bit dtypes, dense dout (ldo == Co), B*Ho*Wo a multiple of 8 and >= 256, enough
 * 256 x 256 tiles: szn_conv2d_dgrad_gemm_native_supported(d) says whether this shape qualifies (callers fall back to
 * szn_conv2d_dgrad_gemm otherwise).  Workspace: szn_conv2d_dgrad_gemm_native_workspace_bytes(d) (Y fp32 | dout^T).             */
int szn_conv2d_dgrad_gemm_native_supported(const szn_conv_desc_t* d);
size_t szn_conv2d_dgrad_gemm_native_workspace_bytes(const szn_conv_desc_t* d);
int szn_conv2d_dgrad_gemm_native(const szn_conv_desc_t* d, const void* dout, const void* w, void* din,
                                 szn_stream_t stream);

/* dw[co][kh][kw][ci] (+)= sum_pixels dout[p][co] * in[p shifted by (kh,kw)][ci]   (fp32, OHWI)
 * accumulate != 0 adds into dw (split-K partial sums are added with fp32 atomics; dw must then be
 * zero or hold a running gradient); accumulate == 0 zeroes dw first on the same stream.           */
int szn_conv2d_wgrad(const szn_conv_desc_t* d, const void* in, const void* dout, float* dw,
                     int accumulate, szn_stream_t stream);
/* Weight gradient + Adam step of the layer's weights in ONE launch (fc6 / fc7, i.e. the layers szn_conv2d_wgrad gives to
 * conv_wgrad_wide: szn_conv2d_wgrad_adam_supported == 1).  Equivalent to szn_conv2d_wgrad(accumulate = 0) followed by szn_adam_step
 * over the layer's slice (train.py:130-133,174-175: loss.backward(); optim.step()), bit for bit; only valid where the gradient
 * is final when the kernel ends (one rank, no gradient accumulation, no dynamic loss scale).  param / exp_avg / exp_avg_sq (f32)
 * and w_lp (optional image of the compute dtype) in the gradient's OHWI order; dw may be NULL (gradient not stored).
 * SZN_ERR_UNSUPPORTED (nothing launched) for other layers.                                                              */
typedef struct szn_adam_args {
    float* param; float* exp_avg; float* exp_avg_sq;
    void* w_lp; int w_lp_dtype;
    float lr, beta1, beta2, eps, weight_decay;
    int step;              /* 1-based, like szn_adam_step */
    float grad_scale;
    int grad_optional;     /* 1: the caller does not read dw afterwards: the gradient is not stored even when dw != NULL */
} szn_adam_args_t;
int szn_conv2d_wgrad_adam_supported(const szn_conv_desc_t* d);
int szn_conv2d_wgrad_adam(const szn_conv_desc_t* d, const void* x, const void* dout, float* dw,
                          const szn_adam_args_t* opt, szn_stream_t stream);

/* db[n] (+)= sum_m dout[m][n], m < M rows with pixel stride ldd.                                  */
int szn_bias_grad(int dtype, long M, int Co, int ldd, const void* dout, float* db, int accumulate,
                  szn_stream_t stream);
/* the same with a slab for the per-block partial rows ([colsum_slab_rows][Co] fp32, see szn_conv_desc_t.colsum_slab): db is
 * only zeroed (accumulate == 0), the sums arrive through szn_colsum_reduce_batch.  colsum_slab == NULL: as szn_bias_grad. */
int szn_bias_grad_slab(int dtype, long M, int Co, int ldd, const void* dout, float* db, int accumulate,
                       float* colsum_slab, int colsum_slab_rows, int* colsum_rows_out /* host, optional: rows written */, szn_stream_t stream);
/* Deterministic bias gradients.  The kernels that produce column sums (szn_conv2d_fwd / _dgrad with colsum,
 * szn_maxpool2x2_ceil_bwd, szn_bias_grad_slab) write partial rows into the caller's slab when one is given;
 * every such call reports the number of rows it wrote (0: it used no slab) through its own out-parameter (szn_conv_desc_t.result /
 * colsum_rows_out), and szn_colsum_reduce_batch adds out[j][c] += sum_{r < rows[j]} slabs[j][r * C[j] + c] for n jobs in one launch, rows in
 * ascending order (host arrays of length n; every bias gradient of a backward pass in ONE launch).                  */
int szn_colsum_reduce_batch(int n, const float* const* slabs, const int* rows, const int* C, float* const* out,
                            szn_stream_t stream);

/* the "pixel projection" of the north star: score_fr (|| seenmask_score) 1x1 conv, models.py:93,97,
 * 145,149.  Thin aliases of the conv entry points with KH=KW=1, pad=0 (M = B*h*w rows).           */
int szn_gemm_proj_fwd(int dtype, long M, int K, int N, int ldo, const void* x, const void* w,
                      const float* bias, float* out_f32, szn_stream_t stream);
int szn_gemm_proj_dgrad(int dtype, long M, int K, int N, int ldd, const void* dout, const void* wT,
                        const void* gate, const float* chan_scale, void* dx, szn_stream_t stream);
int szn_gemm_proj_wgrad(int dtype, long M, int K, int N, int ldd, const void* x, const void* dout,
                        float* dw, int accumulate, szn_stream_t stream);

/* ---- conv1_1: 3 -> 64 channels, 3x3, pad 100, reads the NCHW f32 image directly ----------------
 * models.py:43,116 (+ ReLU models.py:44).  w is OHWI f32 [64][3][3][3], out NHWC dtype.
 * dtype SZN_F32: exact fp32 products (v_mfma_f32_16x16x4_f32).  SZN_BF16 / SZN_F16: image values and filters are rounded to the
 * storage type before the 16-bit MFMA, fp32 accumulation -- the arithmetic of every other layer on those paths (max error against
 * fp32 on pixel-valued inputs 4e-3 / 6e-4 of the output range); SZN_CONV1_1_F32MMA=1 keeps fp32 operands there too.             */
int szn_conv1_1_fwd(int dtype, int B, int H, int W, int pad, const float* x_nchw, const float* w,
                    const float* bias, void* out, szn_stream_t stream);
/* The same forward pass writing a CROPPED map (round 5): cut = {ya, ye, ya2, ye2, xa, xe, xa2, xe2}, output rows [ya, ye) and [ya2, ye2) and
 * columns [xa, xe), [xa2, xe2) are not stored -- the constant band the caller removes in front of conv1_2 (models._band_cut; models.py:43 pads
 * by 100, so those rows hold relu(bias) and a 3x3 convolution behind them needs only a few of them); out is [B][Hc][Wc][64].  Staged 16-bit
 * kernel only (SZN_ERR_UNSUPPORTED otherwise: crop the full map with szn_band_remap).  szn_conv1_1_wgrad_c reads its dout in that
 * cropped layout (the removed pixels see no image pixel and contribute nothing); db is not produced (column sums of conv1_2's dgrad).   */
int szn_conv1_1_fwd_c(int dtype, int B, int H, int W, int pad, const float* x_nchw, const float* w,
                      const float* bias, void* out, const int cut[8], szn_stream_t stream);
int szn_conv1_1_wgrad_c(int dtype, int B, int H, int W, int pad, const float* x_nchw, const void* dout, float* dw,
                        int accumulate, void* workspace, const int cut[8], szn_stream_t stream);
/* dw[64][3][3][3], db[64] from dout (already ReLU-gated) -- no dgrad: the image needs no gradient.
 * bf16: a fused MFMA kernel (taps gathered from the image in registers, padding-only pixels skipped, fp32 slabs in
 * `workspace`, deterministic); f32: an MFMA wgrad over the im2col image (27 taps padded to 32) in `workspace`.  */
size_t szn_conv1_1_wgrad_workspace_bytes(int dtype, int B, int H, int W, int pad);
int szn_conv1_1_wgrad(int dtype, int B, int H, int W, int pad, const float* x_nchw,
                      const void* dout, float* dw, float* db, int accumulate, void* workspace,
                      szn_stream_t stream);
/* The part of dout a szn_conv1_1_wgrad call with db == NULL and these arguments reads: rect = rows [r0, r1) x columns [c0, c1) of
 * the (H + 2 pad - 2) x (W + 2 pad - 2) map.  Returns 1 when that is a proper sub-rectangle (the fused 16-bit kernel skips the pixels
 * whose windows hold padding only), 0 when the call reads everything (rect = the whole map).  What the producer of dout -- conv1_2's
 * dgrad -- may leave unwritten: szn_conv_desc_t.cb_const.                                                                          */
int szn_conv1_1_wgrad_reads(int dtype, int B, int H, int W, int pad, int rect[4]);

/* ---- MaxPool2d(2, stride 2, ceil_mode=True): models.py:47,54,63,72,81 ---------------------------- */
int szn_maxpool2x2_ceil_fwd(int dtype, int B, int Hi, int Wi, int C, const void* in, void* out,
                            szn_stream_t stream);
/* din = relu_bwd(pool_bwd(dout)): the gradient goes to the FIRST maximum of each window (torch
 * scan order) and is then gated by in > 0 (the ReLU that precedes every pool).                    */
int szn_maxpool2x2_ceil_bwd(int dtype, int B, int Hi, int Wi, int C, const void* in,
                            const void* out, const void* dout, void* din, float* colsum /* [C] += sum of din, or NULL */,
                            float* colsum_slab /* optional, see szn_conv_desc_t.colsum_slab */, int colsum_slab_rows,
                            int* colsum_rows_out /* host, optional: partial rows written into the slab */, szn_stream_t stream);
/* The pair that works from winner codes (one byte per pooled element: 0 .. 3 = position 2 dy + dx of the first maximum, 4 = maximum
 * not positive) instead of the pool's input: the forward pass writes them (here, or fused into the producing conv through
 * szn_conv_desc_t.pool_code), the backward pass reads d(pooled) + codes only.  Same gradients bit for bit.                     */
int szn_maxpool2x2_ceil_fwd_code(int dtype, int B, int Hi, int Wi, int C, const void* in, void* out, void* code /* or NULL */,
                                 szn_stream_t stream);
int szn_maxpool2x2_ceil_bwd_code(int dtype, int B, int Hi, int Wi, int C, const void* code, const void* dout, void* din,
                                 float* colsum, float* colsum_slab, int colsum_slab_rows, int* colsum_rows_out, szn_stream_t stream);
/* The same pass with dout given in the coordinates of the NEXT conv block's cropped input, [B][Hs][Ws][C] (szn_band_remap): the transposed band map is
 * applied while reading -- pooled pixel (oh, ow) takes the fp32 sum of source rows ytab[oh] = {start, count} x columns xtab[ow] = {start, count}
 * (device int tables of (Hi + 1) / 2 and (Wi + 1) / 2 pairs; almost every pair is {shifted index, 1}), rounded once.  Replaces the two szn_band_remap
 * passes the engine ran in front of szn_maxpool2x2_ceil_bwd_code at every cropped block boundary. */
int szn_maxpool2x2_ceil_bwd_code_gather(int dtype, int B, int Hi, int Wi, int C, const void* code, const void* dsrc, int Hs, int Ws,
                                        const int* ytab, const int* xtab, void* din, float* colsum, float* colsum_slab,
                                        int colsum_slab_rows, int* colsum_rows_out, szn_stream_t stream);
/* The same, also summing din over the regions its consumers -- the conv in front of the pool's weight gradient and dgrad -- do not run
 * tile by tile under the constant-border hint: skip_regions [n_regions][8] (pixels, even) from szn_conv2d_wgrad_cb_region() /
 * szn_conv2d_dgrad_border_region(), n_regions = 1 or 2, skip_sum [n_regions][C] out (szn_conv_desc_t.colsum of the weight-gradient call /
 * skip_sum of szn_conv2d_dgrad_border_finish), skip_slab [n_regions][colsum_slab_rows][C] scratch.  colsum / colsum_slab required. */
int szn_maxpool2x2_ceil_bwd_code_cb(int dtype, int B, int Hi, int Wi, int C, const void* code, const void* dout, void* din,
                                    float* colsum, float* colsum_slab, int colsum_slab_rows, int* colsum_rows_out, const int* skip_regions,
                                    int n_regions, float* skip_sum, float* skip_slab, szn_stream_t stream);
int szn_conv2d_wgrad_cb_region(const szn_conv_desc_t* d, int region[8]);

/* ---- upscore: ConvTranspose2d(E,E,64,stride 32,bias=False) with the fixed bilinear kernel of
 * get_upsampling_weight (models.py:11-24,94,146) fused with the crop [19:19+H] (models.py:147).
 * coarse is NHWC f32 [B][h][w] with pixel stride ldc, channels [c0, c0+E); score is NCHW f32.     */
int szn_bilinear_up32_crop_fwd(int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop,
                               const float* coarse, float* score_nchw, szn_stream_t stream);
/* dcoarse[b][i][j][c0+c] = sum_{y,x} dscore[b][c][y][x] * filt[y+crop-32i][x+crop-32j]            */
int szn_bilinear_up32_crop_bwd(int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop,
                               const float* dscore_nchw, float* dcoarse, szn_stream_t stream);

/* ---- the same fixed bilinear ConvTranspose2d(E,E,2*stride,stride) + crop for stride 32 (== the two entries above) and
 * stride 8: the last stage of the FCN8s skip head (BASELINE north_star / SURVEY N1: public pytorch-fcn FCN8s, `upscore8`
 * ConvTranspose2d(E,E,16,stride 8) + crop 31; NOT in /root/reference -- parity unpinned).                              */
int szn_bilinear_up_crop_fwd(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop,
                             const float* coarse, float* score_nchw, szn_stream_t stream);
int szn_bilinear_up_crop_bwd(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop,
                             const float* dscore_nchw, float* dcoarse, szn_stream_t stream);
/* FCN8s `upscore2` / `upscore_pool4`: fixed bilinear ConvTranspose2d(C,C,4,stride 2) between NHWC f32 maps with pixel stride ld:
 * in [B][h][w][ld] -> out [B][2h+2][2w+2][ld], channels [0,C); bwd is its transpose (dout -> din).                         */
int szn_bilinear_up2_nhwc_fwd(int B, int h, int w, int C, int ld, const float* in, float* out, szn_stream_t stream);
int szn_bilinear_up2_nhwc_bwd(int B, int h, int w, int C, int ld, const float* dout, float* din, szn_stream_t stream);

/* ---- seenmask_upscore: ConvTranspose2d(C,C,64,stride 32,bias=False) with a LEARNED dense kernel
 * (models.py:98,150-151; trained in phase 2, train.py:170-175).  weight is torch layout
 * (Cin,Cout,64,64) f32; C <= 4.                                                                   */
int szn_deconv64s32_fwd(int B, int h, int w, int C, int ldc, int c0, int H, int W, int crop,
                        const float* coarse, const float* weight, float* out_nchw,
                        szn_stream_t stream);
int szn_deconv64s32_dgrad(int B, int h, int w, int C, int ldc, int c0, int H, int W, int crop,
                          const float* dout_nchw, const float* weight, float* dcoarse,
                          szn_stream_t stream);
int szn_deconv64s32_wgrad(int B, int h, int w, int C, int ldc, int c0, int H, int W, int crop,
                          const float* coarse, const float* dout_nchw, float* dweight,
                          int accumulate, szn_stream_t stream);

/* ---- phase 2 (BASELINE configs[2]): the seen-mask head fused from the 1/32 map -------------------------
 * Equivalent to szn_deconv64s32_fwd -> [target = np.in1d(label, seen), trainer_seenmask.py:55-56] -> szn_ce2d_fwd
 * (size_average) -> channel argmax (trainer_seenmask.py:67) -> szn_ce2d_bwd -> szn_deconv64s32_dgrad / _wgrad
 * (models.py:150-151, utils.py:19-48) without the (B,2,H,W) score or its gradient in HBM.  coarse: NHWC f32
 * [B][h][w] with pixel stride ldc, the two seen-mask channels at [c0, c0+2); weight: seenmask_upscore.weight
 * (2,2,64,64) f32.  Binary target of a pixel: n_class > 0: (0 <= label < n_class and bit `label` of seen_bits) ? 1 : 0
 * -- unlabelled pixels (-1) become 0 and COUNT, like the reference; labels below -1 mark batch padding (datasets.pad_collate
 * writes -2 where a smaller image of a ragged batch was extended: no counterpart in the reference, which trains at batch size 1)
 * and are ignored like cross_entropy2d ignores negative targets; n_class == 0: `target` already holds {0,1}
 * (anything else is ignored, cross_entropy2d's mask).  Outputs: loss[1]; stats[2] = {sum of terms, valid pixels}
 * (may be NULL); conf[4] int64 += confusion counts [target][prediction] (may be NULL; the running train metrics,
 * trainer_seenmask.py:87); pred int64 (B,H,W) (may be NULL); dscore2 f32 [B*h*w][2] = d loss / d coarse (compact) and
 * dweight (2,2,64,64) = d loss / d weight -- both NULL for a forward-only call.  target and loss both NULL: a pred-only call
 * (the seen-mask group of szn_fused_head_grouped; stats, conf, dscore2, dweight NULL, pred not).  Bit-reproducible (fixed-order
 * slabs, no atomics).  workspace: szn_seenmask_head_workspace_bytes.                                               */
size_t szn_seenmask_head_workspace_bytes(int B, int h, int w, int H, int W, int crop);
int szn_seenmask_head(int B, int h, int w, int ldc, int c0, int H, int W, int crop, const float* coarse,
                      const float* weight, const int64_t* target, int n_class, uint64_t seen_bits, float* loss,
                      float* stats, int64_t* conf, int64_t* pred, float* dscore2, float* dweight, void* workspace,
                      szn_stream_t stream);
/* the same with n_class <= SZN_MAX_CLASSES and the seen classes as a szn_class_set */
int szn_seenmask_head_k(int B, int h, int w, int ldc, int c0, int H, int W, int crop, const float* coarse,
                        const float* weight, const int64_t* target, int n_class, const szn_class_set* seen, float* loss,
                        float* stats, int64_t* conf, int64_t* pred, float* dscore2, float* dweight, void* workspace,
                        szn_stream_t stream);
/* szn_seenmask_margin: the pred-only call with the decision left open.  margin (B,H,W) f32 = s1 - s0 per pixel, where s0 and s1 are the
 * two seen-mask scores from exactly the chain szn_seenmask_head_k runs (ci outer, then di, then dj, one fmaf per tap and channel, cells
 * outside the map contribute exact zeros) and the difference is one fp32 subtraction with denormals kept: margin > 0 exactly where that
 * head's pred is 1 (s1 > s0), a tie or a NaN gives "not seen" in both.  The caller thresholds it (szn_seen_sweep_head); 4 B per pixel,
 * half of the int64 group map.  coarse, weight, ldc, c0, crop: szn_seenmask_head_k's.  No workspace.  szn_last_kernel():
 * smh_margin_kernel.  SZN_ERR_ARG, before any launch: a size below 1, a negative crop, a NULL pointer, an output (+ crop) that does not
 * fit the map at stride 32 (szn_seenmask_head_k's checks).                                                                          */
int szn_seenmask_margin(int B, int h, int w, int ldc, int c0, int H, int W, int crop,
                        const float* coarse, const float* weight, float* margin, szn_stream_t stream);
/* seenmask_score = Conv2d(4096, 2, 1) (models.py:97,149) backward from the compact gradient above:
 * dw[c][k] = sum_m dscore2[m][c] * feat[m][k], db[c] = sum_m dscore2[m][c]; feat [M][ldf] of `dtype` (relu7 after
 * Dropout2d), F a multiple of 8.  Fixed-order slabs in `workspace` (szn_seenmask_score_wgrad_workspace_bytes).     */
size_t szn_seenmask_score_wgrad_workspace_bytes(long M, int F);
int szn_seenmask_score_wgrad(int dtype, long M, int F, int ldf, const void* feat, const float* dscore2, float* dw,
                             float* db, void* workspace, szn_stream_t stream);

/* ---- losses (utils.py) --------------------------------------------------------------------------
 * score (B,E,H,W) NCHW f32; target (B,H,W) int64, <0 = ignore.  The target embedding of a pixel is
 * either gathered from embed[K][E] by label (target_embed == NULL; ignore pixels use row 0 exactly
 * like context_dataset.py:128-141) or read from target_embed (B,E,H,W) NCHW f32.
 * Batched definition (the reference is n = 1 only): per-image loss, mean over images.
 * stats: f32 [B][2] = {sum over valid px of the per-pixel term, number of valid px};
 * loss: f32 [1].  workspace: szn_loss_workspace_bytes(B,H,W).                                       */
size_t szn_loss_workspace_bytes(int B, int H, int W);
/* utils.py:75-102  loss_b = (N_b - sum cos) / N_b                                                  */
int szn_cosine_loss_fwd(int B, int E, int H, int W, int K, const float* score,
                        const int64_t* target, const float* embed, const float* target_embed,
                        float* loss, float* stats, void* workspace, szn_stream_t stream);
/* dscore = gout * dloss/dscore  (gout: device scalar, NULL = 1)                                    */
int szn_cosine_loss_bwd(int B, int E, int H, int W, int K, const float* score,
                        const int64_t* target, const float* embed, const float* target_embed,
                        const float* stats, const float* gout, float* dscore, szn_stream_t stream);
/* utils.py:50-73  loss_b = sum_{valid px, c} (s - t)^2 / N_b                                       */
int szn_mse_loss_fwd(int B, int E, int H, int W, int K, const float* score, const int64_t* target,
                     const float* embed, const float* target_embed, float* loss, float* stats,
                     void* workspace, szn_stream_t stream);
int szn_mse_loss_bwd(int B, int E, int H, int W, int K, const float* score, const int64_t* target,
                     const float* embed, const float* target_embed, const float* stats,
                     const float* gout, float* dscore, szn_stream_t stream);
/* utils.py:19-48  cross_entropy2d: sum over ALL valid pixels of the batch of -weight[target] * log_softmax[target]
 * (weight: optional f32 [C] class weights, NULL = 1; F.nll_loss(weight=, size_average=False), utils.py:46);
 * size_average divides by the NUMBER of valid pixels (utils.py:47-48, not by the weight sum).  pred (may be NULL) receives
 * the channel argmax (score.data.max(1)[1], trainer_fcn.py:117 / trainer_seenmask.py:67) as int64 (B,H,W).           */
int szn_ce2d_fwd(int B, int C, int H, int W, const float* score, const int64_t* target, const float* weight,
                 int size_average, float* loss, float* stats, int64_t* pred, void* workspace, szn_stream_t stream);
int szn_ce2d_bwd(int B, int C, int H, int W, const float* score, const int64_t* target, const float* weight,
                 int size_average, const float* stats, const float* gout, float* dscore, szn_stream_t stream);

/* ---- nearest-class-embedding inference (utils.py:159-205) --------------------------------------
 * sim[k] = (score_px . embed[k]) / (||score_px|| * (||embed[k]|| == 0 ? 1 : ||embed[k]||)),
 * pred = first argmax_k.  embed[K][E] f32.  K <= 64 through the uint64_t entry points below, K <= SZN_MAX_CLASSES (256)
 * through the _k forms, which take class sets as szn_class_set (the reference's unseen lists are plain Python lists of any
 * length, trainer_fcn.py:56-64; 64 classes cover its two datasets -- 21 and 33/59 classes -- but not a 150-class label set).
 * mode 0 (infer_lbl):    all K rows of embed compete.
 * mode 1 (stich_seen_unseen_with_mask / infer_lbl_szn / infer_lbl_forced_unseen):
 *        rows with bit k of unseen_bits set form the "unseen-only" matrix, the others the
 *        "seen-only" matrix (the other group's rows zeroed, trainer_fcn.py:56-64, which score
 *        exactly 0 and still compete); a pixel takes the unseen-only prediction when
 *          - seenmask != NULL: argmax over the 2 channels of seenmask (B,2,H,W) is 0
 *            (utils.py:197-198), or
 *          - seenmask == NULL: its target label is an unseen class (utils.py:190-191).
 * pred: int64 (B,H,W).                                                                             */
int szn_embed_argmax(int B, int E, int H, int W, int K, const float* score, const float* embed,
                     int mode, uint64_t unseen_bits, const float* seenmask, const int64_t* target,
                     int64_t* pred, szn_stream_t stream);
int szn_embed_argmax_k(int B, int E, int H, int W, int K, const float* score, const float* embed,
                       int mode, const szn_class_set* unseen, const float* seenmask, const int64_t* target,
                       int64_t* pred, szn_stream_t stream);

/* ---- confusion histogram (utils.py:104-154) ------------------------------------------------------
 * hist[3][K][K] int64 += bincount(K*gt+pred) over pixels with 0 <= gt < K, for {all, gt in seen,
 * gt in unseen}; unseen_bits == 0 fills only hist[0].                                              */
int szn_confusion_hist(long npix, int K, const int64_t* label_true, const int64_t* label_pred,
                       uint64_t unseen_bits, int64_t* hist, szn_stream_t stream);
/* K <= SZN_MAX_CLASSES; an empty or NULL set fills only hist[0] */
int szn_confusion_hist_k(long npix, int K, const int64_t* label_true, const int64_t* label_pred,
                         const szn_class_set* unseen, int64_t* hist, szn_stream_t stream);

/* ---- fused head: coarse -> (loss, prediction, dcoarse) without materialising (B,E,H,W) ----------
 * Equivalent to szn_bilinear_up32_crop_fwd -> szn_cosine_loss_fwd -> szn_embed_argmax ->
 * szn_cosine_loss_bwd -> szn_bilinear_up32_crop_bwd (models.py:146-147 + utils.py:75-102,159-185)
 * evaluated algebraically per 32x32 cell.  pred / dcoarse may be NULL.  dcoarse is written in
 * `dcoarse_dtype` with pixel stride ldc (channels [c0,c0+E) only).                                 */
size_t szn_fused_head_workspace_bytes(int B, int h, int w, int E, int K);
int szn_fused_head(int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                   const float* coarse, const float* embed, const int64_t* target,
                   float* loss, float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse,
                   void* workspace, szn_stream_t stream);
/* the same head over stride-8 cells (coarse = the 1/8 fused map of the FCN8s skip head, crop 31); stride in {32, 8};
 * szn_fused_head == stride 32.  The workspace size is szn_fused_head_workspace_bytes of the map's own h, w.            */
int szn_fused_head_strided(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                           const float* coarse, const float* embed, const int64_t* target, float* loss, float* stats,
                           int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream);
/* The class embeddings are constants of a run (trainer_fcn.py:49-62): szn_fused_head_prepare writes their transpose and norms to the head of
 * `workspace` once, szn_fused_head_prepared is szn_fused_head_strided without that launch (23 us of dependent loads per step) for a caller
 * that keeps the workspace and prepares again whenever the embeddings or the workspace change.  Same results bit for bit. */
int szn_fused_head_prepare(int E, int K, const float* embed, void* workspace, szn_stream_t stream);
int szn_fused_head_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                            const float* coarse, const float* embed, const int64_t* target, float* loss, float* stats,
                            int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream);
/* The same head with the class assignment of the full SZN network (train.py -m test_all, trainer_fcn.py:123-147) or of forced-unseen
 * runs (trainer_fcn.py:110-112): the prediction of szn_embed_argmax_k mode 1 (utils.py:188-204) without the (B,E,H,W) score.  A pixel
 * competes among its group's classes; every class outside the group scores 0 / (||s|| * 1) -- the zeroed row of the seen-only /
 * unseen-only matrix (trainer_fcn.py:56-64), which still competes (a zero-norm pixel gives NaN and class 0) -- first index on ties.
 * A pixel takes the unseen group (classes in `unseen`, NULL = the empty set) when
 *   group_mode 1: group_map[pix] == 0 -- group_map int64 (B,H,W) = the seen-mask prediction (szn_seenmask_head's pred: s1 > s0),
 *   group_mode 2: target[pix] is in `unseen` (np.in1d(target, unseen)); negative labels (-1, padding -2) take the seen group.
 * group_mode 0 is szn_fused_head_strided bit for bit.  Loss, stats and dcoarse do not depend on the group: they are those of the
 * full matrix, bit for bit.  NULL rules as szn_fused_head_strided, and: modes 1 and 2 need pred; mode 1 needs group_map, mode 2
 * target (so also loss and stats); a class in `unseen` >= K is an error.  _prepared: the workspace holds szn_fused_head_prepare. */
int szn_fused_head_grouped(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                           const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                           int group_mode, const int64_t* group_map, float* loss, float* stats, int64_t* pred,
                           int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream);
int szn_fused_head_grouped_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                    const float* coarse, const float* embed, const int64_t* target,
                                    const szn_class_set* unseen, int group_mode, const int64_t* group_map, float* loss,
                                    float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace,
                                    szn_stream_t stream);

/* ---- fused MSE embedding head (train.py -loss mse): coarse -> (loss, stats, prediction, dcoarse) without the (B,E,H,W) score -----
 * Equivalent to szn_bilinear_up_crop_fwd(stride) -> szn_mse_loss_fwd (embedding gather) -> szn_embed_argmax_k ->
 * szn_mse_loss_bwd (gout NULL) -> szn_bilinear_up_crop_bwd(stride) (models.py:146-147 upscore + crop; utils.py:50-73 mse_loss as
 * trainer_fcn.py forward / forward_szn call it; utils.py:159-204 infer_lbl).  Arguments, strides (32 | 8), group modes, NULL rules
 * (pred-only, loss-only, no dcoarse), error codes, workspace (szn_fused_head_workspace_bytes) and prepare step
 * (szn_fused_head_prepare for _prepared) are those of szn_fused_head_grouped[_prepared].  pred is that head's pred bit for bit: the
 * class assignment is the cosine argmax whatever the loss.  stats f32 [B][2] = {sum over valid px of |s - e_lbl|^2, number of valid
 * px}; loss = mean_b S_b / N_b (labels >= K take row 0, negative labels are ignored: szn_mse_loss_fwd's contract); dcoarse =
 * 2 (s - e_lbl) / (B N_b) carried back through the upsample, channels [c0, c0+E) only.  The per-pixel term is the quadratic form
 * sum_{t,u} w_t w_u (C_t - e).(C_u - e) over the cell's four taps, never |s|^2 - 2 s.e + |e|^2 (which cancels near convergence).
 * Fixed-order reductions, no atomics: two calls give bitwise-equal outputs.                                                        */
int szn_fused_mse_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                       const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                       int group_mode, const int64_t* group_map, float* loss, float* stats, int64_t* pred,
                       int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream);
int szn_fused_mse_head_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                const float* coarse, const float* embed, const int64_t* target,
                                const szn_class_set* unseen, int group_mode, const int64_t* group_map, float* loss,
                                float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace,
                                szn_stream_t stream);

/* ---- fused similarity cross-entropy head (train.py -loss sim_ce): a softmax over the seen classes' cosines, without the score --------
 * Equivalent to szn_bilinear_up_crop_fwd(stride) -> utils.sim_ce_loss (forward and autograd backward) -> szn_embed_argmax_k ->
 * szn_bilinear_up_crop_bwd(stride).  Arguments, strides (32 | 8), group modes, NULL rules (pred-only, loss-only, no dcoarse), error
 * codes, workspace (szn_fused_head_workspace_bytes) and prepare step (szn_fused_head_prepare for _prepared) are those of
 * szn_fused_mse_head[_prepared]; pred is szn_fused_head_grouped's pred bit for bit (the class assignment is the cosine argmax whatever
 * the loss).  For a pixel with upsampled score s (fp32 arithmetic):
 *   cos_k = s.e_k / (|s| n_k), n_k = |e_k| (1 where |e_k| = 0);  S = the classes of [0, K) not in `exclude` (NULL: all K compete);
 *   z_k = cos_k / temperature for k in S;  term = logsumexp_{k in S} z_k - z_label (the maximum subtracted first).
 * A pixel counts when 0 <= label < K and label is in S: -1, -2 (padding), labels >= K and labels in `exclude` are ignored (the CE head's
 * rule for labels >= K, not the cosine head's row 0).  stats f32 [B][2] = {sum of terms, number of counted px}; loss = mean_b S_b / N_b.
 * dcoarse = d loss / d coarse with, p = softmax_S(z) (0 outside S) and y = onehot(label),
 *   d term / d s = (1 / temperature) sum_k (p_k - y_k) (e_k / (|s| n_k) - cos_k s / |s|^2),
 * scaled by 1 / (B N_b) and carried back through the upsample, channels [c0, c0+E) only, in dcoarse_dtype.  A pred-only call
 * (target NULL) evaluates no softmax.  Errors, all before any launch: temperature <= 0 or not finite, a class in `exclude` >= K, and an
 * `exclude` that leaves no class competing are SZN_ERR_ARG.  Fixed-order reductions, no atomics: two calls give bitwise-equal outputs. */
int szn_fused_simce_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                         const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                         int group_mode, const int64_t* group_map, const szn_class_set* exclude, float temperature,
                         float* loss, float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace,
                         szn_stream_t stream);
int szn_fused_simce_head_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                  const float* coarse, const float* embed, const int64_t* target,
                                  const szn_class_set* unseen, int group_mode, const int64_t* group_map,
                                  const szn_class_set* exclude, float temperature, float* loss, float* stats, int64_t* pred,
                                  int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream);

/* ---- fused hinge ranking head (train.py -loss rank, DeViSE): the label's cosine against the other seen classes', without the score ----
 * Equivalent to szn_bilinear_up_crop_fwd(stride) -> utils.rank_loss (forward and autograd backward) -> szn_embed_argmax_k ->
 * szn_bilinear_up_crop_bwd(stride).  Arguments, strides (32 | 8), group modes, NULL rules (pred-only, loss-only, no dcoarse), error
 * codes, workspace (szn_fused_head_workspace_bytes) and prepare step (szn_fused_head_prepare for _prepared) are those of
 * szn_fused_mse_head[_prepared]; pred is szn_fused_head_grouped's pred bit for bit.  For a pixel with upsampled score s (fp32
 * arithmetic), cos_k and n_k as szn_fused_simce_head defines them (n_k = 1 where |e_k| = 0):
 *   S = the classes of [0, K) not in `exclude` (NULL: all K compete);  v_k = margin - cos_label + cos_k for k in S, k != label;
 *   hardest = 0 (sum of hinges):  term = sum_k max(0, v_k),  c_k = 1[v_k > 0];
 *   hardest = 1 (hardest negative):  k* = argmax_k v_k (the lowest index on an exact tie),  term = max(0, v_k*),  c_k* = 1[v_k* > 0],
 *   every other c_k = 0;   c_label = -sum_{k != label} c_k.
 * A pixel counts when 0 <= label < K and label is in S (sim_ce's rule): -1, -2, -3 (hidden), labels >= K and labels in `exclude` are
 * ignored.  stats f32 [B][2] = {sum of terms, number of counted px}; loss = mean_b S_b / N_b.  dcoarse = d loss / d coarse with
 *   d term / d s = sum_k c_k (e_k / (|s| n_k) - cos_k s / |s|^2)
 * (at v_k = 0 exactly the coefficient is 0: the hinge is flat there as far as this head is concerned), scaled by 1 / (B N_b) and carried back through the
 * upsample, channels [c0, c0+E) only, in dcoarse_dtype.  A pred-only call (target NULL) evaluates no hinge.  Errors, all before any
 * launch: margin < 0 or not finite, hardest not 0 | 1, a class in `exclude` >= K, and an `exclude` that leaves fewer than two classes
 * competing (the loss would be identically zero) are SZN_ERR_ARG.  Fixed-order reductions, no atomics: two calls give bitwise-equal
 * outputs.                                                                                                                             */
int szn_fused_rank_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                        const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                        int group_mode, const int64_t* group_map, const szn_class_set* exclude, float margin, int hardest,
                        float* loss, float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace,
                        szn_stream_t stream);
int szn_fused_rank_head_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                 const float* coarse, const float* embed, const int64_t* target,
                                 const szn_class_set* unseen, int group_mode, const int64_t* group_map,
                                 const szn_class_set* exclude, float margin, int hardest, float* loss, float* stats, int64_t* pred,
                                 int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream);

/* ---- fused sim_ce head with the unseen-bias term (train.py -loss sim_ce --bias-loss, QFSL): hidden pixels pull towards the unseen set --
 * Equivalent to szn_bilinear_up_crop_fwd(stride) -> utils.sim_ce_bias_loss (forward and autograd backward) -> szn_embed_argmax_k ->
 * szn_bilinear_up_crop_bwd(stride).  szn_fused_simce_head[_prepared]'s arguments, strides, group modes, NULL rules, error codes,
 * workspace, prepare step and dcoarse_dtype codes, with (bias_unseen, weight, hidden_label) after `temperature`; pred is
 * szn_fused_head_grouped's pred bit for bit.  cos_k, n_k, z_k = cos_k / temperature as szn_fused_simce_head defines them; X = `exclude`,
 * U = `bias_unseen` (non-empty, not all K classes; independent of the `unseen` of the group modes), lambda = `weight` > 0,
 * hl = `hidden_label` < -1 (datasets.HIDDEN_LABEL).
 *   A labelled pixel (0 <= label < K, label not in X): term = logsumexp_{k not in X} z_k - z_label, szn_fused_simce_head's term, its
 *   gradient and its bits.
 *   A hidden pixel (label == hl): the softmax runs over ALL K classes whatever X holds, p_k = softmax_k(z_k), and
 *     term = lambda * -log sum_{u in U} p_u = lambda * (logsumexp_{all k} z_k - logsumexp_{u in U} z_u),
 *   each log-sum-exp with its own maximum subtracted (m over all k, m_U over U), so the term and the gradient are finite where
 *   P_U = sum_U p_u itself underflows;  q_k = 1[k in U] exp(z_k - m_U) / sum_{u in U} exp(z_u - m_U)  (= p_k / P_U), and
 *     d term / d s = (lambda / temperature) sum_k (p_k - q_k) (e_k / (|s| n_k) - cos_k s / |s|^2).
 *   Every other pixel (-1, -2, other negative labels, labels >= K, labels in X) is ignored.
 * stats f32 [B][2] = {S_b = sum of all terms, N_b = labelled + hidden px}; loss = mean_b S_b / N_b: one joint mean per image, not
 * QFSL's separate means over labelled and unlabelled data.  dcoarse is scaled by 1 / (B N_b).  With no hidden pixel in `target` every
 * output is szn_fused_simce_head's bit for bit.  Errors, all before any launch (SZN_ERR_ARG): U empty or all K classes or naming a
 * class >= K, weight not finite or <= 0, hidden_label >= -1, and the temperature and `exclude` szn_fused_simce_head refuses.
 * Fixed-order reductions, no atomics: two calls give bitwise-equal outputs. */
int szn_fused_simce_bias_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                              const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                              int group_mode, const int64_t* group_map, const szn_class_set* exclude, float temperature,
                              const szn_class_set* bias_unseen, float weight, int64_t hidden_label, float* loss, float* stats,
                              int64_t* pred, int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream);
int szn_fused_simce_bias_head_prepared(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                                       const float* coarse, const float* embed, const int64_t* target,
                                       const szn_class_set* unseen, int group_mode, const int64_t* group_map,
                                       const szn_class_set* exclude, float temperature, const szn_class_set* bias_unseen,
                                       float weight, int64_t hidden_label, float* loss, float* stats, int64_t* pred,
                                       int dcoarse_dtype, void* dcoarse, void* workspace, szn_stream_t stream);

/* ---- fused softmax cross-entropy head: coarse -> (loss, stats, prediction, dcoarse) without the (B,C,H,W) score ---------
 * Equivalent to szn_bilinear_up_crop_fwd(stride) -> szn_ce2d_fwd (pred = channel argmax) -> szn_ce2d_bwd (gout NULL) ->
 * szn_bilinear_up_crop_bwd(stride) (models.py:94,146-147 upscore + crop, utils.py:19-48 cross_entropy2d, trainer_fcn.py:117
 * score.max(1)[1]).  stride 32: FCN32s' upscore (crop 19); stride 8: the FCN8s upscore8 stage (crop 31).  coarse: NHWC f32
 * [B][h][w] with pixel stride ldc, the C class channels at [c0, c0+C); 1 <= C <= SZN_MAX_CLASSES.
 * Bit identity (-ffp-contract=off): a pixel's logits are those of the materialised score element (bilinear weights formed as
 * double products rounded to float, fmaf chain over taps (I-1,J-1), (I-1,J), (I,J-1), (I,J)); max, first-index argmax, sum of
 * exps, logf, the per-pixel term and the class-weight product are ce_fwd_kernel's operations in its order, so pred and every
 * per-pixel term equal the chain's bit for bit.  The per-pixel gradient is ce_bwd_kernel's g * (softmax_c - [c == label]).
 * Labels: a pixel counts when 0 <= label < C; -1 (unlabelled), -2 (batch padding) and labels >= C are ignored.  Every pixel
 * gets a prediction.  weight: optional f32 [C] class weights (NULL = 1).  loss[1]: the sum of the terms, or the sum divided by
 * the number of valid pixels of the batch (size_average); stats f32 [B][2] = {sum of terms, valid pixels} (may be NULL).
 * pred int64 (B,H,W) (may be NULL).  dcoarse (may be NULL): d loss / d coarse in dcoarse_dtype (SZN_F32 | SZN_BF16 | SZN_F16),
 * written to channels [c0, c0+C) of pixel stride ldc only -- padding channels are left untouched.  target and loss both NULL:
 * a pred-only call (stats and dcoarse NULL, pred not).  Reductions: loss partials in double per pixel cell, fixed-order
 * finalize; dcoarse is the per-cell table A[t][c] = sum_px w_t * d_c gathered over the <= 4 cells that use each coarse
 * position -- no atomics, two calls give bitwise-equal outputs.  Bad arguments return SZN_ERR_ARG (geometry, NULL rules, crop
 * window larger than the deconv output) or SZN_ERR_UNSUPPORTED (stride not 32 or 8, C > SZN_MAX_CLASSES) before any launch.
 * workspace: szn_fused_ce_head_workspace_bytes of the map's own stride, B, h, w, C.                                      */
size_t szn_fused_ce_head_workspace_bytes(int stride, int B, int h, int w, int C);
int szn_fused_ce_head(int stride, int B, int h, int w, int C, int ldc, int c0, int H, int W, int crop,
                      const float* coarse, const int64_t* target, const float* weight, int size_average,
                      float* loss, float* stats, int64_t* pred, int dcoarse_dtype, void* dcoarse,
                      void* workspace, szn_stream_t stream);

/* ---- optimizers (train.py:126-133,174-175; torch.optim.Adam / SGD semantics) ----------------------
 * One launch per flat fp32 parameter buffer.  grad_scale multiplies the gradient first (1/world
 * after a sum all-reduce; 1/(world * loss_scale) on the fp16 path).  If w_lp != NULL the updated weight is
 * also written as a 16-bit image of type w_lp_dtype (SZN_BF16 | SZN_F16) for the next forward pass.    */
int szn_adam_step(long n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                  float grad_scale, void* w_lp, int w_lp_dtype, szn_stream_t stream);
int szn_sgd_momentum_step(long n, float* param, const float* grad, float* momentum_buf, float lr,
                          float momentum, float weight_decay, int first_step, float grad_scale,
                          void* w_lp, int w_lp_dtype, szn_stream_t stream);
/* The same steps reading the gradient as a 16-bit image (grad_dtype = SZN_BF16 | SZN_F16) -- the summed wire buffer of the
 * data-parallel exchange (szn_conv_desc_t.dw_lp -> all-reduce / reduce-scatter in place -> here): the widening copy back into an
 * fp32 gradient buffer disappears and the pass reads 2 B per weight instead of 4.  Arithmetic after widening: identical.   */
int szn_adam_step_g16(long n, float* param, const void* grad, int grad_dtype, float* exp_avg, float* exp_avg_sq,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                      float grad_scale, void* w_lp, int w_lp_dtype, szn_stream_t stream);
int szn_sgd_momentum_step_g16(long n, float* param, const void* grad, int grad_dtype, float* momentum_buf, float lr,
                              float momentum, float weight_decay, int first_step, float grad_scale,
                              void* w_lp, int w_lp_dtype, szn_stream_t stream);

/* ---- dynamic loss scaling for the IEEE-half path (BASELINE configs[4]: "fp16 activations"; the reference is fp32 and has
 * no counterpart).  scale_state: device float[4] = {loss scale S, found_inf flag, optimizer steps applied, clean steps
 * since S last changed}.  Per step: d(loss)/d(coarse) is multiplied by S in fp32 before it enters the 16-bit backward pass;
 * szn_grad_check_finite (after the gradient all-reduce, so every rank sees the same flag: inf / NaN survive a sum) raises
 * found_inf if any gradient element is not finite; the *_scaled optimizer entry points read S, the flag and the step count
 * from scale_state: they divide the gradient by S and do NOTHING when the flag is set (masters, moments and the 16-bit
 * weight image stay as they were); szn_loss_scale_update then backs S off (x backoff, >= min_scale) after an overflow,
 * or counts the step and grows S (x growth, <= max_scale) after growth_interval clean steps, and clears the flag.
 * No host synchronisation anywhere: the scale never leaves the device.                                                  */
int szn_grad_check_finite(long n, const float* grad, float* scale_state, szn_stream_t stream);
int szn_adam_step_scaled(long n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                         float beta2, float eps, float weight_decay, const float* scale_state, float grad_scale,
                         void* w_lp, int w_lp_dtype, szn_stream_t stream);
int szn_sgd_momentum_step_scaled(long n, float* param, const float* grad, float* momentum_buf, float lr, float momentum,
                                 float weight_decay, const float* scale_state, float grad_scale, void* w_lp,
                                 int w_lp_dtype, szn_stream_t stream);
int szn_loss_scale_update(float* scale_state, float growth, float backoff, int growth_interval, float min_scale,
                          float max_scale, szn_stream_t stream);

/* ---- averaged weights (exponential moving average of the parameters, Polyak averaging; the reference has no counterpart) ----
 * One step of the average over n fp32 elements:   avg = fmaf(D, avg - param, param)   =   param + D * (avg - param),
 *     D = pow(min(decay, (1 + s) / (10 + s)), every)     (computed in double, rounded to float once)
 * with s = the optimizer steps applied BEFORE this one: step - 1 from the host when scale_state == NULL, scale_state[2] otherwise
 * (as the *_scaled optimizer entries take their step count).  The (1 + s) / (10 + s) ramp is the usual warm-up; step == 0 switches
 * it off (D = decay^every).  `every` = the optimizer steps this one update stands for (the caller launches it every `every`-th
 * step).  With scale_state != NULL and its found_inf flag set the kernel does nothing -- the optimizer entries skipped the same
 * step -- so launch it before szn_loss_scale_update clears the flag.  Exact corners: D == 1 leaves avg untouched, D == 0 makes
 * avg a bitwise copy of param, avg == param is a fixed point.  Any 4-byte-aligned pointer pair is taken (16-byte accesses where
 * both pointers allow them).  decay outside [0, 1], every < 1, step < 0, n < 0 or a NULL buffer with n > 0: SZN_ERR_ARG; n == 0 is
 * a successful no-op.  szn_last_kernel: "ema_kernel".                                                                          */
int szn_ema_step(long n, float* avg, const float* param, float decay, int every, int step, const float* scale_state,
                 szn_stream_t stream);
/* Exchange the contents of two non-overlapping fp32 buffers as 32-bit words (NaN payloads and -0 survive).  Overlapping ranges:
 * SZN_ERR_ARG, nothing is written.  szn_last_kernel: "swap_kernel".                                                             */
int szn_swap_f32(long n, float* a, float* b, szn_stream_t stream);

/* ---- gradient accumulation (torch's backward() without zero_grad(); the reference steps after every backward) ----
 * The running sum of a flat fp32 gradient buffer over a window of micro-steps, one IEEE addition per element and nothing else:
 *     SZN_ACCUM_SET    acc[i] = grad[i]                               the first micro-step of a window    ( 8 B / element)
 *     SZN_ACCUM_ADD    acc[i] = acc[i] + grad[i]                      the ones in between                 (12 B / element)
 *     SZN_ACCUM_FINAL  grad[i] = acc[i] + grad[i], acc is only read   the last one                        (12 B / element)
 * so that after SET, ADD, ..., FINAL grad holds ((g1 + g2) + g3) + ... + gA, left to right, in the buffer every consumer of the
 * gradient already reads (the exchange, szn_grad_check_finite, szn_grad_stats, the optimizer entries).  inf / NaN survive the sum.
 * No atomics and no reduction: two calls give the same bits.  Any 4-byte-aligned pointer pair is taken (16-byte accesses where both
 * pointers allow them).  SZN_ERR_ARG, nothing launched: n < 0, mode outside 0..2, a NULL buffer with n > 0, a pointer not 4-byte
 * aligned, overlapping ranges.  n == 0 is a successful no-op.  szn_last_kernel: "grad_accum_kernel".                             */
#define SZN_ACCUM_SET   0
#define SZN_ACCUM_ADD   1
#define SZN_ACCUM_FINAL 2
int szn_grad_accum(long n, float* acc, float* grad, int mode, szn_stream_t stream);

/* ---- gradient statistics and gradient-norm clipping (torch.nn.utils.clip_grad_norm_'s rule; the reference does not clip, it
 * prints score_fr's gradient sum: trainer_fcn.py:160-162) ----
 * szn_grad_stats: per segment s = elements [seg_end[s-1], seg_end[s]) of one flat buffer (fp32, or a 16-bit image: the summed wire
 * buffer of the exchange), stats[s] = {sum g, sum g*g}.  seg_end is a HOST array read during the call (ascending, seg_end[n_seg-1]
 * == n); the table travels by value in the kernel arguments -- hence at most SZN_GRAD_STATS_MAX_SEGS segments -- so nothing is
 * copied to the device and the call can be captured.  Segments start at any element offset; an empty one gives {0, 0}; rows of
 * stats are overwritten; grad is only read.  Arithmetic: every element is widened to double first, so g*g is exact for all three
 * input types and the additions in double are the only roundings.  Their order is fixed: a segment is cut into chunks of 16384
 * elements from its own start; one block reduces a chunk (grad_stats_chunk_kernel: per lane its vectors in ascending order, the
 * wave by halving shuffles, the four waves through LDS in ascending order) and writes its pair to the workspace; a second kernel
 * (grad_stats_sum_kernel, one wave per segment) adds the segment's chunk pairs: 64 contiguous runs, each in ascending chunk order,
 * then the 64 run sums in ascending order.  No atomics: two calls give the same bits.  A non-finite element makes its segment's
 * sum of squares non-finite.  Any pointer aligned to its element size is taken (16-byte loads -- 8-byte for 16-bit input -- on the
 * aligned body of each chunk, scalar loads for the <= 3 elements in front and behind).  SZN_ERR_ARG before any launch: n < 0,
 * n_seg outside [1, SZN_GRAD_STATS_MAX_SEGS], seg_end not ascending or not ending at n, NULL seg_end / stats, NULL grad /
 * workspace with n > 0, a dtype other than SZN_F32 | SZN_BF16 | SZN_F16, grad not aligned to its element size, stats / workspace
 * not 8-byte aligned.  n == 0 writes zeros.  workspace: szn_grad_stats_workspace_bytes(n, n_seg).
 * szn_last_kernel(): grad_stats_sum_kernel; szn_prev_kernel(): grad_stats_chunk_kernel.                                        */
#define SZN_GRAD_STATS_MAX_SEGS 64
size_t szn_grad_stats_workspace_bytes(long n, int n_seg);
int szn_grad_stats(long n, const void* grad, int grad_dtype, int n_seg, const int64_t* seg_end, double* stats, void* workspace,
                   szn_stream_t stream);
/* The step's decision from the statistics of all its buffers (stats: device [n_seg][2], any n_seg >= 1), one tiny launch:
 *     total = sum_s stats[s][1] (ascending, double);  S = scale_state ? scale_state[0] : 1;  norm = sqrt(total) * grad_scale / S
 * total not finite (an element was inf / NaN: finite fp32 squares cannot overflow a double): clip_state = {1, (float)norm, -, -}
 * with both counters untouched and, if scale_state is given, scale_state[1] = 1 -- the found_inf flag szn_grad_check_finite would
 * have raised.  Otherwise coef = norm + 1e-6 > max_norm ? (float)(max_norm / (norm + 1e-6)) : 1 and
 *     clip_state = {coef, (float)norm, steps clipped + (coef < 1), steps seen + 1}       (device float[4])
 * max_norm = +inf measures only (coef is exactly 1).  SZN_ERR_ARG: max_norm NaN or <= 0, n_seg < 1, NULL stats / clip_state.
 * szn_last_kernel(): clip_coef_kernel.                                                                                          */
int szn_clip_coef(int n_seg, const double* stats, float max_norm, float grad_scale, float* scale_state, float* clip_state,
                  szn_stream_t stream);
/* The optimizer steps under clipping: supersets of szn_*_step, _g16 and _scaled.  The only new arithmetic is one fp32 multiply in
 * the kernel preamble: the effective gradient scale is grad_scale * clip_state[0], or (grad_scale / scale_state[0]) *
 * clip_state[0] with scale_state; the per-element chain is unchanged, so clip_state[0] == 1 reproduces the matching entry above
 * bit for bit.  With scale_state the step count / first_step flag and the skip come from it as in the _scaled entries (step /
 * first_step are ignored).  SZN_ERR_ARG: NULL clip_state, a 16-bit grad_dtype together with scale_state, and what the entries
 * above refuse.                                                                                                                  */
int szn_adam_step_clipped(long n, float* param, const void* grad, int grad_dtype, float* exp_avg, float* exp_avg_sq, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                          const float* scale_state, const float* clip_state, void* w_lp, int w_lp_dtype, szn_stream_t stream);
int szn_sgd_momentum_step_clipped(long n, float* param, const void* grad, int grad_dtype, float* momentum_buf, float lr,
                                  float momentum, float weight_decay, int first_step, float grad_scale,
                                  const float* scale_state, const float* clip_state, void* w_lp, int w_lp_dtype,
                                  szn_stream_t stream);

/* ---- row / column remapping of an NHWC map (the constant band of the pad-100 network inside the conv3 block) --------------
 * models.py:43 pads conv1_1 by 100: at 1/4 resolution most rows / columns between the tensor edge and the image's reach hold one
 * value per channel, and conv3_1 .. conv3_3 (models.py:56-62,123-128) need not compute them.  One kernel does the four index maps
 * the caller needs (crop, put the pooled rows back, and their two backward forms):
 *     out[b][y][x][c] = sum over sy in [ytab[2y], ytab[2y] + ytab[2y+1]), sx in [xtab[2x], xtab[2x] + xtab[2x+1]) of in[b][sy][sx][c]
 * (count 0 = zeros; fp32 accumulation in ascending order; a single source is moved bit for bit).  in [B][Hi][Wi][C], out
 * [B][Ho][Wo][C] dense, 16-B aligned, C a multiple of 8 (16-bit) / 4 (f32); ytab [Ho][2], xtab [Wo][2] int32 on the device.          */
int szn_band_remap(int dtype, int B, int Hi, int Wi, int Ho, int Wo, int C, const void* in, void* out, const int* ytab,
                   const int* xtab, szn_stream_t stream);
/* In place: every run {start, count} of `runs` (device int [n_runs][2]) summed (fp32, ascending) into its first row (axis 0) / column (axis 1) of
 * d [B][H][W][C].  The summing rows / columns of a transposed band map are few; folded first, the map is a one-source gather that
 * szn_maxpool2x2_ceil_bwd_code_gather applies while reading (rows, then columns = the two szn_band_remap passes, bit for bit). */
int szn_band_fold(int dtype, int B, int H, int W, int C, void* d, int axis, const int* runs, int n_runs, szn_stream_t stream);

/* ---- small utilities -------------------------------------------------------------------------------- */
int szn_cast(int src_dtype, int dst_dtype, long n, const void* src, void* dst, szn_stream_t stream);
/* Dropout2d factors: scale[i] = (u_i >= p) ? 1/(1-p) : 0 with a counter-based generator (seed, i)   */
int szn_dropout2d_mask(long n, float p, uint64_t seed, uint64_t offset, float* scale,
                       szn_stream_t stream);
/* fp8 pixel projection (BASELINE configs[4]: "fp8 MFMA projection GEMM"; score_fr || seenmask_score forward, models.py:
 * 93,97,145,149).  x [M][K] (x_dtype) and w [N][K] (w_dtype) are quantised to OCP e4m3 with per-tensor scales
 * amax/448 (round to nearest even), multiplied on the fp8 matrix cores with fp32 accumulation and rescaled:
 * out[m][n] = (sum_k xq wq) * sx * sw + bias[n], fp32, row stride ldo.  K must be a multiple of 128.  workspace:
 * szn_proj_fp8_workspace_bytes(M, K, N) bytes, 16-B aligned.                                                       */
size_t szn_proj_fp8_workspace_bytes(long M, int K, int N);
/* Backward of that layer on the fp8 matrix cores (the e4m3-forward / e5m2-gradient recipe; no reference counterpart):
 *   dgrad: dx[m][k] = epi( sum_n g[m][n] * w[n][k] ),  wgrad: dw[n][k] = sum_m g[m][n] * x[m][k]
 * g (the gradient wrt the projection output, row stride ldg) is quantised to OCP e5m2 with the per-tensor scale
 * amax / 57344, w [N][K] and x [M][ldx] to e4m3 (amax / 448); products exact in fp32, fp32 accumulation, one rescale.
 * dgrad epilogue like szn_conv2d_dgrad: optional gate (gate[m][k] > 0 ? v : 0; element type gate_dtype, row stride ldgate),
 * optional chan_scale[image][k] (image = m / rows_per_image), output element type out_dtype, row stride ldx.
 * dw is fp32 [N][K], dense.  workspace: szn_proj_fp8_bwd_workspace_bytes(M, K, N), 16-B aligned.                      */
size_t szn_proj_fp8_bwd_workspace_bytes(long M, int K, int N);
int szn_proj_fp8_dgrad(int g_dtype, int w_dtype, long M, int K, int N, int ldg, const void* g, const void* w,
                       const void* gate, int gate_dtype, int ldgate, const float* chan_scale, int rows_per_image,
                       int out_dtype, void* dx, int ldx, void* workspace, szn_stream_t stream);
int szn_proj_fp8_wgrad(int g_dtype, int x_dtype, long M, int K, int N, int ldg, int ldx, const void* g, const void* x,
                       float* dw, void* workspace, szn_stream_t stream);
int szn_proj_fp8_fwd(int x_dtype, int w_dtype, long M, int K, int N, int ldo, const void* x, const void* w,
                     const float* bias, float* out_f32, void* workspace, szn_stream_t stream);
/* Dataset transform on the device (context_dataset.py:143-150, pascal_dataset.py:138-145): RGB uint8 HWC image(s)
 * [B][H][W][3] -> BGR, minus mean_bgr (three doubles, BGR order), as the (B,3,H,W) f32 NCHW network input.  The
 * subtraction is done in float64 and rounded once to float32, like the reference (bit-identical).              */
int szn_image_u8_to_bgr_f32(int B, int H, int W, const uint8_t* rgb_hwc, const double* mean_bgr, float* out_nchw,
                            szn_stream_t stream);

/* ---- validation visualisations (vis_utils.py:4-109; trainer_fcn.py:198-219, trainer_seenmask.py:117-133) -------------------
 * The uint8 RGB panels the reference draws on the host per validation image, written by one kernel from the device tensors the
 * validation pass already holds.  img: img_kind 0 = uint8 RGB [B][H][W][3]; 1 = the network input, f32 [B][3][H][W], BGR minus
 * mean_bgr (host, three doubles, BGR order; required for kind 1).  lbl_true / lbl_pred: int64 [B][H][W] on the device.  out: image b
 * starts at out + b * out_image_bytes, its rows are out_row_bytes apart (so a caller can render into a larger canvas); bytes outside
 * the panels are never written.  Integer-exact contract, per source pixel (b, y, x):
 *   pixel    kind 0: the bytes.  kind 1: v = (double)x_c + mean_bgr[c], u_c = clamp((int)floor(v + 0.5), 0, 255), BGR -> RGB.  (Rounded
 *            where dataset.untransform truncates: u - mean -> f32 -> + mean comes back exactly u only with rounding, so both kinds
 *            give the same bytes for an image that went through szn_image_u8_to_bgr_f32.)
 *   grey     g = (19595 R + 38470 G + 7471 B + 32768) >> 16                                   (PIL's convert('L'))
 *   colour   of class k in [0, K): for j = 0..7: r |= bit0(c) << (7-j), g |= bit1(c) << (7-j), b |= bit2(c) << (7-j), c >>= 3, from
 *            c = k (the PASCAL map: 1 -> (128,0,0), 15 -> (192,128,128), 255 -> (224,224,192)); a label outside [0, K) is black
 *   overlay  (colour + g) >> 1 per channel
 *   mask     255 on all channels iff the label is in [0, K) and not in `unseen`, else 0
 *   noise    byte_c = ((h >> 40) * 255) >> 24, h = splitmix64(seed * 0xD1342543DE82EF95 + 3 * ((b*H + y)*W + x) + c): 0..254, the
 *            generator of szn_dropout2d_mask.  (The reference's noise is unseeded.)
 * szn_viz_segmentation: panels H x W; columns image | colour | overlay | mask (the mask column only with unseen != NULL: n_col = 4,
 * else 3); row 0 from lbl_true, row 1 from lbl_pred: the rendered image is 2H x n_col*W.  A pixel is unlabelled iff lbl_true is
 * < 0 or >= K there (-1, the batch padding -2); an unlabelled pixel is noise in every panel but the image panels, in BOTH rows, the
 * same three bytes everywhere.  lbl_true == NULL: only the prediction row (H x n_col*W), no noise.
 * szn_viz_seenmask: one row of three panels, image | 255 * (lbl_true == 1) | 255 * (lbl_pred == 1); pixels with lbl_true < 0 are
 * noise in panels 1 and 2.
 * SZN_ERR_ARG: NULL img / lbl_pred / out (seen-mask: lbl_true too), an empty shape, an unknown img_kind, K outside
 * [1, SZN_MAX_CLASSES], a set naming a class >= K, out_row_bytes below a panel row (3 * n_col * W), out_image_bytes below a rendered
 * image ((rows*H - 1) * out_row_bytes + 3 * n_col * W).  szn_last_kernel(): viz_panels_kernel, or viz_panels_kernel_v4 when W % 4 == 0,
 * out, out_row_bytes and out_image_bytes are multiples of 4 (every 4-pixel panel segment is then three aligned dword stores).   */
int szn_viz_segmentation(int B, int H, int W, const void* img, int img_kind, const double* mean_bgr, const int64_t* lbl_true,
                         const int64_t* lbl_pred, int K, const szn_class_set* unseen, uint64_t seed, uint8_t* out,
                         long out_row_bytes, long out_image_bytes, szn_stream_t stream);
int szn_viz_seenmask(int B, int H, int W, const void* img, int img_kind, const double* mean_bgr, const int64_t* lbl_true,
                     const int64_t* lbl_pred, uint64_t seed, uint8_t* out, long out_row_bytes, long out_image_bytes,
                     szn_stream_t stream);

/* ---- training augmentation (no reference counterpart: the reference shows every image as stored) ------------------------------
 * Random scale, crop to a fixed size and horizontal flip of a raw batch, in one kernel: uint8 RGB canvases [B][Hm][Wm][3] and their
 * int64 labels [B][Hm][Wm] (image b occupies the top-left h x w of its canvas) -> the (B,3,Ho,Wo) f32 BGR-minus-mean network input and
 * the (B,Ho,Wo) int64 target.  params: DEVICE memory, SZN_AUG_NPARAM int32 per image, built on the host:
 *   [0] h  [1] w           the image's own size inside the canvas
 *   [2] Hs [3] Ws          its size after scaling
 *   [4] step_y [5] step_x  source step per output pixel, 16.16 fixed point:  step_y = ((h << 16) + Hs/2) / Hs
 *   [6] oy [7] ox          origin of the crop window in the scaled image; may be negative and may run past Hs / Ws
 *   [8] flip               non-zero: mirror the crop horizontally
 * mean_bgr: host, three doubles, BGR order.  Integer-exact contract, per output pixel (b, yo, xo):
 *   position  xo' = flip ? Wo-1-xo : xo;  gy = yo + oy, gx = xo' + ox.  gy outside [0, Hs) or gx outside [0, Ws): the pixel is padding,
 *             all three planes exactly 0.0f (the mean colour) and the label SZN_PAD_LABEL.  Otherwise
 *             sy = (((2*gy + 1) * (int64)step_y) >> 1) - 32768 (the pixel-centre map of align_corners=False), sx likewise.
 *   image     sy clamped to [0, (h-1) << 16]; y0 = sy >> 16, y1 = min(y0 + 1, h - 1), wy = (sy & 0xffff) >> 5 (11 bits); x0, x1, wx the
 *             same from sx and w.  v = (2048-wy) * ((2048-wx)*p00 + wx*p01) + wy * ((2048-wx)*p10 + wx*p11) in int32 (<= 255 * 2^22:
 *             no overflow, no rounding); out_c = (float)((double)v / 4194304.0 - mean_bgr[c]), plane c from source byte 2 - c.  With
 *             step 65536, zero origin and no flip, v = p << 22: bit-identical to szn_image_u8_to_bgr_f32.  (Bilinear without
 *             antialiasing when shrinking.)
 *   label     nearest neighbour from the UNCLAMPED position: ly = clamp((sy + 32768) >> 16, 0, h-1), lx likewise; the value is copied
 *             as is (-1 stays -1).
 * Record fields that cannot be right are made harmless on the device, where alone they can be seen: h, w are clamped to [1, Hm] /
 * [1, Wm] and every source index to the image, so no read leaves the canvas; Hs or Ws < 1 makes the whole image padding.
 * SZN_ERR_ARG: a NULL pointer, a size that is not positive, B > 65535.  szn_last_kernel(): augment_u8_kernel_v4 when Wo % 4 == 0 and
 * out_nchw, out_label are 16-byte aligned (a thread's 4 adjacent output pixels leave as 16-byte stores), else augment_u8_kernel
 * (scalar stores; the last run of a row is partial).                                                                          */
#define SZN_AUG_NPARAM 9
#define SZN_PAD_LABEL (-2)          /* datasets.PAD_LABEL: ignored by every loss, class-assignment and histogram kernel */
int szn_augment_u8(int B, int Hm, int Wm, const uint8_t* rgb_hwc, const int64_t* label, const int32_t* params,
                   const double* mean_bgr, int Ho, int Wo, float* out_nchw, int64_t* out_label, szn_stream_t stream);

/* szn_augment_affine_u8: szn_augment_u8 with a 2 x 3 affine position map (rotation; the scale, the crop window and the mirror are folded
 * into it by the host) and a 3 x 4 colour matrix (brightness, contrast, saturation and hue are affine in RGB and collapse into one).
 * Inputs, outputs, canvas convention, mean_bgr and the error rules are szn_augment_u8's.  params: DEVICE memory, SZN_AUGA_NPARAM int32
 * per image:
 *   [0] h  [1] w              the image's own size inside the canvas; clamped to [1, Hm] / [1, Wm] on the device
 *   [2] mxx [3] mxy [4] tx    source x as a function of the output pixel, 16.16 fixed point
 *   [5] myx [6] myy [7] ty    source y, likewise
 *   [8..16] Cm[c][d]          colour matrix, Q16, row-major: output channel c from input channel d, both in RGB order
 *   [17..19] Co[c]            colour offset, grey levels in Q16
 * Integer-exact contract, per output pixel (b, yo, xo); all arithmetic is int64, >> is the arithmetic (floor) shift:
 *   position  X = 2*xo + 1, Y = 2*yo + 1;  sx = ((mxx*X + mxy*Y) >> 1) + tx - 32768,  sy = ((myx*X + myy*Y) >> 1) + ty - 32768
 *             (szn_augment_u8's pixel-centre convention).
 *   padding   lx = (sx + 32768) >> 16, ly = (sy + 32768) >> 16.  lx outside [0, w) or ly outside [0, h): the pixel is padding, all three
 *             planes exactly 0.0f and the label SZN_PAD_LABEL.
 *   taps      sx clamped to [0, (w-1) << 16]; x0 = sx >> 16, x1 = min(x0 + 1, w - 1), wx = (sx & 0xffff) >> 5; the same in y.  Per source
 *             byte d: acc_d = (2048-wy) * ((2048-wx)*p00 + wx*p01) + wy * ((2048-wx)*p10 + wx*p11)  (<= 255 * 2^22).
 *   colour    u_c = sum_d Cm[c][d] * acc_d + ((int64)Co[c] << 22), clamped to [0, 255 << 38] (unit: 2^-38 grey level);
 *             out plane 2-c = (float)((double)u_c / 2^38 - mean_bgr[2-c]).  u_c < 2^46, so the conversion and the division are exact and
 *             the only rounding is the double subtraction and the cast: the rounding of szn_image_u8_to_bgr_f32.  Every Cm word is
 *             clamped to +-2^20 before use, so that no record can overflow int64 (|sum| <= 3 * 2^50 + 2^53).
 *   label     label[ly][lx], copied as is.
 * Two identities hold bit for bit:
 *   identity colour   Cm = 65536 * I, Co = 0 gives u = acc << 16, hence (double)acc / 2^22 - mean: szn_augment_u8's value.
 *   axis-aligned      the record (h, w, Hs, Ws, step_y, step_x, oy, ox, flip) of szn_augment_u8 becomes  mxx = flip ? -step_x : step_x,
 *                     mxy = 0, tx = step_x * (ox + (flip ? Wo : 0)),  myx = 0, myy = step_y, ty = step_y * oy:  the source positions
 *                     are szn_augment_u8's exactly, because (a + 2k) >> 1 == (a >> 1) + k.  The padding rule differs in form (source
 *                     space here, the scaled grid there); the two agree whenever Ws * Ws < 65536 * w and Hs * Hs < 65536 * h.
 * The products are exact for Ho, Wo < 2^29; beyond that, as for a garbage record, they wrap modulo 2^64 and every index is still checked
 * against the image before it is used: no read leaves the canvas.
 * SZN_ERR_ARG exactly where szn_augment_u8 returns it.  szn_last_kernel(): augment_affine_u8_kernel_v4 when Wo % 4 == 0 and out_nchw,
 * out_label are 16-byte aligned, else augment_affine_u8_kernel.                                                                   */
#define SZN_AUGA_NPARAM 20
int szn_augment_affine_u8(int B, int Hm, int Wm, const uint8_t* rgb_hwc, const int64_t* label, const int32_t* params,
                          const double* mean_bgr, int Ho, int Wo, float* out_nchw, int64_t* out_label, szn_stream_t stream);

/* ---- multi-scale / mirrored inference (no reference counterpart: the reference evaluates every image once, as stored) -----------
 * szn_resize_flip_f32 makes one view of the network input: in (B,3,H,W) f32 NCHW -> out (B,3,Hs,Ws), bilinear without antialiasing,
 * with the position map and the 11-bit weights of szn_augment_u8.  Per output pixel (b, yo, xo), xo' = flip ? Ws-1-xo : xo:
 *   step_y = ((H << 16) + Hs/2) / Hs;  sy = (((2*yo + 1) * (int64)step_y) >> 1) - 32768 clamped to [0, (H-1) << 16];
 *   y0 = sy >> 16, y1 = min(y0 + 1, H - 1), wy = (sy & 0xffff) >> 5;  x0, x1, wx the same from xo', W and Ws;
 *   out = (float)(((2048-wy) * ((2048-wx)*(double)p00 + wx*(double)p01) + wy * ((2048-wx)*(double)p10 + wx*(double)p11)) / 4194304.0)
 * in that operation order, no contraction.  Hs == H, Ws == W, flip == 0 reproduces the input bit for bit.
 * SZN_ERR_ARG: a NULL pointer, a size that is not positive, B > 65535.                                                            */
int szn_resize_flip_f32(int B, int H, int W, const float* in_nchw, int Hs, int Ws, int flip, float* out_nchw, szn_stream_t stream);

/* szn_ms_head: the view-ensemble embedding head.  It reads the coarse maps the network produced for n_views views of one batch
 * (szn_resize_flip_f32 of the (B,3,H,W) input) and writes the class prediction at the original size, without a per-pixel score in
 * memory.  One view: its NHWC f32 coarse map (DEVICE pointer) [B][h][w] with pixel stride ldc, the E embedding channels at
 * [c0, c0+E); Hs x Ws = the view's image size; flip = the view was mirrored.  The array of views is HOST memory, read during the call.
 * Per original pixel (b, y, x) and view v, in array order:
 *   xm = flip_v ? W-1-x : x; (y, xm) is mapped into the view's Hs x Ws grid by the map above (source size Hs, Ws; destination H, W):
 *   four view pixels with 11-bit weights.  A view pixel's score vector is the stride-S bilinear upsample + crop of coarse_v
 *   (szn_bilinear_up_crop_fwd's definition); s_v = the weighted sum of the four;
 *   sim_v[k] = s_v . e_k / (||s_v|| * (||e_k|| == 0 ? 1 : ||e_k||))   (szn_embed_argmax's formula);   A[k] = sum_v sim_v[k], added in
 *   fp32 in view order.
 * pred = the first k whose value exceeds the running best, starting from k = 0 (a NaN gives class 0).  Group modes 0 / 1 / 2 are
 * szn_fused_head_grouped's: a class outside the pixel's group competes with the value 0 instead of A[k]; negative labels take the
 * seen group.  acc (optional, [B][H][W][K] f32) receives the ungrouped A; pred does not depend on it.  The E-long products are taken
 * once per coarse position (C_pos . e_k and the Gram entries C_pos . C_q of the 13 neighbour offsets a pixel's 3 x 3 composite taps
 * can pair), the pixel pass combines them.  Fixed order, no atomics: two calls are bit-equal.  szn_last_kernel(): ms_pixel_kernel.
 * workspace: szn_ms_head_workspace_bytes (0 for arguments szn_ms_head refuses), 16-byte aligned; its head is a szn_fused_head_prepare
 * image, written by the call.
 * SZN_ERR_ARG, before any launch: n_views outside [1, SZN_MS_MAX_VIEWS]; stride not 8 or 32; a NULL views[i].coarse, embed, pred or
 * workspace; a size that is not positive; a map with h or w > 32767 or B h w >= 2^33; Hs or Ws < 1; ldc < c0 + E; a view with Hs + crop > stride * (h + 1) or Ws + crop >
 * stride * (w + 1); K > SZN_MAX_CLASSES; group mode 1 without group_map, 2 without target; a class in `unseen` >= K.             */
typedef struct szn_ms_view {
    const float* coarse;
    int h, w, ldc, c0, Hs, Ws, flip;
} szn_ms_view_t;
#define SZN_MS_MAX_VIEWS 16
size_t szn_ms_head_workspace_bytes(int stride, int B, int E, int K, int n_views, const szn_ms_view_t* views);
int szn_ms_head(int stride, int B, int E, int K, int H, int W, int crop, int n_views, const szn_ms_view_t* views,
                const float* embed, const szn_class_set* unseen, int group_mode, const int64_t* group_map,
                const int64_t* target, int64_t* pred, float* acc, void* workspace, szn_stream_t stream);

/* ---- calibrated generalized zero-shot inference (calibrated stacking) ---------------------------------------------------------
 * szn_calib_head: one scalar gamma is subtracted from the similarity of every SEEN class (a class not in `unseen`) before the argmax,
 * for n_gammas candidate values in one pass over the pixels: per gamma a confusion histogram, and for one of them the prediction.
 * coarse, embed, stride (32 | 8), crop, ldc and c0 are szn_fused_head_strided's.  gammas: HOST memory, read during the call, finite and
 * strictly ascending.  Per pixel:
 *   sim[k] = the ungrouped similarity of szn_fused_head_strided, the same operations in the same order (the G / Q tables, the fmaf chain
 *            over the four taps, d / (sn * en[k]) with a zero norm replaced by 1);
 *   a, va  = the first seen class holding the seen maximum (the running best starts at the first seen class, only a strictly larger
 *            value replaces it);  b, vb = the same over the unseen classes;  m = va - vb, one fp32 subtraction;
 *   pred_g = 0 if m is NaN; else a if m > gammas[g], or if m == gammas[g] and a < b; else b.
 * The rule is written on the margin, not as an argmax over sim[k] - gamma: rounding the penalised values could create ties and reorder
 * the classes inside the seen group.  Consequences: at gamma = 0 pred equals szn_fused_head_strided's pred bit for bit wherever the
 * similarities are finite (m > 0 exactly when va > vb, an exact tie goes to the smaller index); a zero-norm pixel gives class 0 in both.
 *   hist [n_gammas][K][K] int64 (device, or NULL):  hist[g][t][pred_g] += 1 for every pixel whose target t has 0 <= t < K
 *            (szn_confusion_hist_k's rule: -1, the padding label and labels >= K are skipped).  The seen / unseen histograms of a
 *            validation pass are row subsets of hist[g]; the caller takes them.
 *   pred (B,H,W) int64 (device, or NULL): pred_g for g = pred_index.
 * With ascending gammas the g at which a pixel takes b are upward closed, so a pixel is described by (t, a, b, bin), bin = the first g
 * at which it takes b (n_gammas: never).  The pixel pass adds the pixel to two crossing tables XA[t][a][bin], XB[t][b][bin] in the
 * workspace (zeroed by the call; equal keys of a wave are combined first, one 64-bit integer atomic add per distinct key and table), a
 * second small kernel adds sum_{bin > g} XA[t][k][bin] + sum_{bin <= g} XB[t][k][bin] to hist[g][t][k]: the cost does not grow with
 * n_gammas.  The counts are integers: any accumulation order gives the same result, two calls are bit-equal.
 * szn_last_kernel(): calib_hist_kernel when hist is given (szn_prev_kernel(): the pixel kernel), else the pixel kernel --
 * calib_cell_kernel (stride 32) or calib_cell_tab_kernel (stride 8).
 * workspace: szn_calib_head_workspace_bytes (0 for arguments szn_calib_head refuses), 16-byte aligned: a szn_fused_head_prepare image
 * written by the call, the stride-8 position tables, and the crossing tables, 2 * K^2 * (n_gammas + 1) int64 (1.9 MB at K = 59, 33 gammas).
 * SZN_ERR_ARG, before any launch: stride not 8 or 32; n_gammas outside [1, SZN_CALIB_MAX_GAMMAS]; a gamma that is not finite, or gammas
 * not strictly ascending; hist and pred both NULL; hist without target; pred with pred_index outside [0, n_gammas); NULL coarse, embed,
 * workspace or gammas; `unseen` NULL or empty, or containing every class below K (both groups must be non-empty); a class in `unseen`
 * >= K; K > SZN_MAX_CLASSES; a size that is not positive, ldc < c0 + E, a crop window larger than the deconv output, a workspace that is
 * not 16-byte aligned (szn_fused_head_strided's checks).                                                                            */
#define SZN_CALIB_MAX_GAMMAS 64
size_t szn_calib_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int n_gammas);
int szn_calib_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                   const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                   int n_gammas, const float* gammas, int64_t* hist, int pred_index, int64_t* pred,
                   void* workspace, szn_stream_t stream);

/* ---- full SZN inference with a seen-mask threshold ------------------------------------------------------------------------------
 * szn_seen_sweep_head: szn_fused_head_grouped's class assignment (group mode 1) with the group decided by a threshold on the seen-mask
 * logit margin (szn_seenmask_margin) instead of s1 > s0, for n_taus thresholds in one pass over the pixels: per threshold a confusion
 * histogram, and for one of them the prediction.  coarse, embed, stride (32 | 8), crop, ldc and c0 are szn_fused_head_strided's; margin
 * (B,H,W) f32 device; taus: HOST memory, read during the call, finite and strictly ascending.  Per pixel and per g:
 *   pred_g = what szn_fused_head_grouped (group mode 1) writes for the pixel when group_map[pix] = (margin[pix] > taus[g]) ? 1 : 0, bit
 *            for bit: the classes outside the pixel's group score 0 / (sn * 1) and still compete, the first index wins a tie, a
 *            zero-norm pixel gives class 0.  A NaN margin compares false: the unseen group at every g, as s1 > s0 does.
 * tau = 0 is szn_seenmask_head_k's decision; p(seen) > sigmoid(tau) in general.  With ascending taus the g at which a pixel takes the
 * unseen group are upward closed, so a pixel is described by (t, a, b, bin): a = the grouped head's answer in the seen group, b = in the
 * unseen group (one trip through the classes, two running bests that each see the grouped head's own sequence of values), bin = the
 * first g with !(margin > taus[g]) (n_taus: never).  From there on the call is szn_calib_head: XA[t][a][bin] and XB[t][b][bin] in the
 * workspace, one 64-bit integer atomic add per distinct key of a wave and table, calib_hist_kernel adds the prefix sums to
 *   hist [n_taus][K][K] int64 (device, or NULL):  hist[g][t][pred_g] += 1 for every pixel whose target t has 0 <= t < K;
 *   pred (B,H,W) int64 (device, or NULL): pred_g for g = pred_index.
 * The cost does not grow with n_taus; integer counts, two calls are bit-equal.
 * szn_last_kernel(): calib_hist_kernel when hist is given (szn_prev_kernel(): the pixel kernel), else the pixel kernel --
 * sweep_cell_kernel (stride 32) or sweep_cell_tab_kernel (stride 8).
 * workspace: szn_seen_sweep_head_workspace_bytes (0 for sizes the call refuses), 16-byte aligned, szn_calib_head's layout: the prepared
 * embedding image written by the call, the stride-8 position tables, the crossing tables, 2 * K^2 * (n_taus + 1) int64.
 * SZN_ERR_ARG, before any launch: everything szn_calib_head refuses, with taus for gammas (stride, n_taus outside
 * [1, SZN_SEEN_SWEEP_MAX_TAUS], a tau that is not finite or taus not strictly ascending, hist and pred both NULL, hist without target,
 * pred_index outside [0, n_taus), NULL coarse / embed / workspace / taus, `unseen` NULL, empty, holding every class below K or a class
 * >= K, K > SZN_MAX_CLASSES, sizes, ldc < c0 + E, the crop window, the workspace alignment), and a NULL margin.                        */
#define SZN_SEEN_SWEEP_MAX_TAUS 64
size_t szn_seen_sweep_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int n_taus);
int szn_seen_sweep_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                        const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                        const float* margin, int n_taus, const float* taus, int64_t* hist, int pred_index, int64_t* pred,
                        void* workspace, szn_stream_t stream);
/* the same for a caller that has just run a fused embedding head (szn_fused_head_strided / _grouped / _mse_head / _simce_head or their
 * _prepared forms) with this stride, B, h, w, E, K, coarse, ldc, c0 and embed on the head of THIS workspace, earlier on this stream: the
 * prepared embedding image and the stride-8 position tables that call left there are exactly what this one would build, so it builds
 * neither (full SZN validation runs the plain head for the loss first; at stride 8 the tables are the larger part of either call).  The
 * caller vouches for that; nothing else differs: arguments, refusals, results and szn_last_kernel() are szn_seen_sweep_head's.        */
int szn_seen_sweep_head_tabled(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                               const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                               const float* margin, int n_taus, const float* taus, int64_t* hist, int pred_index, int64_t* pred,
                               void* workspace, szn_stream_t stream);

/* ---- full SZN inference with a soft seen/unseen gate --------------------------------------------------------------------------------
 * szn_soft_gate_head: the probabilistic form of the seen-mask route (a novelty detector in front of two classifiers, Socher et al. 2013;
 * Atzmon & Chechik 2019): p(k | x) = p(group(k) | x) p(k | group(k), x) with p(seen | x) = sigmoid(m - tau), m = margin[pix], and inside
 * each group a softmax over the cosines at `temperature`.  With a / b the best seen / best unseen class, the pixel takes a iff
 * m - tau > log P_U(b) - log P_S(a): a per-pixel adaptive threshold on the margin, so the call is szn_seen_sweep_head with another
 * per-pixel body.  Arguments, workspace layout (szn_soft_gate_head_workspace_bytes == szn_seen_sweep_head_workspace_bytes), refusals and
 * the _tabled form are szn_seen_sweep_head's.  Per pixel:
 *   sim[k]   = szn_calib_head's ungrouped similarity, the same operations in the same order;
 *   a, va / b, vb = the TRUE argmax inside the seen / the unseen group, the first index winning (szn_calib_head's two running bests).
 *              This is NOT szn_seen_sweep_head's pair: there a class outside the group competes with 0 / (sn * 1), the reference's
 *              zeroed-row quirk, which has no probabilistic meaning.  The two agree where each group's best cosine is positive;
 *   inv_t    = 1.0f / temperature (one fp32 division on the host);
 *   l_S      = logf(sum_{k seen} expf((sim[k] - va) * inv_t)) = -log P_S(a), l_U likewise over `unseen` with vb: 0 <= l_G <= log n_G, each
 *              sum shifted by its own group's maximum (an online sum, rescaled when the running best moves: one expf per class, every
 *              exponent <= 0); a group of one class gives exactly 0.0f;
 *   D        = l_S - l_U,  e = fmaf(-weight, D, m);
 *   the pixel takes a at g iff e > taus[g]; bin = the first g at which that fails (n_taus: never).
 * D NaN (a zero-norm pixel): a = b = 0, class 0 at every tau (szn_calib_head's rule).  A NaN margin compares false: b at every tau.
 * weight = 0 is the hard threshold on the true groups (e == m bit for bit), weight = 1 the probabilistic rule, larger weights trust the
 * two experts more.  hist, pred, the crossing tables and calib_hist_kernel are szn_seen_sweep_head's: integer counts, two calls bit-equal.
 *   eff (B,H,W) f32 (device, or NULL): e per pixel (NaN where D or the margin is NaN).
 * szn_last_kernel(): calib_hist_kernel when hist is given (szn_prev_kernel(): the pixel kernel), else the pixel kernel --
 * gate_cell_kernel (stride 32) or gate_cell_tab_kernel (stride 8).
 * SZN_ERR_ARG, before any launch: everything szn_seen_sweep_head refuses, except that hist and pred may both be NULL when eff is given
 * (hist, pred and eff all NULL is refused); a temperature that is not finite or <= 0; a weight that is not finite or < 0.             */
size_t szn_soft_gate_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int n_taus);
int szn_soft_gate_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                       const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                       const float* margin, float temperature, float weight,
                       int n_taus, const float* taus, int64_t* hist, int pred_index, int64_t* pred, float* eff,
                       void* workspace, szn_stream_t stream);
/* on a workspace in whose head a fused embedding head has just run on this map: szn_seen_sweep_head_tabled's vouching rule            */
int szn_soft_gate_head_tabled(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                              const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                              const float* margin, float temperature, float weight,
                              int n_taus, const float* taus, int64_t* hist, int pred_index, int64_t* pred, float* eff,
                              void* workspace, szn_stream_t stream);

/* ---- hubness correction for zero-shot inference ---------------------------------------------------------------------------------------
 * A few class vectors end up near a large share of all projected pixels and take their predictions (hubness: Radovanovic et al. 2010; Dinu
 * et al. 2015).  The label-free answers act per class: centering subtracts from each class's similarity its mean similarity to the queries
 * (Suzuki et al. 2013), standardising divides by the spread as well.  The queries are the pixels of the image being segmented.
 *
 * szn_hub_stats writes per image and class a pair (scale, shift): table [B][K][2] f32 (device).  coarse, embed, stride (32 | 8), crop, ldc and
 * c0 are szn_fused_head_strided's.  A pixel of image b counts when it lies inside H x W, target is NULL or target[pix] != SZN_PAD_LABEL, and
 * its norm sn is finite and > 0; unlabelled (-1) and hidden pixels count: the statistics are label-free.  For a counted pixel and class k:
 *   sim[k] = szn_calib_head's similarity, the same operations in the same order;
 *   q      = clamp((long long)rintf(sim[k] * 1048576.f), -2^21, 2^21);   S1[b][k] += q;  S2[b][k] += q * q;  n[b] += 1 once per pixel,
 * all int64: any accumulation order gives the same bits, two calls are bit-equal, and a batch's composition changes nothing.  A second
 * kernel (one thread per (b, k), double arithmetic) forms mean = S1 / (n 2^20), sd = sqrt(max(S2 / (n 2^40) - mean^2, 0)) and the row
 *   mode SZN_HUB_MEAN:    scale = 1,                        shift = (float)(beta * mean);
 *   mode SZN_HUB_ZSCORE:  f = max(sd, min_sd),  scale = (float)(1 / f),  shift = (float)(beta * mean / f);
 *   n[b] == 0:            the identity row (1, 0).
 * beta = 1 is the textbook form, beta = 0 in mean mode the identity.  sums [B][K][2] int64 (S1, S2) and counts [B] int64 (device, or NULL)
 * are inspection copies, written, not accumulated.  No host synchronisation; the call can be captured into a graph.
 * Pixel pass: classes outermost, each thread adds its own pixels for class k, a wave reduction, one LDS slot per wave, class and moment, and
 * one 64-bit integer atomic add per block (stride 8: per image present in the block), class and moment.
 * szn_last_kernel(): hub_table_kernel (szn_prev_kernel(): hub_stats_cell_kernel at stride 32, hub_stats_cell_tab_kernel at stride 8).
 * workspace: szn_hub_stats_workspace_bytes (0 for sizes the call refuses), 16-byte aligned: the fused head's (prepared embedding image,
 * stride-8 position tables), then S1 / S2 and n.
 * SZN_ERR_ARG, before any launch: everything szn_fused_head_strided refuses (stride not 8 or 32, a size that is not positive,
 * K > SZN_MAX_CLASSES, ldc < c0 + E, the crop window, NULL coarse / embed / workspace, the workspace alignment); a mode other than the two; beta
 * not finite or < 0; min_sd not finite or <= 0; NULL table; H * W > SZN_HUB_MAX_PIXELS (2^22: S2 <= 2^42 per pixel stays inside int64).
 *
 * szn_hub_head is szn_calib_head with one change: the value that enters the two running bests is
 *   adj[k] = fmaf(sim[k], table[b][k][0], -table[b][k][1])
 * (k is uniform per wave and b per block or wave: two scalar loads per class).  Everything else is szn_calib_head's: the first index wins, a
 * strictly larger value replaces, m = va - vb, pred = 0 if m is NaN, else a if m > gamma or (m == gamma and a < b), else b; the keys into the
 * crossing tables, calib_hist_kernel, pred_index, the workspace layout (szn_hub_head_workspace_bytes == szn_calib_head_workspace_bytes) and
 * the refusals, plus a NULL table.  With the identity table fmaf(sim, 1, -0.0f) == sim bit for bit, so pred and hist equal szn_calib_head's
 * exactly.  The table is a plain device input [B][K][2] f32: a caller may pass one of its own (dataset-level statistics, class priors as
 * shifts) instead of szn_hub_stats'.  A NaN or infinite entry makes that class's adj NaN or infinite for every pixel of the image.
 * szn_last_kernel(): calib_hist_kernel when hist is given (szn_prev_kernel(): the pixel kernel), else the pixel kernel --
 * hub_cell_kernel (stride 32) or hub_cell_tab_kernel (stride 8).                                                                          */
#define SZN_HUB_MEAN 0
#define SZN_HUB_ZSCORE 1
#define SZN_HUB_MAX_PIXELS (1 << 22)
size_t szn_hub_stats_workspace_bytes(int stride, int B, int h, int w, int E, int K);
int szn_hub_stats(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                  const float* coarse, const float* embed, const int64_t* target, int mode, float beta, float min_sd,
                  float* table, int64_t* sums, int64_t* counts, void* workspace, szn_stream_t stream);
size_t szn_hub_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int n_gammas);
int szn_hub_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                 const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                 const float* table, int n_gammas, const float* gammas, int64_t* hist, int pred_index, int64_t* pred,
                 void* workspace, szn_stream_t stream);

/* ---- ConSE zero-shot inference for the softmax FCN ---------------------------------------------------------------------------------
 * szn_conse_head: convex combination of semantic embeddings (Norouzi et al., ICLR 2014) per pixel, from the logit map of a network that
 * was trained on the seen classes with szn_fused_ce_head, with the seen-class penalty gamma of szn_calib_head swept over n_gammas values
 * in one pass.  coarse: the fp32 NHWC logit map, the K class channels at [c0, c0 + K) of pixel stride ldc; stride (32 | 8), crop, h, w, H
 * and W are szn_fused_ce_head's.  embed [K][E] f32 (device).  unseen: as in szn_calib_head, non-empty and not every class.  gammas: HOST
 * memory, read during the call, finite and strictly ascending.  Per pixel (only the logits are pinned bit for bit, the rest is
 * mathematics plus tie rules):
 *   z[c]   = szn_fused_ce_head's logit (the same bilinear weights, the same fmaf chain over the four taps): bit-identical;
 *   S      = the first min(top_t, n_seen) SEEN classes ordered by (z descending, class index ascending); the channels of unseen classes
 *            are never read;
 *   p_t    = exp(z_t - max_S z) / sum_S exp(z - max_S z): the seen-class softmax renormalised over S (ConSE's normalisation; what the
 *            full seen-class denominator adds cancels);
 *   sim[k] = (sum_{t in S} p_t G[t][k]) / (|f| * en[k]),  G = embed embed^T (products accumulated in double, stored fp32, built once per
 *            call), en[k] = sqrt(G[k][k]), |f| = sqrt(sum_{t,u in S} p_t p_u G[t][u]), a zero |f| or en[k] replaced by 1 (the cosine
 *            heads' rule).  The mixture f = sum_t p_t e_t is never formed: E is not on the per-pixel path;
 *   a, va  = the first seen class holding the seen maximum of sim;  b, vb = the same over the unseen classes;  m = va - vb;
 *   pred_g = szn_calib_head's rule: 0 if m is NaN; else a if m > gammas[g], or if m == gammas[g] and a < b; else b.
 * forced = 0:  hist [n_gammas][K][K] int64 (device, or NULL): hist[g][t][pred_g] += 1 for every pixel whose target t has 0 <= t < K (-1,
 *            the padding label and labels >= K are skipped);  pred (B,H,W) int64 (device, or NULL): pred_g for g = pred_index.  The pixel's
 *            (t, a, b, bin) record goes through szn_calib_head's crossing tables and calib_hist_kernel: the cost does not grow with n_gammas.
 * forced = 1 (the reference's -fu): pred = b where target names an unseen class, a elsewhere (0 where m is NaN); gammas and hist must be
 *            NULL, n_gammas 0, target and pred given.
 * No atomics except the crossing tables' integer adds: two calls are bit-equal.  Scalar arguments, no allocation, no host sync.
 * szn_last_kernel(): calib_hist_kernel when hist is given (szn_prev_kernel(): the pixel kernel), else the pixel kernel -- conse_cell_kernel
 * (G copied into LDS: taps + en + G within 64 KiB, K <= 119 at stride 8 and K <= 125 at stride 32) or conse_cell_global_kernel (G read
 * through L2); the launch before the pixel kernel is conse_prep_kernel.
 * workspace: szn_conse_head_workspace_bytes (0 for sizes the call refuses; n_gammas = 0 sizes the forced call), 16-byte aligned: G
 * [K][K | 1] and en [K] floats, then the crossing tables, 2 * K^2 * (n_gammas + 1) int64 (none for the forced call).
 * SZN_ERR_ARG, before any launch: everything szn_calib_head refuses (stride not 8 or 32; n_gammas outside [1, SZN_CALIB_MAX_GAMMAS]; a
 * gamma that is not finite, or gammas not strictly ascending; hist and pred both NULL; hist without target; pred with pred_index outside
 * [0, n_gammas); NULL coarse, embed, workspace or gammas; `unseen` NULL, empty, holding every class below K or a class >= K; K >
 * SZN_MAX_CLASSES; a size that is not positive; a crop window larger than the deconv output; a workspace that is not 16-byte aligned),
 * with ldc < c0 + K in place of its ldc rule; top_t outside [1, SZN_CONSE_MAX_TOP]; forced not 0 or 1; a forced call with gammas, hist
 * or n_gammas != 0, or without target or pred.  SZN_ERR_UNSUPPORTED: a cell's taps that do not fit LDS (no K <= SZN_MAX_CLASSES does that). */
#define SZN_CONSE_MAX_TOP 16
size_t szn_conse_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int n_gammas);
int szn_conse_head(int stride, int B, int h, int w, int K, int ldc, int c0, int H, int W, int crop, int E,
                   const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                   int top_t, int forced, int n_gammas, const float* gammas, int64_t* hist, int pred_index, int64_t* pred,
                   void* workspace, szn_stream_t stream);

/* ---- self-training on the hidden pixels: top-p% pseudo labels ------------------------------------------------------------------
 * szn_pseudo_head: the network's own calibrated prediction labels the most confident keep_permille / 1000 of the pixels whose label is
 * hidden (target == cand_label, a negative value: datasets.HIDDEN_LABEL), per unseen class, and writes the relabelled target.
 * coarse, embed, stride (32 | 8), crop, ldc, c0 and unseen are szn_calib_head's.  sim[k], a, va, b, vb and m = va - vb per pixel are that
 * head's, the same operations in the same order (the same device functions).  Three passes:
 *   1. candidates.  A pixel is a candidate when target[pix] == cand_label, m is not NaN, the calibrated rule at `gamma` picks b -- NOT
 *      (m > gamma or (m == gamma and a < b)) -- and vb >= conf_floor (a conf_floor <= -2 disables the floor).  Its class is b, its
 *      confidence c = vb (fp32), its bin q = clamp((int)floorf(fmaf(c, 512.f, 512.f)), 0, 1023): c * 512 is exact in fp32, so the
 *      float32 expression c * 512 + 512 gives the same q.  Every candidate adds 1 to Q[b][q], a [K][SZN_PSEUDO_BINS] integer table in the
 *      workspace, zeroed on the stream by the call (equal keys of a wave are combined first, one 64-bit integer atomic add per distinct
 *      key).  Pixels of other labels are not evaluated at all; pixels of a cell outside the image contribute nothing.
 *   2. thresholds, per class k, integers only: n_k = sum_q Q[k][q]; keep_k = (n_k * keep_permille + 999) / 1000; thr[k] = the largest
 *      bin t with sum_{q >= t} Q[k][q] >= keep_k, SZN_PSEUDO_BINS when n_k == 0; counts[k] = { n_k, sum_{q >= thr[k]} Q[k][q] }.  The
 *      whole threshold bin is taken: the selection does not depend on any order inside it, and selected_k >= keep_k.
 *   3. relabel, elementwise: target_out[pix] = b for a candidate with q >= thr[b]; target[pix] verbatim everywhere else (-1, the padding
 *      label, labels >= K, candidates that were not selected).
 * target_out (B,H,W) int64 is required and must not alias target.  Inspection copies, each NULL or device memory, all written (not
 * accumulated): cand (B,H,W) int64 (-1: no candidate), conf (B,H,W) fp32 (NaN: no candidate), qhist [K][SZN_PSEUDO_BINS] int64,
 * thr [K] int32, counts [K][2] int64.  gamma, conf_floor, keep_permille and cand_label are kernel arguments: no host synchronisation, no
 * allocation, capturable in a hipGraph.  Integer atomics only: two calls give bit-equal outputs.
 * szn_last_kernel(): pseudo_relabel_kernel; szn_prev_kernel(): pseudo_thr_kernel (before them pseudo_cell_kernel at stride 32,
 * pseudo_cell_tab_kernel at stride 8).
 * workspace: szn_pseudo_head_workspace_bytes (0 for shapes szn_pseudo_head refuses), 16-byte aligned: a szn_fused_head_prepare image written
 * by the call, the stride-8 position tables, Q, thr and the per-pixel record of pass 1 (8 bytes per pixel).
 * SZN_ERR_ARG, before any launch: everything szn_calib_head refuses about the arguments the two share (stride, sizes, K, ldc / c0, the crop
 * window, the workspace alignment, NULL coarse / embed / workspace, an `unseen` set that is NULL, empty, names a class >= K or holds every
 * class); gamma or conf_floor not finite; keep_permille outside [1, 1000]; cand_label >= 0; NULL target or target_out; target_out == target. */
#define SZN_PSEUDO_BINS 1024
size_t szn_pseudo_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int H, int W);
int szn_pseudo_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                    const float* coarse, const float* embed, const int64_t* target, const szn_class_set* unseen,
                    float gamma, float conf_floor, int keep_permille, int64_t cand_label,
                    int64_t* target_out, int64_t* cand, float* conf, int64_t* qhist, int32_t* thr, int64_t* counts,
                    void* workspace, szn_stream_t stream);

/* ---- hard-pixel mining for the embedding losses: keep the hardest labelled pixels of every image ---------------------------------
 * szn_ohem_head: per image, the keep_permille / 1000 of the labelled pixels whose own-class cosine is lowest -- and every pixel whose
 * cosine lies below `thresh` -- keep their label; every other labelled pixel reads drop_label (a negative value the heads ignore) in
 * target_out.  The head kernels are untouched: they train on target_out.  coarse, embed, stride (32 | 8), crop, ldc and c0 are
 * szn_fused_head_strided's.  Three passes, everything per image (the heads normalise per image):
 *   1. evaluate.  A pixel is evaluated when 0 <= target[pix] < K and its label is not in `skip` (NULL: the empty set; the exclude set of
 *      szn_fused_simce_head, whose pixels that head ignores and which must not use up the budget).  Its value c is the cosine-loss term
 *      of the fused head, the same operations in the same order: the fmaf chain over the four taps of G[t][label], divided by
 *      (sn * ent[label]) with the raw norm; c is NaN for a zero-norm pixel or class row.  Its bin q = 0 when c is NaN, else
 *      clamp((int)floorf(fmaf(c, 512.f, 512.f)), 0, 1023) (szn_pseudo_head's bin).  Every evaluated pixel adds 1 to Q[b][q], a
 *      [B][SZN_OHEM_BINS] integer table in the workspace, zeroed on the stream by the call (the bins of a block are counted in LDS first,
 *      one 64-bit integer atomic add per non-empty bin).  Pixels that are not evaluated skip the arithmetic.
 *   2. cut, per image b, integers only: n_b = sum_q Q[b][q]; keep_b = (n_b * keep_permille + 999) / 1000; tmin_b = the smallest t in
 *      [1, 1024] with sum_{q < t} Q[b][q] >= keep_b; tbin = clamp((int)floorf(thresh * 512 + 512), 0, 1024) (thresh rounded down to a bin
 *      edge; multiples of 1/512 are exact; thresh <= -1 turns it off); cut_b = max(tmin_b, tbin), 0 when n_b == 0;
 *      counts[b] = { n_b, sum_{q < cut_b} Q[b][q] }.  Whole bins are taken: the selection does not depend on any order inside a bin, at
 *      least keep_b >= 1 pixels of every image that has any are kept (no image is left without a counted pixel), and bin 0 is always
 *      kept (a NaN pixel reaches the head as it does without this call).
 *   3. relabel, elementwise: target_out[pix] = drop_label for an evaluated pixel with q >= cut_b; target[pix] verbatim everywhere else
 *      (kept pixels, negative labels, labels >= K, labels in `skip`).
 * target_out (B,H,W) int64 is required and must not alias target.  Inspection copies, each NULL or device memory, all written (not
 * accumulated): conf (B,H,W) fp32 (c where the pixel was evaluated, NaN elsewhere), qhist [B][SZN_OHEM_BINS] int64, cut [B] int32,
 * counts [B][2] int64.  keep_permille, thresh and drop_label are kernel arguments: no host synchronisation, no allocation, capturable in
 * a hipGraph.  Integer atomics only: two calls give bit-equal outputs.
 * szn_last_kernel(): ohem_relabel_kernel; szn_prev_kernel(): ohem_cut_kernel (before them ohem_cell_kernel at stride 32,
 * ohem_cell_tab_kernel at stride 8).
 * workspace: szn_ohem_head_workspace_bytes (0 for shapes szn_ohem_head refuses), 16-byte aligned: a szn_fused_head_prepare image written
 * by the call, the stride-8 position tables, Q, cut and the per-pixel record of pass 1 (4 bytes per pixel).
 * SZN_ERR_ARG, before any launch: everything szn_pseudo_head refuses about the arguments the two share (stride, sizes, K, ldc / c0, the
 * crop window, the workspace alignment, NULL coarse / embed / workspace; an E too large for LDS is SZN_ERR_UNSUPPORTED as there);
 * keep_permille outside [1, 1000]; thresh not finite; drop_label >= 0; a class in `skip` >= K; a `skip` that holds every class; NULL
 * target or target_out; target_out == target. */
#define SZN_OHEM_BINS 1024
size_t szn_ohem_head_workspace_bytes(int stride, int B, int h, int w, int E, int K, int H, int W);
int szn_ohem_head(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                  const float* coarse, const float* embed, const int64_t* target, const szn_class_set* skip,
                  int keep_permille, float thresh, int64_t drop_label,
                  int64_t* target_out, float* conf, int64_t* qhist, int32_t* cut, int64_t* counts,
                  void* workspace, szn_stream_t stream);

/* ---- class prototypes: masked average pooling of the upsampled score, per class (few-shot adaptation of the class embeddings) -----
 * szn_class_proto: for every class k the sum, over the pixels `labels` gives it, of the pixel's score vector (SZN_PROTO_RAW) or of its
 * unit vector (SZN_PROTO_UNIT, the mean a cosine classifier wants), and the pixel counts -- without the (B,E,H,W) score in memory.
 * coarse, stride (32 | 8), crop, ldc, c0, h, w, H and W are szn_fused_head_strided's; labels is any int64 (B,H,W) map (ground truth, a
 * prediction, szn_pseudo_head's target_out).
 *   A pixel PARTICIPATES when 0 <= labels[pix] < K and its label is in `classes` (NULL: all K classes).  Every other label -- -1, -2,
 *   -3, a label >= K, a class outside the set -- is skipped without arithmetic.
 *   s = the pixel's upsampled, cropped score in fp32: the blend of the four taps of its cell with the weights of get_upsampling_weight
 *   (models.py:13-24).  |s| is formed as the fused head forms it: |s|^2 = the fmaf chain over the 16 (t, u) pairs of w_t w_u (C_t . C_u),
 *   each dot product 64 strided fp32 chains + xor butterfly, then sqrtf.
 *   A participating pixel CONTRIBUTES when |s| is finite and > 0 (UNIT), always (RAW).
 *   counts[K][2] int64 = { participating pixels, contributing pixels } of every class.
 *   sums[K][E] double = the sum over the contributing pixels of s (RAW) or s / |s| (UNIT), evaluated as sum_pos T[pos][k] *
 *   coarse[pos][c0 + e]: T[pos][k] = the sum over the class's contributing pixels that blend position pos of w_t (RAW) or w_t / |s|
 *   (UNIT).  w_t and |s| are fp32, the quotient, T and everything after are double (RAW: T and every product are exact, only the
 *   additions over the positions round).  Positions whose coefficient is 0 are skipped: a NaN under no contributing pixel stays out.
 *   Channels outside [c0, c0 + E) are never read.
 * accumulate = 0 writes all K rows of sums and counts: rows of classes outside the set, or without a pixel, are exactly 0.
 * accumulate = 1 adds the value the call would have written to what is there -- one double add per element of sums, one integer add per
 * count: a support set is pooled batch by batch.
 * Every reduction runs in a fixed order; the only atomics are integer adds into the count table (zeroed on the stream by the call): two
 * calls give bit-equal outputs.  Scalar arguments only: no host synchronisation, no allocation, capturable in a hipGraph.
 * szn_last_kernel(): proto_finalize_kernel; szn_prev_kernel(): proto_reduce_kernel (before them proto_tables_kernel in UNIT mode,
 * proto_cell_kernel and proto_gather_kernel).
 * workspace: szn_class_proto_workspace_bytes (0 for shapes szn_class_proto refuses), 16-byte aligned: the Gram table of the positions
 * (8 floats each), the per-cell coefficient tables [4][K] and the per-position table T [K] in double, up to 64 [K][E] partial sums.
 * Nothing in it grows with H * W * E or H * W * K.
 * SZN_ERR_ARG, before any launch: stride not 32 | 8; a size that is not positive; K > SZN_MAX_CLASSES; c0 < 0 or ldc < c0 + E; a crop
 * window larger than the deconv output; NULL coarse, labels, sums, counts or workspace; a workspace that is not 16-byte aligned; a class
 * in `classes` >= K; an empty `classes`; mode not SZN_PROTO_RAW | SZN_PROTO_UNIT; accumulate not 0 | 1.  SZN_ERR_UNSUPPORTED: an E too
 * large for LDS (the table pass stages four position vectors: E > 3840).                                                              */
#define SZN_PROTO_RAW  0
#define SZN_PROTO_UNIT 1
size_t szn_class_proto_workspace_bytes(int stride, int B, int h, int w, int E, int K);
int szn_class_proto(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                    const float* coarse, const int64_t* labels, const szn_class_set* classes, int mode, int accumulate,
                    double* sums, int64_t* counts, void* workspace, szn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SZN_H_ */
