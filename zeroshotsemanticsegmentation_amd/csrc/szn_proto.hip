// szn_proto.hip -- class prototypes by masked average pooling (szn_class_proto): per class the sum, over the pixels a label map gives
// it, of the upsampled + cropped score vector (SZN_PROTO_RAW) or of its unit vector (SZN_PROTO_UNIT), without ever materialising the
// (B,E,H,W) score.  The contract is stated in include/szn.h.
//
// The upsample is linear and every pixel of a stride-S cell blends the same four coarse vectors C_t (szn_upcell.h), so for a cell and a
// class k
//     sum_{p in cell, label_p = k} a_p s_p = sum_t ( sum_p a_p w_t(p) ) C_t,      a_p = 1 (RAW) | 1 / |s_p| (UNIT)
// The work per pixel is O(1): |s_p|^2 = sum_{t,u} w_t w_u (C_t . C_u) from the cell's Gram matrix, looked up in a per-position table
// (the fused head's stride-8 scheme, used here at both strides).  The E-wide work happens once per coarse position.
// Kernels, in launch order (every reduction runs in a fixed order, no floating-point atomics: two calls are bit-equal):
//   proto_tables_kernel    UNIT only: one wave per coarse position writes N[pos][5] = C_pos . C_nbr, nbr in {self, E, S, SE, SW} (64 strided
//                          fp32 partial chains + xor butterfly: fh_tables_kernel's chains)
//   proto_cell_kernel<S>   S = 8: one wave per cell; S = 32: one block per cell.  Per pixel the label, the weights, |s|; then the wave
//                          walks the distinct classes its pixels carry and reduces the four tap coefficients of each in double (xor
//                          butterfly; lanes, then waves through LDS).  Writes the cell's table A[cell][4][K] (zeros for the classes that are
//                          absent) and adds the pixel counts to a [K][2] integer table (integer atomics: order-free)
//   proto_gather_kernel    T[pos][k] = the four cells that use pos as a tap, combine4 in tap order
//   proto_reduce_kernel    sums = T^t x coarse in double: a block takes a chunk of positions, 16 classes and 64 channels; lanes span the
//                          channels, each wave walks its share of the chunk in ascending order (zero coefficients are skipped), the four
//                          waves meet in LDS (combine4) -> part[chunk][K][E]
//   proto_finalize_kernel  the chunks in ascending order, then the single add of accumulate = 1; the counts
#include "szn_upcell.h"

namespace {

constexpr int kNLd = 8;          // row pitch of the Gram table N (5 used)
constexpr int kRedK = 16;        // classes per block of proto_reduce_kernel
constexpr int kMaxChunks = 64;   // position chunks of proto_reduce_kernel

struct ProtoArgs {
    const int64_t* labels;
    const float* N;                  // [B h w][kNLd]
    double* cellA;                   // [B (h+1) (w+1)][4][K]
    unsigned long long* cnt;         // [K][2], zeroed by the call
    ClassBits set;
    int B, h, w, H, W, crop, K, unit;
};

__global__ __launch_bounds__(256) void proto_tables_kernel(const float* __restrict__ coarse, float* __restrict__ N, int B, int h, int w,
                                                           int E, int ldc, int c0) {
    extern __shared__ __attribute__((aligned(16))) float sm[];            // [4 waves][E]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long npos = (long)B * h * w;
    const long pos = (long)blockIdx.x * 4 + wave;
    const bool ok = pos < npos;
    const long p = ok ? pos : 0;
    const int b = (int)(p / (h * w)), r = (int)(p % (h * w));
    const int i = r / w, j = r % w;
    const float* cv = coarse + (size_t)p * ldc + c0;
    float* Cs = sm + wave * E;
    for (int c = lane; c < E; c += 64) Cs[c] = cv[c];
    __syncthreads();
    const int di[5] = {0, 0, 1, 1, 1}, dj[5] = {0, 1, 0, 1, -1};
#pragma unroll
    for (int n = 0; n < 5; ++n) {
        const int ni = i + di[n], nj = j + dj[n];
        float q = 0.f;
        if (ni < h && nj >= 0 && nj < w) {                                  // wave-uniform
            const float* nv = coarse + (((size_t)b * h + ni) * w + nj) * ldc + c0;
            for (int c = lane; c < E; c += 64) q = fmaf(Cs[c], nv[c], q);
        }
        q = wave_sum(q);
        if (ok && lane == 0) N[(size_t)pos * kNLd + n] = q;
    }
}

// |s|^2 of one pixel from the cell's Gram matrix: the fused head's chain over the 16 (t, u) pairs
__device__ __forceinline__ float proto_ss(const float (&wt)[4], const float (&Q)[16]) {
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) ss = fmaf(wt[t] * wt[u], Q[t * 4 + u], ss);
    return ss;
}

template <int S>
__global__ __launch_bounds__(256) void proto_cell_kernel(const ProtoArgs a) {
    constexpr bool kBlockCell = S * S > 64;           // S = 32: the block shares one cell; S = 8: one cell per wave
    static_assert(S * S == 64 || (S * S) % 256 == 0, "every lane of a wave takes the same number of turns");
    extern __shared__ __attribute__((aligned(16))) double smd[];          // [4 waves][4][K] doubles | [4 waves][K][2] unsigned
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = a.K;
    const int cells_w = a.w + 1, cells = (a.h + 1) * cells_w;
    const long ncell = (long)a.B * cells;
    const long cid = kBlockCell ? (long)blockIdx.x : (long)blockIdx.x * 4 + wave;
    const bool ok = cid < ncell;
    const long cc = ok ? cid : 0;
    const int b = (int)(cc / cells), cell = (int)(cc % cells);
    const int I = cell / cells_w, J = cell % cells_w;
    double* wA = smd + (size_t)wave * 4 * K;
    unsigned* wC = (unsigned*)(smd + (size_t)16 * K) + (size_t)wave * 2 * K;
    for (int i = lane; i < 4 * K; i += 64) wA[i] = 0.0;
    for (int i = lane; i < 2 * K; i += 64) wC[i] = 0u;

    // the cell's Gram matrix from the position table (UNIT): entry (t, u), t <= u, lives in the row of the lower tap
    float Q[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) Q[v] = 0.f;
    if (a.unit) {
        long tp[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) tp[t] = tap_pos(b, a.h, a.w, I, J, t);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int u = t; u < 4; ++u) {
                // (t, u) -> neighbour slot of the lower tap: self, E, S, SE | (1,2) SW, (1,3) S | (2,3) E
                const int slot = (t == u) ? 0 : (t == 0 ? u : (t == 1 ? (u == 2 ? 4 : 2) : 1));
                const float q = (tp[t] >= 0 && tp[u] >= 0) ? a.N[(size_t)tp[t] * kNLd + slot] : 0.f;
                Q[t * 4 + u] = q;
                Q[u * 4 + t] = q;
            }
    }
    __syncthreads();

    for (int q = kBlockCell ? tid : lane; q < S * S; q += kBlockCell ? 256 : 64) {
        const int ty = q / S, tx = q % S;
        const int y = S * I + ty - a.crop, x = S * J + tx - a.crop;         // image coords y = Y - crop
        bool part = false, contrib = false;
        int k = -1;
        double cf[4] = {0.0, 0.0, 0.0, 0.0};
        if (ok && y >= 0 && y < a.H && x >= 0 && x < a.W) {
            const long l = a.labels[((size_t)b * a.H + y) * a.W + x];
            if (l >= 0 && l < K && in_set(a.set, l)) {
                part = true;
                k = (int)l;
                float wt[4];
                cell_weights<S>(ty, tx, wt);
                if (a.unit) {
                    const float sn = sqrtf(proto_ss(wt, Q));
                    contrib = isfinite(sn) && sn > 0.f;
                    if (contrib) {
                        const double inv = 1.0 / (double)sn;
#pragma unroll
                        for (int t = 0; t < 4; ++t) cf[t] = (double)wt[t] * inv;
                    }
                } else {
                    contrib = true;
#pragma unroll
                    for (int t = 0; t < 4; ++t) cf[t] = (double)wt[t];
                }
            }
        }
        // the distinct classes of this wave's pixels, in the order of their first lane
        unsigned long long todo = __ballot(part);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            const int kl = __shfl(k, src, 64);
            const bool mine = part && k == kl;
            const unsigned long long who = __ballot(mine);
            const unsigned n_part = (unsigned)__popcll(who), n_con = (unsigned)__popcll(__ballot(mine && contrib));
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double s = wave_sum_d(mine ? cf[t] : 0.0);
                if (lane == 0) wA[t * K + kl] += s;
            }
            if (lane == 0) { wC[2 * kl] += n_part; wC[2 * kl + 1] += n_con; }
            todo &= ~who;
        }
    }
    __syncthreads();
    if (kBlockCell) {
        double* out = a.cellA + (size_t)cid * 4 * K;
        for (int i = tid; i < 4 * K; i += 256) out[i] = combine4(smd[i], smd[4 * K + i], smd[8 * K + i], smd[12 * K + i]);
        const unsigned* C0 = (const unsigned*)(smd + (size_t)16 * K);
        for (int i = tid; i < 2 * K; i += 256) {
            const unsigned long long c = (unsigned long long)C0[i] + C0[2 * K + i] + C0[4 * K + i] + C0[6 * K + i];
            if (c) atomicAdd(a.cnt + i, c);
        }
    } else if (ok) {
        double* out = a.cellA + (size_t)cid * 4 * K;
        for (int i = lane; i < 4 * K; i += 64) out[i] = wA[i];
        for (int i = lane; i < 2 * K; i += 64)
            if (wC[i]) atomicAdd(a.cnt + i, (unsigned long long)wC[i]);
    }
}

__global__ __launch_bounds__(256) void proto_gather_kernel(const double* __restrict__ cellA, double* __restrict__ T, int B, int h, int w,
                                                           int K) {
    const long n = (long)B * h * w * K;
    const int cells_w = w + 1, cells = (h + 1) * cells_w;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < n; g += (long)gridDim.x * 256) {
        const long pos = g / K;
        const int k = (int)(g - pos * K);
        const int b = (int)(pos / (h * w)), r = (int)(pos % (h * w));
        const int i = r / w, j = r % w;
        double v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const long cell = (long)b * cells + (long)tap_cell_I(i, t) * cells_w + tap_cell_J(j, t);
            v[t] = cellA[((size_t)cell * 4 + t) * K + k];
        }
        T[g] = combine4(v[0], v[1], v[2], v[3]);
    }
}

// grid (chunks, ceil(K / kRedK), ceil(E / 64)); per_wave = positions one wave walks
__global__ __launch_bounds__(256) void proto_reduce_kernel(const double* __restrict__ T, const float* __restrict__ coarse,
                                                           double* __restrict__ part, long npos, int per_wave, int K, int E, int ldc,
                                                           int c0) {
    __shared__ double red[4][kRedK][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k0 = blockIdx.y * kRedK;
    const int e = blockIdx.z * 64 + lane;
    const bool e_ok = e < E;                          // lanes beyond E read nothing: the padding channels never enter
    const long p0 = ((long)blockIdx.x * 4 + wave) * per_wave;
    const long p1 = p0 + per_wave < npos ? p0 + per_wave : npos;
    double acc[kRedK];
#pragma unroll
    for (int kk = 0; kk < kRedK; ++kk) acc[kk] = 0.0;
    for (long p = p0; p < p1; ++p) {
        const double* Tr = T + (size_t)p * K + k0;
        const double c = e_ok ? (double)coarse[(size_t)p * ldc + c0 + e] : 0.0;
#pragma unroll
        for (int kk = 0; kk < kRedK; ++kk) {
            if (k0 + kk < K) {                        // wave-uniform, like the test on the coefficient
                const double tv = Tr[kk];
                if (tv != 0.0) acc[kk] = fma(tv, c, acc[kk]);
            }
        }
    }
#pragma unroll
    for (int kk = 0; kk < kRedK; ++kk) red[wave][kk][lane] = acc[kk];
    __syncthreads();
    for (int i = threadIdx.x; i < kRedK * 64; i += 256) {
        const int kk = i >> 6, l = i & 63;
        const int k = k0 + kk, ee = blockIdx.z * 64 + l;
        if (k < K && ee < E)
            part[((size_t)blockIdx.x * K + k) * E + ee] = combine4(red[0][kk][l], red[1][kk][l], red[2][kk][l], red[3][kk][l]);
    }
}

__global__ __launch_bounds__(256) void proto_finalize_kernel(const double* __restrict__ part, const unsigned long long* __restrict__ cnt,
                                                             int chunks, int K, int E, int accumulate, double* __restrict__ sums,
                                                             int64_t* __restrict__ counts) {
    const long n = (long)K * E;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < n; g += (long)gridDim.x * 256) {
        double v = 0.0;
        for (int c = 0; c < chunks; ++c) v += part[(size_t)c * n + g];
        sums[g] = accumulate ? sums[g] + v : v;
    }
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < 2 * K; i += 256) counts[i] = (accumulate ? counts[i] : 0) + (int64_t)cnt[i];
}

struct ProtoWorkspace { size_t N, cnt, cellA, T, part, bytes; int chunks, per_wave; };       // byte offsets
ProtoWorkspace proto_workspace(int B, int h, int w, int E, int K) {
    const size_t npos = (size_t)B * h * w, cells = (size_t)B * (h + 1) * (w + 1);
    ProtoWorkspace L;
    long chunks = ((long)npos + 63) / 64;             // at least 16 positions per wave before a second chunk pays
    L.chunks = (int)(chunks < 1 ? 1 : (chunks > kMaxChunks ? kMaxChunks : chunks));
    L.per_wave = (int)((npos + (size_t)L.chunks * 4 - 1) / ((size_t)L.chunks * 4));
    L.N = 0;
    L.cnt = align256(L.N + npos * kNLd * sizeof(float));
    L.cellA = align256(L.cnt + (size_t)K * 2 * sizeof(unsigned long long));
    L.T = align256(L.cellA + cells * 4 * K * sizeof(double));
    L.part = align256(L.T + npos * K * sizeof(double));
    L.bytes = align256(L.part + (size_t)L.chunks * K * E * sizeof(double));
    return L;
}

// what szn_class_proto and its workspace query refuse about sizes; 0 = fine
const char* proto_bad_geometry(int stride, int B, int h, int w, int E, int K) {
    if (stride != 32 && stride != 8) return "stride must be 8 or 32";
    if (B <= 0 || h <= 0 || w <= 0 || E <= 0 || K <= 0) return "a size that is not positive";
    if (K > SZN_MAX_CLASSES) return "K above SZN_MAX_CLASSES";
    // h * w stays an int in the kernels; one block per cell at stride 32, one wave per position in the table pass
    if (h > 32767 || w > 32767 || (long)B * (h + 1) * (w + 1) > 0x7fffffffL) return "the map is too large (h, w <= 32767, B (h+1) (w+1) < 2^31)";
    return nullptr;
}

}  // namespace

extern "C" size_t szn_class_proto_workspace_bytes(int stride, int B, int h, int w, int E, int K) {
    if (proto_bad_geometry(stride, B, h, w, E, K)) return 0;
    if ((size_t)4 * E * sizeof(float) > 60 * 1024) return 0;
    return proto_workspace(B, h, w, E, K).bytes;
}

extern "C" int szn_class_proto(int stride, int B, int h, int w, int E, int ldc, int c0, int H, int W, int crop, int K,
                               const float* coarse, const int64_t* labels, const szn_class_set* classes, int mode, int accumulate,
                               double* sums, int64_t* counts, void* workspace, szn_stream_t stream) {
    if (const char* why = proto_bad_geometry(stride, B, h, w, E, K)) SZN_FAIL(SZN_ERR_ARG, "class_proto: %s", why);
    if (!coarse || !labels || !sums || !counts || !workspace)
        SZN_FAIL(SZN_ERR_ARG, "class_proto: coarse, labels, sums, counts and workspace are required");
    if (c0 < 0 || ldc < c0 + E || H <= 0 || W <= 0 || H > 32767 || W > 32767 || crop < 0)
        SZN_FAIL(SZN_ERR_ARG, "class_proto: bad argument (ldc %d, c0 %d, E %d, image %d x %d, crop %d)", ldc, c0, E, H, W, crop);
    if (H + crop > stride * h + stride || W + crop > stride * w + stride)
        SZN_FAIL(SZN_ERR_ARG, "class_proto: crop window exceeds the deconv output");
    if (((uintptr_t)workspace) & 15) SZN_FAIL(SZN_ERR_ARG, "class_proto: workspace must be 16-B aligned");
    if (mode != SZN_PROTO_RAW && mode != SZN_PROTO_UNIT) SZN_FAIL(SZN_ERR_ARG, "class_proto: mode %d is neither SZN_PROTO_RAW nor SZN_PROTO_UNIT", mode);
    if (accumulate != 0 && accumulate != 1) SZN_FAIL(SZN_ERR_ARG, "class_proto: accumulate %d must be 0 or 1", accumulate);
    ClassBits set = class_bits(classes);
    if (classes) {
        if (!class_bits_any(set)) SZN_FAIL(SZN_ERR_ARG, "class_proto: the class set is empty");
        if (!class_bits_fit(set, K)) SZN_FAIL(SZN_ERR_ARG, "class_proto: the class set names a class >= K = %d", K);
    } else {
        for (int k = 0; k < K; ++k) set.w[k >> 6] |= 1ull << (k & 63);
    }
    if ((size_t)4 * E * sizeof(float) > 60 * 1024) SZN_FAIL(SZN_ERR_UNSUPPORTED, "class_proto: E=%d too large for LDS", E);

    hipStream_t st = (hipStream_t)stream;
    const ProtoWorkspace L = proto_workspace(B, h, w, E, K);
    char* ws = (char*)workspace;
    const long npos = (long)B * h * w, ncell = (long)B * (h + 1) * (w + 1);
    ProtoArgs a{};
    a.labels = labels; a.N = (const float*)(ws + L.N); a.cellA = (double*)(ws + L.cellA); a.cnt = (unsigned long long*)(ws + L.cnt);
    a.set = set; a.B = B; a.h = h; a.w = w; a.H = H; a.W = W; a.crop = crop; a.K = K; a.unit = mode == SZN_PROTO_UNIT;
    double* T = (double*)(ws + L.T);
    double* part = (double*)(ws + L.part);
    if (hipMemsetAsync(ws + L.cnt, 0, (size_t)K * 2 * sizeof(unsigned long long), st) != hipSuccess)
        SZN_FAIL(SZN_ERR_LAUNCH, "class_proto: clearing the counts failed");
    if (a.unit) {
        hipLaunchKernelGGL(proto_tables_kernel, dim3((unsigned)((npos + 3) / 4)), dim3(256), (size_t)4 * E * sizeof(float), st, coarse,
                           (float*)(ws + L.N), B, h, w, E, ldc, c0);
        SZN_CHECK_LAUNCH("proto_tables_kernel");
    }
    const size_t lds = (size_t)16 * K * sizeof(double) + (size_t)8 * K * sizeof(unsigned);
    if (stride == 32) hipLaunchKernelGGL(proto_cell_kernel<32>, dim3((unsigned)ncell), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(proto_cell_kernel<8>, dim3((unsigned)((ncell + 3) / 4)), dim3(256), lds, st, a);
    SZN_CHECK_LAUNCH("proto_cell_kernel");
    hipLaunchKernelGGL(proto_gather_kernel, dim3(szn_grid_for(npos * K)), dim3(256), 0, st, (const double*)a.cellA, T, B, h, w, K);
    SZN_CHECK_LAUNCH("proto_gather_kernel");
    hipLaunchKernelGGL(proto_reduce_kernel, dim3((unsigned)L.chunks, (unsigned)((K + kRedK - 1) / kRedK), (unsigned)((E + 63) / 64)),
                       dim3(256), 0, st, (const double*)T, coarse, part, npos, L.per_wave, K, E, ldc, c0);
    SZN_CHECK_LAUNCH("proto_reduce_kernel");
    hipLaunchKernelGGL(proto_finalize_kernel, dim3(szn_grid_for((long)K * E)), dim3(256), 0, st, (const double*)part,
                       (const unsigned long long*)a.cnt, L.chunks, K, E, accumulate, sums, counts);
    SZN_CHECK_LAUNCH("proto_finalize_kernel");
    return SZN_OK;
}
