// szn_calib.h -- the crossing-table scheme of the one-pass sweeps, shared by szn_fused_head.hip (szn_calib_head, szn_seen_sweep_head) and
// szn_conse_head.hip (szn_conse_head).
//
// A pixel is (t, a, b, bin): target, the class it takes below its crossing point, the class it takes from there on, and the first
// sweep value at which it takes b (n: never; include/szn.h).  XA [K][K][n + 1] counts (t, a, bin), XB (t, b, bin), both int64, zeroed by
// the call.  Integer atomics: the result does not depend on their order.  The sweep values travel as kernel arguments; the per-pixel
// search is a wave-uniform loop over them (scalar loads).
#pragma once
#include "szn_common.h"

namespace {

struct CalArgs {
    float gamma[SZN_CALIB_MAX_GAMMAS];
    unsigned long long* XA; unsigned long long* XB;
    int64_t* pred; int n, pred_index;
};

// the keys of a wave, equal ones combined: one atomic add of the popcount per distinct key and table.  A: the head's argument block (its
// class count K).  Key: t | a << 8 | b << 16 | bin << 24, or -1 where the pixel is not counted; every lane of the wave must call
template <typename A>
__device__ __forceinline__ void calib_count(const A& a, const CalArgs& c, int key, int lane) {
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const int k0 = __shfl(key, src, 64);
        const unsigned long long same = __ballot(key == k0);
        if (lane == src) {
            const unsigned long long cnt = (unsigned long long)__popcll(same);
            const int t = k0 & 255, ia = (k0 >> 8) & 255, ib = (k0 >> 16) & 255, bin = (k0 >> 24) & 127;
            atomicAdd(c.XA + ((size_t)t * a.K + ia) * (c.n + 1) + bin, cnt);
            atomicAdd(c.XB + ((size_t)t * a.K + ib) * (c.n + 1) + bin, cnt);
        }
        todo &= ~same;
    }
}

// hist[g][t][k] += sum_{bin > g} XA[t][k][bin] + sum_{bin <= g} XB[t][k][bin]: one thread per (t, k), running prefixes over the bins
__global__ __launch_bounds__(256) void calib_hist_kernel(const unsigned long long* __restrict__ XA,
                                                         const unsigned long long* __restrict__ XB, int K, int n,
                                                         int64_t* __restrict__ hist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K * K) return;
    const unsigned long long* xa = XA + (size_t)i * (n + 1);
    const unsigned long long* xb = XB + (size_t)i * (n + 1);
    unsigned long long above = 0, below = 0;
    for (int bin = 0; bin <= n; ++bin) above += xa[bin];
    for (int g = 0; g < n; ++g) {
        above -= xa[g];
        below += xb[g];
        hist[(size_t)g * K * K + i] += (int64_t)(above + below);
    }
}

}  // namespace
