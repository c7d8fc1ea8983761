// scan.cuh — prefix sums of u32 counts: the inclusive scan of one 256-lane workgroup in LDS (wg_scan_u32) and the
// exclusive scan of a device vector in three launches built on it (scan_u32).  Users: keygen's column and chunk offsets,
// the trace sort's digit histogram, the failing-row ranks of the R1CS check.
#pragma once
#include "hk_internal.h"

namespace hk {

constexpr u32 SCAN_U32_TILE = 256 * 16;      // u32 elements per block of the exclusive scan

// u32 of scratch scan_u32 needs for n elements (`tops`)
static inline size_t scan_u32_tops_len(size_t n) { return n / SCAN_U32_TILE + 1; }

#if defined(__HIPCC__)

// Inclusive scan of v over the 256 lanes of a workgroup (Hillis-Steele, 8 steps): returns v of lanes 0 .. tid summed; s[255]
// is the total.  s: 256 u32 of LDS.  Holds barriers: every lane of the workgroup calls it, from uniform control flow.
__device__ __forceinline__ u32 wg_scan_u32(u32* s, u32 tid, u32 v) {
    s[tid] = v;
    __syncthreads();
    HK_NOUNROLL for (u32 off = 1; off < 256; off <<= 1) {
        const u32 x = tid >= off ? s[tid - off] : 0u;
        __syncthreads();
        s[tid] += x;
        __syncthreads();
    }
    return s[tid];
}

// exclusive scan of n u32 in three launches: per tile (prefix within the tile into out, the tile's total into tops), over
// the tops (one block), then the tops added back
template <int UNUSED>
__global__ void __launch_bounds__(256) k_scan_u32_tile(const u32* __restrict__ in, u32* __restrict__ out, u32* __restrict__ tops,
                                                       u32 n) {
    __shared__ u32 s[256];
    const u32 tid = threadIdx.x;
    const u64 base = (u64)blockIdx.x * SCAN_U32_TILE + (u64)tid * 16;
    u32 v[16], sum = 0;
    HK_UNROLL for (int j = 0; j < 16; j++) {
        v[j] = base + j < n ? in[base + j] : 0u;
        sum += v[j];
    }
    u32 run = wg_scan_u32(s, tid, sum) - sum;
    HK_UNROLL for (int j = 0; j < 16; j++) {
        if (base + j < n) out[base + j] = run;
        run += v[j];
    }
    if (tid == 255) tops[blockIdx.x] = s[255];
}
template <int UNUSED>
__global__ void __launch_bounds__(256) k_scan_u32_tops(u32* __restrict__ tops, u32 nt) {
    __shared__ u32 s[256];
    const u32 tid = threadIdx.x;
    u32 carry = 0;
    for (u32 b = 0; b < nt; b += 256) {
        u32 i = b + tid;
        u32 v = i < nt ? tops[i] : 0u;
        u32 incl = wg_scan_u32(s, tid, v);
        if (i < nt) tops[i] = carry + incl - v;
        carry += s[255];
        __syncthreads();
    }
}
template <int UNUSED>
__global__ void __launch_bounds__(256) k_scan_u32_add(u32* __restrict__ out, const u32* __restrict__ tops, u32 n) {
    u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] += tops[k / SCAN_U32_TILE];
}

// out[i] = in[0] + ... + in[i - 1], i < n, on stream s.  tops: scan_u32_tops_len(n) u32 of scratch.  n == 0: nothing to
// write and nothing launched (a grid of zero blocks is a launch error).
static hk_status scan_u32(hipStream_t s, const u32* in, u32* out, u32* tops, u32 n) {
    if (n == 0) return HK_OK;
    u32 nt = (n + SCAN_U32_TILE - 1) / SCAN_U32_TILE;
    HK_LAUNCH((k_scan_u32_tile<0>), dim3(nt), dim3(256), 0, s, in, out, tops, n);
    HK_LAUNCH((k_scan_u32_tops<0>), dim3(1), dim3(256), 0, s, tops, nt);
    HK_LAUNCH((k_scan_u32_add<0>), dim3((n + 255) / 256), dim3(256), 0, s, out, (const u32*)tops, n);
    return HK_OK;
}

#endif  // __HIPCC__

}  // namespace hk
