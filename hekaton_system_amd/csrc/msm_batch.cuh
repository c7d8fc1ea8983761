// msm_batch.cuh — the digit sort and bucket pipeline of msm.cuh for a batch of proofs in lock-step (hk_prove_batch).
// Every kernel here is its single-proof twin with the proof index on grid.y (grid.x for the one-workgroup stages): the
// proof's slices of the sort / bucket buffers are selected by fixed per-proof strides and the twin's body runs on them
// unchanged (kbody/*.inc, shared source).  Sorted entries keep the encoding sign << 31 | group << gshift | i: they index
// their own proof's slice and never carry the proof.  `p` is the per-proof plan of the batch (msm_driver_impl.cuh
// msm_lane_plan_b: the chip's resident accumulate lanes split across the proofs).
//
// Per-proof strides (MsmSort::alloc_b / MsmRun::alloc_b): count, cursor NB; start NB + 1; sorted n W + 1; digits n W + 8;
// buckets NB + 1 (the reduction ticket rides behind them); boundary partials 2 T[0] and msm_p1_stride; reduction
// partials WP B / K.
#pragma once
#include "msm.cuh"

namespace hk {

HK_HD size_t msm_sorted_stride(const MsmPlan& p) { return (size_t)p.n * p.W + 1; }
HK_HD size_t msm_digits_stride(const MsmPlan& p) { return (size_t)p.n * p.W + 8; }
HK_HD size_t msm_p1_stride(const MsmPlan& p) { return p.n_levels > 1 ? 2ull * p.T[1] : 2ull; }

#if defined(__HIPCC__)

// proof b's scalars start scalar_stride_words u32 after proof b - 1's
template <class Fr>
__global__ void __launch_bounds__(MSM_SORT_THREADS)
k_msm_hist_b(const u32* __restrict__ scalars_all, size_t scalar_stride_words, int is_mont, MsmPlan p,
             u32* __restrict__ count_all, short* __restrict__ digits_all) {
    const size_t pr = blockIdx.y;
    const u32* __restrict__ scalars = scalars_all + pr * scalar_stride_words;
    u32* __restrict__ count = count_all + pr * p.NB;
    short* __restrict__ digits = digits_all + pr * msm_digits_stride(p);
#include "kbody/msm_hist.inc"
}

// one workgroup per proof (blockIdx.x)
template <int UNUSED>
__global__ void __launch_bounds__(1024)
k_msm_scan_b(const u32* __restrict__ count_all, u32* __restrict__ start_all, u32* __restrict__ cursor_all, u32 NB) {
    const size_t pr = blockIdx.x;
    const u32* __restrict__ count = count_all + pr * NB;
    u32* __restrict__ start = start_all + pr * (NB + 1);
    u32* __restrict__ cursor = cursor_all + pr * NB;
#include "kbody/msm_scan.inc"
}

template <class Fr>
__global__ void __launch_bounds__(MSM_SORT_THREADS)
k_msm_scatter_b(const short* __restrict__ digits_all, MsmPlan p, u32* __restrict__ cursor_all, u32* __restrict__ sorted_all) {
    const size_t pr = blockIdx.y;
    const short* __restrict__ digits = digits_all + pr * msm_digits_stride(p);
    u32* __restrict__ cursor = cursor_all + pr * p.NB;
    u32* __restrict__ sorted = sorted_all + pr * msm_sorted_stride(p);
#include "kbody/msm_scatter.inc"
}

// all proofs over ONE shared base table
template <class F>
__global__ void __launch_bounds__(64, AccumOcc<F>::waves)
k_msm_accum0_b(const Affine<F>* __restrict__ bases, u32 n_bases, u32 idx_off,
               const u32* __restrict__ sorted_all, const u32* __restrict__ start_all, MsmPlan p,
               XYZZ<F>* __restrict__ buckets_all, u32* __restrict__ pkeys_all, XYZZ<F>* __restrict__ ppts_all) {
    const size_t pr = blockIdx.y, s0 = 2ull * p.T[0];
    const u32* __restrict__ sorted = sorted_all + pr * msm_sorted_stride(p);
    const u32* __restrict__ start = start_all + pr * (p.NB + 1);
    XYZZ<F>* __restrict__ buckets = buckets_all + pr * (p.NB + 1);
    u32* __restrict__ pkeys = pkeys_all + pr * s0;
    XYZZ<F>* __restrict__ ppts = ppts_all + pr * s0;
#include "kbody/msm_accum0.inc"
}

// s_in / s_out: per-proof strides of the partial buffers this level reads / writes (2 T[0] or msm_p1_stride)
template <class F>
__global__ void __launch_bounds__(64)
k_msm_accum_lvl_b(int level, const u32* __restrict__ keys_in, const XYZZ<F>* __restrict__ pts_in, size_t s_in,
                  const u32* __restrict__ start, MsmPlan p, XYZZ<F>* __restrict__ buckets,
                  u32* __restrict__ keys_out, XYZZ<F>* __restrict__ pts_out, size_t s_out) {
    const size_t pr = blockIdx.y;
    u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    u32 E = start[pr * (p.NB + 1) + p.NB];
    LevelInfo li = msm_level_info(p, E, level);
    if (t >= li.active) return;
    msm_accum_level<F>(level, t, li, keys_in + pr * s_in, pts_in + pr * s_in, p, buckets + pr * (p.NB + 1),
                       keys_out + pr * s_out, pts_out + pr * s_out);
}

// one workgroup per proof (blockIdx.x)
template <class F>
__global__ void __launch_bounds__(MSM_TAIL_THREADS)
k_msm_accum_tail_b(int level0, u32* __restrict__ keys0_all, XYZZ<F>* __restrict__ pts0_all, u32* __restrict__ keys1_all,
                   XYZZ<F>* __restrict__ pts1_all, const u32* __restrict__ start_all, MsmPlan p,
                   XYZZ<F>* __restrict__ buckets_all) {
    const size_t pr = blockIdx.x, s0 = 2ull * p.T[0], s1 = msm_p1_stride(p);
    u32* __restrict__ keys0 = keys0_all + pr * s0;
    XYZZ<F>* __restrict__ pts0 = pts0_all + pr * s0;
    u32* __restrict__ keys1 = keys1_all + pr * s1;
    XYZZ<F>* __restrict__ pts1 = pts1_all + pr * s1;
    const u32* __restrict__ start = start_all + pr * (p.NB + 1);
    XYZZ<F>* __restrict__ buckets = buckets_all + pr * (p.NB + 1);
#include "kbody/msm_accum_tail.inc"
}

// every proof takes the tickets of its own slice (the u32 behind its buckets) and writes res_all[pr * res_stride]
template <class F>
__global__ void __launch_bounds__(MSM_REDUCE_THREADS)
k_msm_reduce_fused_b(XYZZ<F>* __restrict__ buckets_all, const u32* __restrict__ start_all, MsmPlan p,
                     XYZZ<F>* __restrict__ partial_all, XYZZ<F>* __restrict__ res_all, u32 res_stride) {
    const size_t pr = blockIdx.y;
    const XYZZ<F>* __restrict__ buckets = buckets_all + pr * (p.NB + 1);
    const u32* __restrict__ start = start_all + pr * (p.NB + 1);
    XYZZ<F>* __restrict__ partial = partial_all + pr * ((size_t)p.WP * (p.B / p.K));
    u32* __restrict__ ticket = reinterpret_cast<u32*>(buckets_all + pr * (p.NB + 1) + p.NB);
    XYZZ<F>* __restrict__ res = res_all + pr * res_stride;
#include "kbody/msm_reduce_fused.inc"
}

#endif  // __HIPCC__

}  // namespace hk
