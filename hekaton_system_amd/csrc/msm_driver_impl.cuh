// msm_driver_impl.cuh — definitions for msm_driver.cuh (see there).
#pragma once
#include "msm_driver.cuh"
#include "fixed_base.cuh"
#include "endo.cuh"
#include "scan.cuh"

namespace hk {

template <class Fr>
void MsmSort<Fr>::alloc(Carve& c, const MsmPlan& p, SortBufs* out, u32 batch) {
    out->count = c.n<u32>((size_t)p.NB * batch);
    out->start = c.n<u32>((size_t)(p.NB + 1) * batch);
    out->cursor = c.n<u32>((size_t)p.NB * batch);
    out->sorted = c.n<u32>(msm_sorted_stride(p) * batch);
    out->digits = c.n<short>(msm_digits_stride(p) * batch);
}

template <class Fr>
void MsmSort<Fr>::alloc_sub(Carve& c, const MsmPlan& src, const MsmPlan& p, SortBufs* out, u32 batch) {
    const size_t tiles = (size_t)msm_sub_tiles(src) * batch;
    out->count = nullptr;
    out->cursor = nullptr;
    out->digits = nullptr;
    out->start = c.n<u32>((size_t)(p.NB + 1) * batch);
    out->sorted = c.n<u32>(msm_sorted_stride(p) * batch);
    out->mask = c.n<u64>(tiles * MSM_SUB_WORDS);
    out->tcount = c.n<u32>(tiles);
    out->toff = c.n<u32>(tiles);
    out->tops = c.n<u32>(scan_u32_tops_len(tiles));
}

template <class Fr>
hk_status MsmSort<Fr>::sublist(hipStream_t s, const MsmPlan& src, const SortBufs& sb_src, const MsmPlan& dst, const u32* rank,
                               const SortBufs& sb_dst, u32 batch) {
    if (batch == 0 || batch > 65535u) return HK_ERR_ARG;
    // the sub-list reuses the source's digits: same windows, same buckets; and it is no longer than the source
    if (dst.c != src.c || dst.W != src.W || dst.WP != src.WP || dst.NB != src.NB || dst.n > src.n) return HK_ERR_ARG;
    const u32 tiles = msm_sub_tiles(src);
    if ((u64)tiles * batch > 0xffffffffull) return HK_ERR_ARG;
    const dim3 gt((tiles + MSM_SUB_THREADS / 64 - 1) / (MSM_SUB_THREADS / 64), batch);
    HK_LAUNCH((k_msm_sub_mark<0>), gt, dim3(MSM_SUB_THREADS), 0, s, (const u32*)sb_src.sorted,
              (const u32*)sb_src.start, src, rank, sb_dst.mask, sb_dst.tcount);
    HK_TRY(scan_u32(s, sb_dst.tcount, sb_dst.toff, sb_dst.tops, tiles * batch));
    HK_LAUNCH((k_msm_sub_emit<0>), gt, dim3(MSM_SUB_THREADS), 0, s, (const u32*)sb_src.sorted, src, rank,
              (const u64*)sb_dst.mask, (const u32*)sb_dst.toff, dst, sb_dst.sorted);
    HK_LAUNCH((k_msm_sub_starts<0>), dim3((src.NB + 1 + 255) / 256, batch), dim3(256), 0, s,
              (const u32*)sb_src.start, src, (const u64*)sb_dst.mask, (const u32*)sb_dst.toff, sb_dst.start);
    return HK_OK;
}

template <class Fr>
hk_status MsmSort<Fr>::run(hipStream_t s, const MsmPlan& p, const u32* scalars_d, int is_mont,
                           const SortBufs& sb, bool count_is_zero, u32 batch, size_t scalar_stride) {
    if (p.NB > (u32)MSM_LDS_COUNTERS || p.c < 3 || p.c > 16) return HK_ERR_ARG;       // digits are stored as int16
    if (batch == 0 || batch > 65535u) return HK_ERR_ARG;
    if (!count_is_zero) HK_HIP(hipMemsetAsync(sb.count, 0, sizeof(u32) * p.NB * batch, s));
    u32 blocks = (p.n + p.chunk - 1) / p.chunk;
    if (blocks == 0) blocks = 1;
    const size_t words = scalar_stride * (sizeof(Fr) / sizeof(u32));
    HK_LAUNCH((k_msm_hist<Fr>), dim3(blocks, batch), dim3(MSM_SORT_THREADS), 0, s,
              scalars_d, words, is_mont, p, sb.count, sb.digits);
    HK_LAUNCH((k_msm_scan<0>), dim3(batch), dim3(1024), 0, s, sb.count, sb.start, sb.cursor, p.NB);
    HK_LAUNCH((k_msm_scatter<Fr>), dim3(blocks, batch), dim3(MSM_SORT_THREADS), 0, s,
              (const short*)sb.digits, p, sb.cursor, sb.sorted);
    return HK_OK;
}

// accumulate schedule for this coordinate field: as many lanes as the kernel keeps resident
// (AccumOcc<F>::waves per SIMD x 1024 SIMDs x 64), so the sorted list is consumed in ONE balanced round; a batch of
// proofs side by side splits those lanes (they are not multiplied by the batch)
template <class F>
static inline MsmPlan msm_lane_plan(const MsmPlan& p0, u32 batch = 1) {
    MsmPlan p = p0;
    u32 lanes = (u32)AccumOcc<F>::waves * 65536u / (batch ? batch : 1u);
    msm_set_lanes(p, lanes ? lanes : 1u);
    return p;
}

template <class F>
void MsmRun<F>::alloc(Carve& c, const MsmPlan& p0, Bufs* out, u32 batch) {
    const MsmPlan p = msm_lane_plan<F>(p0, batch);
    const size_t n0 = 2ull * p.T[0], n1 = msm_p1_stride(p);
    out->buckets = c.n<XYZZ<F>>((size_t)(p.NB + 1) * batch);     // + one slot: the reduction ticket
    out->pkeys[0] = c.n<u32>(n0 * batch);
    out->ppts[0] = c.n<XYZZ<F>>(n0 * batch);
    out->pkeys[1] = c.n<u32>(n1 * batch);
    out->ppts[1] = c.n<XYZZ<F>>(n1 * batch);
    out->red = c.n<XYZZ<F>>((size_t)p.WP * (p.B / p.K) * batch);
    out->wsum = c.n<XYZZ<F>>((size_t)p.WP * batch);
}

template <class F>
hk_status MsmRun<F>::run(hipStream_t s, const MsmPlan& p0, const Affine<F>* table, u32 n_bases, u32 idx_off,
                         const SortBufs& sb, const Bufs& b, XYZZ<F>* result_d,
                         hipEvent_t ev0, hipEvent_t ev1, u32 batch, u32 res_stride) {
    if (batch == 0 || batch > 65535u) return HK_ERR_ARG;
    const MsmPlan p = msm_lane_plan<F>(p0, batch);
    const size_t n0 = 2ull * p.T[0], n1 = msm_p1_stride(p);
    // no memset of the buckets (4 - 8 MB per MSM): k_msm_accum0 writes every bucket that has entries and clears the
    // ticket, the reductions skip the empty ones
    // with profiling on, ev0/ev1 take the kernel's own start/stop timestamps, so
    // the figure agrees with rocprofv3's kernel trace even when other lanes share the hardware queues
    dim3 g0((p.T[0] + 63) / 64, batch);
    HK_LAUNCH_TIMED((k_msm_accum0<F>), g0, dim3(64), 0, s, ev0, ev1,
                    table, n_bases, idx_off, sb.sorted, sb.start, p, b.buckets, b.pkeys[0], b.ppts[0]);
    u32 k = 1;
    for (; k < p.n_levels && p.T[k] > (u32)MSM_TAIL_THREADS; k++) {
        int in = (k - 1) & 1, out = k & 1;
        HK_LAUNCH((k_msm_accum_lvl<F>), dim3((p.T[k] + 63) / 64, batch), dim3(64), 0, s,
                  (int)k, b.pkeys[in], b.ppts[in], in ? n1 : n0, sb.start, p, b.buckets, b.pkeys[out], b.ppts[out],
                  out ? n1 : n0);
    }
    if (k < p.n_levels) {                                   // the remaining levels fit one workgroup each: one launch
        HK_LAUNCH((k_msm_accum_tail<F>), dim3(batch), dim3(MSM_TAIL_THREADS), 0, s, (int)k, b.pkeys[0], b.ppts[0],
                  b.pkeys[1], b.ppts[1], sb.start, p, b.buckets);
    }
    u32 J = p.B / p.K;
    if (p.WP == 1) {
        u32 blocks = (J + MSM_REDUCE_THREADS - 1) / MSM_REDUCE_THREADS;
        HK_LAUNCH((k_msm_reduce_fused<F>), dim3(blocks, batch), dim3(MSM_REDUCE_THREADS), 0, s, b.buckets, sb.start, p,
                  b.red, result_d, res_stride);
    } else {
        // several windows per group (the HK_MSM_WP experiment only): the three-launch reduction of each proof's slices
        const size_t rs = (size_t)p.WP * J;
        for (u32 pr = 0; pr < batch; pr++) {
            const XYZZ<F>* bk = b.buckets + (size_t)pr * (p.NB + 1);
            const u32* st = sb.start + (size_t)pr * (p.NB + 1);
            HK_LAUNCH((k_msm_bucket_reduce<F>), dim3((p.WP * J + 63) / 64), dim3(64), 0, s, bk, st, p, b.red + pr * rs);
            HK_LAUNCH((k_msm_window_sum<F>), dim3(p.WP), dim3(MSM_WSUM_THREADS), 0, s, b.red + pr * rs, p,
                      b.wsum + (size_t)pr * p.WP);
            HK_LAUNCH((k_msm_final<F>), dim3(1), dim3(64), 0, s, b.wsum + (size_t)pr * p.WP, p,
                      result_d + (size_t)pr * res_stride);
        }
    }
    return HK_OK;
}

template <class F>
hk_status MsmRun<F>::build_tables(hipStream_t s, Affine<F>* table, u32 n, u32 groups, u32 shift_bits) {
    if (groups <= 1 || n == 0) return HK_OK;
    HK_LAUNCH((k_msm_build_tables<F>), dim3((n + 63) / 64), dim3(64), 0, s, table, n, groups,
              shift_bits);
    return HK_OK;
}

template <class F>
hk_status MsmRun<F>::to_affine(hipStream_t s, const XYZZ<F>* in, Affine<F>* out, u32 n) {
    HK_LAUNCH((k_to_affine<F>), dim3((n + 63) / 64), dim3(64), 0, s, in, out, n);
    return HK_OK;
}

template <class F>
hk_status MsmRun<F>::batch_affine(hipStream_t s, const XYZZ<F>* in, Affine<F>* out, F* pref, u32 n) {
    if (n == 0) return HK_OK;
    u32 chunk = (n + 65535) / 65536;                       // 1 up to one wave per SIMD, then longer serial runs per lane
    if (chunk > (u32)FB_CHUNK) chunk = FB_CHUNK;
    u32 lanes = (n + chunk - 1) / chunk;
    HK_LAUNCH((k_batch_affine<F>), dim3((lanes + 63) / 64), dim3(64), 0, s, in, out, pref, n, chunk);
    return HK_OK;
}

// the K-lane sweep (endo.cuh): for G2 with few elements every Fq2 value on a quad of lanes (Fp2Q), else one lane per value
template <class Fr, class P, bool UNIFORM>
static inline hk_status launch_mul_split(hipStream_t s, const SplitVecs<Fp2<P>>& v, u32 k, const Fr* scalars, u32 neg_mask, u32 n,
                                         const EndoSplit<4>& E, Jac<Fp2<P>>* tab, XYZZ<Fp2<P>>* xy, int scalars_mont = 1) {
    const bool no_quad = getenv("HK_ENDO_NO_QUAD") != nullptr;
    u32 lanes = n * 4;
    if (!no_quad && (size_t)lanes * 4 <= SPLIT_MAX_LANES) {
        typedef Fp2Q<P> Q;                                    // same memory layout as Fp2<P>
        SplitVecs<Q> vq;
        for (int y = 0; y < FOLD_MAX; y++) { vq.lo[y] = (const Affine<Q>*)v.lo[y]; vq.pts[y] = (const Affine<Q>*)v.pts[y]; }
        vq.pts_mod = v.pts_mod;
        HK_LAUNCH((k_points_mul_split<Fr, Q, UNIFORM>), dim3((lanes * 4 + 63) / 64, k), dim3(64), 0, s, vq, scalars,
                  neg_mask, n, E, (Jac<Q>*)tab, (XYZZ<Q>*)xy, scalars_mont);
    } else {
        HK_LAUNCH((k_points_mul_split<Fr, Fp2<P>, UNIFORM>), dim3((lanes + 63) / 64, k), dim3(64), 0, s, v, scalars,
                  neg_mask, n, E, tab, xy, scalars_mont);
    }
    return HK_OK;
}
template <class Fr, class P, bool UNIFORM>
static inline hk_status launch_mul_split(hipStream_t s, const SplitVecs<Fp<P>>& v, u32 k, const Fr* scalars, u32 neg_mask, u32 n,
                                         const EndoSplit<2>& E, Jac<Fp<P>>* tab, XYZZ<Fp<P>>* xy, int scalars_mont = 1) {
    HK_LAUNCH((k_points_mul_split<Fr, Fp<P>, UNIFORM>), dim3((n * 2 + 63) / 64, k), dim3(64), 0, s, v, scalars,
              neg_mask, n, E, tab, xy, scalars_mont);
    return HK_OK;
}

template <class F>
hk_status MsmRun<F>::scalar_mul_each(hipStream_t s, const Affine<F>* pts, const void* scalars_mont, u32 n,
                                     XYZZ<F>* xy, F* pref, Affine<F>* out, XYZZ<F>* tab) {
    typedef typename ScalarOf<F>::type Fr;
    if (n == 0) return HK_OK;
    static const bool plain = getenv("HK_SCALAR_MUL_PLAIN") != nullptr;      // the 254-step ladder (A/B, debugging)
    const bool one_lane = getenv("HK_ENDO_ONE_LANE") != nullptr;             // never K lanes per element (A/B, tests)
    if (tab && !plain && !one_lane && (size_t)n * EndoOf<F>::K <= SPLIT_MAX_LANES) {
        // short vector: K lanes per element, 4-bit windows, Jacobian chain (endo.cuh)
        static const auto E = EndoOf<F>::split();
        SplitVecs<F> v = {};
        v.pts[0] = pts;
        HK_TRY((launch_mul_split<Fr, typename F::Params, false>(s, v, 1u, (const Fr*)scalars_mont, 0u, n, E, reinterpret_cast<Jac<F>*>(tab), xy)));
    } else if (tab && !plain) {
        // scalars split on the device along phi / psi: one shared chain of 131 (G1) / 68 (G2) doublings (endo.cuh)
        static const auto E = EndoOf<F>::split();
        HK_LAUNCH((k_scalar_mul_endo<Fr, F>), dim3((n + 63) / 64), dim3(64), 0, s, pts, (const Fr*)scalars_mont, n, E,
                  tab, xy);
    } else {
        HK_LAUNCH((k_scalar_mul_each<Fr, F>), dim3((n + 63) / 64), dim3(64), 0, s, pts, (const Fr*)scalars_mont,
                  n, xy);
    }
    return batch_affine(s, xy, out, pref, n);
}

// sum_i s_i P_i for a SHORT vector without tables: n element-wise products over the endomorphism (k_points_mul_split),
// then one workgroup's sum (k_points_sum_seg over one segment).  scalars: Montgomery (mont != 0) or canonical integers.
template <class F>
hk_status MsmRun<F>::small_msm(hipStream_t s, const Affine<F>* bases, const void* scalars, int mont, u32 n, XYZZ<F>* tab,
                               XYZZ<F>* xy, XYZZ<F>* result) {
    typedef typename ScalarOf<F>::type Fr;
    if (n == 0 || (size_t)n * EndoOf<F>::K > SPLIT_MAX_LANES) return HK_ERR_ARG;
    static const auto E = EndoOf<F>::split();
    SplitVecs<F> v = {};
    v.pts[0] = bases;
    HK_TRY((launch_mul_split<Fr, typename F::Params, false>(s, v, 1u, (const Fr*)scalars, 0u, n, E, reinterpret_cast<Jac<F>*>(tab), xy, mont ? 1 : 0)));
    HK_LAUNCH((k_points_sum_seg<F, PointsSum<F>::THREADS>), dim3(1), dim3(PointsSum<F>::THREADS), 0, s, (const XYZZ<F>*)xy, n, result);
    return HK_OK;
}

// batch x seg element-wise products over ONE base set of seg points (scalars: [batch][seg] Montgomery), summed per row:
// result[b] = sum_t scalars[b][t] * bases[t] - the stage commitments of every subcircuit of a key class in one launch
template <class F>
hk_status MsmRun<F>::small_msm_rows(hipStream_t s, const Affine<F>* bases, const void* scalars, u32 seg, u32 batch, XYZZ<F>* tab,
                                    XYZZ<F>* xy, XYZZ<F>* result) {
    typedef typename ScalarOf<F>::type Fr;
    size_t n = (size_t)seg * batch;
    if (n == 0 || n * EndoOf<F>::K > SPLIT_MAX_LANES) return HK_ERR_ARG;
    static const auto E = EndoOf<F>::split();
    SplitVecs<F> v = {};
    v.pts[0] = bases;
    v.pts_mod = seg;
    HK_TRY((launch_mul_split<Fr, typename F::Params, false>(s, v, 1u, (const Fr*)scalars, 0u, (u32)n, E, reinterpret_cast<Jac<F>*>(tab), xy, 1)));
    HK_LAUNCH((k_points_sum_seg<F, 64>), dim3(batch), dim3(64), 0, s, (const XYZZ<F>*)xy, seg, result);
    return HK_OK;
}

template <class F>
hk_status MsmRun<F>::fold_endo(hipStream_t s, u32 k, const Affine<F>* const* lo, const Affine<F>* const* hi, const void* coeffs_mont,
                               u32 neg_mask, u32 n, XYZZ<F>* tab, XYZZ<F>* xy, F* pref, Affine<F>* out, bool long_mags) {
    typedef typename ScalarOf<F>::type Fr;
    if (n == 0 || k == 0) return HK_OK;
    if (k > (u32)FOLD_MAX) return HK_ERR_ARG;
    const bool one_lane = long_mags || getenv("HK_ENDO_ONE_LANE") != nullptr;
    if (!one_lane && (size_t)n * EndoOf<F>::K <= SPLIT_MAX_LANES) {
        static const auto E = EndoOf<F>::split();                                // unused by the uniform form
        SplitVecs<F> v = {};
        for (u32 y = 0; y < k; y++) { v.lo[y] = lo[y]; v.pts[y] = hi[y]; }
        HK_TRY((launch_mul_split<Fr, typename F::Params, true>(s, v, k, (const Fr*)coeffs_mont, neg_mask, n, E, reinterpret_cast<Jac<F>*>(tab), xy)));
    } else {
        for (u32 y = 0; y < k; y++)                                              // long vectors: throughput-bound, one after the other
            HK_LAUNCH((k_points_fold_endo<Fr, F>), dim3((n + 63) / 64), dim3(64), 0, s, lo[y], hi[y], (const Fr*)coeffs_mont,
                      neg_mask, n, tab, xy + (size_t)y * n);
    }
    return batch_affine(s, xy, out, pref, k * n);
}

template <class F>
hk_status MsmRun<F>::lincomb(hipStream_t s, const Affine<F>* const* vecs, const void* coeffs_mont, u32 k, u32 n,
                             XYZZ<F>* xy, F* pref, Affine<F>* out) {
    typedef typename ScalarOf<F>::type Fr;
    if (n == 0) return HK_OK;
    if (k == 0 || k > (u32)LINCOMB_MAX) return HK_ERR_ARG;
    LincombVecs<F> lv;
    for (u32 j = 0; j < (u32)LINCOMB_MAX; j++) lv.v[j] = j < k ? vecs[j] : nullptr;
    HK_LAUNCH((k_points_lincomb<Fr, F>), dim3((n + 63) / 64), dim3(64), 0, s, lv, (const Fr*)coeffs_mont, k, n, xy);
    return batch_affine(s, xy, out, pref, n);
}

template <class F>
hk_status MsmRun<F>::fixed_base(hipStream_t s, const Affine<F>* base, const void* scalars, int is_mont,
                                u32 n, Affine<F>* table, XYZZ<F>* xy, F* pref, Affine<F>* out, bool build_table) {
    typedef typename ScalarOf<F>::type Fr;
    if (n == 0) return HK_OK;
    if (build_table) HK_LAUNCH((k_fb_table<F>), dim3(FB_WINDOWS * 256 / 64), dim3(64), 0, s, base, table);
    HK_LAUNCH((k_fb_mul<Fr, F>), dim3((n + 63) / 64), dim3(64), 0, s, table, (const Fr*)scalars,
              is_mont, n, xy);
    return batch_affine(s, xy, out, pref, n);
}

}  // namespace hk
