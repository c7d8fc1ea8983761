// curve_ops_impl.cuh — per-curve host orchestration (templated on the curve traits); included by
// hk_<curve>_ops.hip.  Heavy kernels are instantiated in their own translation units
// (hk_<curve>_{g1,g2,fr}.hip) and referenced here through extern templates.
#pragma once
#include "msm_driver.cuh"
#include "endo.cuh"

namespace hk {

// window size for an MSM over caller-supplied bases (no shift tables: all W windows keep their own
// buckets, W * 2^(c-1) counters must fit the 128 KiB LDS histogram)
inline u32 msm_pick_c_plain(size_t n, u32 fr_bits) {
    u32 best = 4;
    double best_cost = 1e300;
    for (u32 c = 3; c <= 12; c++) {
        u32 W = (fr_bits + 2 + c - 1) / c;
        u64 NB = (u64)W << (c - 1);
        if (NB > (u64)MSM_LDS_COUNTERS) continue;
        double cost = (double)n * W + 4.0 * (double)NB;
        if (cost < best_cost) { best_cost = cost; best = c; }
    }
    return best;
}
// window size when shift tables make every window share one bucket set (WP = 1)
inline u32 msm_pick_c_tables(size_t n, u32 fr_bits) {
    u32 best = 6;
    double best_cost = 1e300;
    for (u32 c = 5; c <= 16; c++) {
        u32 W = (fr_bits + 2 + c - 1) / c;
        double cost = (double)n * W + 6.0 * (double)(1u << (c - 1));
        if (cost < best_cost) { best_cost = cost; best = c; }
    }
    return best;
}

template <class C>
struct Ops {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;

    // One MSM into the affine point `out` on the lane's stream: n element-wise products over the endomorphism and one sum
    // (MsmRun::small_msm) when `small`, else the digit sort and the bucket pass over plan *p.  carve() lists its scratch
    // inside the caller's Lane::carve; run() takes n scalars and n bases (group 0 of a table) on the device.
    template <class F>
    struct OneMsm {
        bool small;
        const MsmPlan* p;
        u32 n;
        XYZZ<F>*xy, *tab, *res;
        Affine<F>* aff;
        SortBufs sb;
        typename MsmRun<F>::Bufs rb;

        void carve(Carve& c) {
            if (small) {
                xy = c.n<XYZZ<F>>(n);
                tab = (XYZZ<F>*)c.take(endo_tab_bytes<F>(n));
            } else {
                MsmSort<Fr>::alloc(c, *p, &sb);
                MsmRun<F>::alloc(c, *p, &rb);
            }
            res = c.n<XYZZ<F>>(1);
            aff = c.n<Affine<F>>(1);
        }
        // ev0 / ev1 (optional) bracket the bucket-accumulate launch
        hk_status run(hipStream_t s, const Affine<F>* bases, const void* scalars, int mont, void* out, hipMemcpyKind kind,
                      hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr) const {
            if (small) {
                HK_TRY(MsmRun<F>::small_msm(s, bases, scalars, mont, n, tab, xy, res));
            } else {
                HK_TRY(MsmSort<Fr>::run(s, *p, (const u32*)scalars, mont, sb));
                HK_TRY(MsmRun<F>::run(s, *p, bases, n, 0, sb, rb, res, ev0, ev1));
            }
            HK_TRY(MsmRun<F>::to_affine(s, res, aff, 1));
            HK_HIP(hipMemcpyAsync(out, aff, sizeof(Affine<F>), kind, s));
            return HK_OK;
        }
    };

    template <class F>
    static hk_status msm_plain(hk_ctx* ctx, const void* bases, size_t n_bases, const void* scalars,
                               size_t n_scalars, int mont, int checked, void* out) {
        if (checked && n_bases != n_scalars) return HK_ERR_LEN;     // ark `msm`: Err(min_len)
        size_t n = n_bases < n_scalars ? n_bases : n_scalars;      // ark `msm_unchecked`: zip
        if (n == 0) { memset(out, 0, sizeof(Affine<F>)); return HK_OK; }
        if (!bases || !scalars) return HK_ERR_ARG;
        if (n >= (1u << 26)) return HK_ERR_ARG;
        LaneGuard g(ctx);
        Lane* L = g.lane;
        if (!L) return HK_ERR_DEVICE;
        // short vector, no tables: a Pippenger pass would end in ~254 serial doublings (3 / 8.5 ms whatever n)
        const bool small = n * EndoOf<F>::K <= SPLIT_MAX_LANES && !getenv("HK_MSM_NO_SMALL");
        MsmPlan p;
        if (!small)
            p = msm_make_plan((u32)n, C::FR_BITS, msm_pick_c_plain(n, C::FR_BITS), 0xffffffffu, ctx->max_lanes0, C::Fr::Params::MOD,
                              C::Fr::Params::N);
        OneMsm<F> msm{small, &p, (u32)n};
        const void *sc_d, *b_d;
        HK_TRY(L->carve([&](Carve& c) { sc_d = c.take(n * sizeof(Fr)); b_d = c.take(n * sizeof(Affine<F>)); msm.carve(c); }));
        HK_TRY(to_device(L, scalars, n * sizeof(Fr), &sc_d));
        HK_TRY(to_device(L, bases, n * sizeof(Affine<F>), &b_d));
        HK_TRY(msm.run(L->stream, (const Affine<F>*)b_d, sc_d, mont, out, hipMemcpyDeviceToHost));
        return L->settle();
    }

    static hk_status msm(hk_ctx* ctx, int group, const void* bases, size_t n_bases, const void* scalars,
                         size_t n_scalars, int mont, int checked, void* out) {
        if (group == 1) return msm_plain<Fq>(ctx, bases, n_bases, scalars, n_scalars, mont, checked, out);
        return msm_plain<Fq2>(ctx, bases, n_bases, scalars, n_scalars, mont, checked, out);
    }

    // ---- filled in by later includes (ntt / qap / prove) -------------------------------------------
    static hk_status ntt(hk_ctx*, void*, unsigned, int, int);
    static hk_status witness_map(hk_ctx*, const hk_csr*, const hk_csr*, const hk_csr*, size_t, size_t,
                                 const void*, size_t, void*, size_t, size_t*);
    static hk_status pk_upload(hk_ctx*, const hk_pk_desc*, hk_pk**);
    static void pk_free(hk_pk*);
    static hk_status commit(hk_ctx*, const hk_pk*, size_t, const void*, size_t, const void*, void*);
    static hk_status commit_batch(hk_ctx*, const hk_pk*, size_t, const void*, size_t, const void*, size_t, void*);
    static hk_status prove_batch(hk_ctx*, const hk_pk*, size_t, size_t, const ProveRow*, size_t);
    static void ctx_release(hk_ctx*);
    static hk_status fixed_base(hk_ctx*, int, const void*, const void*, size_t, int, void*);
    static hk_status scalar_pairing(hk_ctx*, int, const void*, const void*, size_t, void*);
    static hk_status field_convert(hk_ctx*, int, const void*, void*, size_t, int);
    static hk_status bases_upload(hk_ctx*, int, const void*, size_t, hk_bases**);
    static void bases_free(hk_bases*);
    static hk_status msm_bases(hk_ctx*, const hk_bases*, const void*, size_t, int, int, void*);
    static hk_status pairing_products(hk_ctx*, const void* const*, size_t, const void* const*, size_t, size_t, void*);
    static hk_status points_lincomb(hk_ctx*, int, const void* const*, const void*, size_t, size_t, void*);
    template <class F>
    static hk_status points_fold(hk_ctx*, size_t, const void* const*, const void* const*, const void*, unsigned, size_t, void* const*);
    static hk_status assignment_scatter(hk_ctx*, const uint32_t*, const void*, size_t, size_t, size_t, void*);
    static hk_status pairing_pairs(hk_ctx*, const void* const*, size_t, const void* const*, size_t, const uint32_t*, const uint32_t*, size_t,
                                   size_t, void*);
    static hk_status points_fold_many(hk_ctx*, int, size_t, const void* const*, const void* const*, const void*, unsigned, size_t, void* const*);
    static hk_status points_fold_g2(hk_ctx*, const void*, const void*, const void*, unsigned, size_t, void*);
    static hk_status points_fold_g1(hk_ctx*, const void*, const void*, const void*, unsigned, size_t, void*);
    static hk_status assignment_from_bits(hk_ctx*, const void*, size_t, const uint32_t*, const void*, size_t, void*);
    static hk_status wprog_upload(hk_ctx*, const uint32_t*, size_t, const uint32_t*, size_t, const uint32_t*, size_t, size_t,
                                  size_t, hk_wprog**);
    static void wprog_free(hk_wprog*);
    static hk_status gt_pow(hk_ctx*, const void*, const void*, size_t, void*, int, size_t);
    static hk_status wprog_run(hk_ctx*, const hk_wprog*, const uint32_t*, size_t, const uint32_t*, const void*, size_t, void*);
    static hk_status qap_eval(hk_ctx*, const hk_csr*, const hk_csr*, const hk_csr*, size_t, size_t, size_t, const void*, void*,
                              void*, void*, void*, size_t*);     // keygen.cuh
    static hk_status keygen(hk_ctx*, const hk_keygen_desc*, const hk_keygen_out*, size_t*);
    static hk_status exec_tree(hk_ctx*, const hk_exec_tree_desc*, const hk_exec_tree_out*);     // exec_tree.cuh
    static hk_status stage1_witness(hk_ctx*, const hk_stage1_desc*, const uint32_t*, size_t, size_t, void*);     // stage1.cuh
    static hk_status trace_sort(hk_ctx*, uint32_t, const void*, size_t, void*, uint32_t*);     // trace_sort.cuh
    static hk_status stage0_witness(hk_ctx*, const uint32_t*, uint32_t, uint32_t, const void*, const void*, const uint32_t*, size_t, void*);

    static size_t max_private_bytes() {
        size_t m = MsmRun<Fq>::max_private_bytes();
        size_t b = MsmRun<Fq2>::max_private_bytes();
        if (b > m) m = b;
        b = PairRun<typename Fq::Params>::max_private_bytes();
        if (b > m) m = b;
        b = VerifyRun<typename Fq::Params>::max_private_bytes();
        if (b > m) m = b;
        b = finish_private_bytes();
        return b > m ? b : m;
    }
    static size_t finish_private_bytes();      // prove_impl.cuh (k_finish)
    static hk_status poseidon_path(hk_ctx*, const void*, size_t, const hk_poseidon_desc*, const hk_poseidon_desc*, const void*,
                                   const void*, const uint32_t*, size_t, size_t, size_t, size_t, void*);

    static const CurveOps* table() {
        static const CurveOps t = {sizeof(Fr), sizeof(Fq), sizeof(Affine<Fq>), sizeof(Affine<Fq2>),
                                   &msm, &ntt, &witness_map, &pk_upload, &pk_free, &commit,
                                   &ctx_release, &fixed_base, &scalar_pairing, &field_convert, &bases_upload,
                                   &bases_free, &msm_bases, &pairing_products,
                                   sizeof(Fp12<typename Fq::Params>), &points_lincomb, &points_fold_g2, &points_fold_g1, &assignment_from_bits, &wprog_upload, &wprog_free, &wprog_run, &gt_pow,
                                   &max_private_bytes, &poseidon_path, &points_fold_many, &pairing_pairs, &assignment_scatter, &commit_batch,
                                   &prove_batch, &VerifyRun<typename Fq::Params>::vk_prepare, &VerifyRun<typename Fq::Params>::vk_free,
                                   &VerifyRun<typename Fq::Params>::vk_alpha_beta, &VerifyRun<typename Fq::Params>::verify_batch,
                                   &VerifyRun<typename Fq::Params>::points_check, &qap_eval, &keygen, &exec_tree, &stage1_witness,
                                   &trace_sort, &stage0_witness};
        return &t;
    }
};

}  // namespace hk
