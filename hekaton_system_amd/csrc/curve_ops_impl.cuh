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
struct Ops final : CurveOps {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    typedef VerifyRun<typename Fq::Params> Verify;
    typedef CodecRun<typename Fq::Params> Codec;

    Ops() : CurveOps(sizeof(Fr), sizeof(Fq), sizeof(Affine<Fq>), sizeof(Affine<Fq2>), sizeof(Fp12<typename Fq::Params>)) {}

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
        Staged in[2] = {staged(scalars, n * sizeof(Fr)), staged(bases, n * sizeof(Affine<F>))};
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
        HK_TRY(L->carve([&](Carve& c) { stage_carve(c, in, 2); msm.carve(c); }));
        HK_TRY(stage_upload(L, in, 2));
        HK_TRY(msm.run(L->stream, (const Affine<F>*)in[1].p, in[0].p, mont, out, hipMemcpyDeviceToHost));
        return L->settle();
    }

    hk_status msm(hk_ctx* ctx, int group, const void* bases, size_t n_bases, const void* scalars,
                  size_t n_scalars, int mont, int checked, void* out) override {
        if (group == 1) return msm_plain<Fq>(ctx, bases, n_bases, scalars, n_scalars, mont, checked, out);
        return msm_plain<Fq2>(ctx, bases, n_bases, scalars, n_scalars, mont, checked, out);
    }

    // ---- defined by the headers named here, in CurveOps's order ----------------------------------------
    // ntt_host.cuh
    hk_status ntt(hk_ctx*, void*, unsigned, int, int) override;
    hk_status witness_map(hk_ctx*, const hk_csr*, const hk_csr*, const hk_csr*, size_t, size_t,
                          const void*, size_t, void*, size_t, size_t*) override;
    void ctx_release(hk_ctx*) override;
    // pk.cuh
    hk_status pk_upload(hk_ctx*, const hk_pk_desc*, hk_pk**) override;
    void pk_free(hk_pk*) override;
    // group_ops.cuh
    hk_status bases_upload(hk_ctx*, int, const void*, size_t, hk_bases**) override;
    void bases_free(hk_bases*) override;
    hk_status msm_bases(hk_ctx*, const hk_bases*, const void*, size_t, int, int, void*) override;
    hk_status fixed_base(hk_ctx*, int, const void*, const void*, size_t, int, void*) override;
    hk_status scalar_pairing(hk_ctx*, int, const void*, const void*, size_t, void*) override;
    hk_status points_lincomb(hk_ctx*, int, const void* const*, const void*, size_t, size_t, void*) override;
    template <class F>
    static hk_status points_fold(hk_ctx*, size_t, const void* const*, const void* const*, const void*, unsigned, size_t, void* const*);
    hk_status points_fold_many(hk_ctx*, int, size_t, const void* const*, const void* const*, const void*, unsigned, size_t,
                               void* const*) override;
    hk_status field_convert(hk_ctx*, int, const void*, void*, size_t, int) override;
    // witness_host.cuh
    hk_status assignment_from_bits(hk_ctx*, const void*, size_t, const uint32_t*, const void*, size_t, void*) override;
    hk_status wprog_upload(hk_ctx*, const uint32_t*, size_t, const uint32_t*, size_t, const uint32_t*, size_t, size_t,
                           size_t, hk_wprog**) override;
    void wprog_free(hk_wprog*) override;
    hk_status wprog_run(hk_ctx*, const hk_wprog*, const uint32_t*, size_t, const uint32_t*, const void*, size_t, void*) override;
    hk_status assignment_scatter(hk_ctx*, const uint32_t*, const void*, size_t, size_t, size_t, void*) override;
    hk_status poseidon_path(hk_ctx*, const void*, size_t, const hk_poseidon_desc*, const hk_poseidon_desc*, const void*,
                            const void*, const uint32_t*, size_t, size_t, size_t, size_t, void*) override;
    // pairing_ops.cuh
    hk_status pairing_products(hk_ctx*, const void* const*, size_t, const void* const*, size_t, size_t, void*) override;
    hk_status pairing_pairs(hk_ctx*, const void* const*, size_t, const void* const*, size_t, const uint32_t*, const uint32_t*, size_t,
                            size_t, void*) override;
    hk_status gt_pow(hk_ctx*, const void*, const void*, size_t, void*, int, size_t) override;
    hk_status gt_check(hk_ctx*, const void*, size_t, unsigned char*) override;
    // prove_impl.cuh
    hk_status commit(hk_ctx*, const hk_pk*, size_t, const void*, size_t, const void*, void*) override;
    hk_status commit_batch(hk_ctx*, const hk_pk*, size_t, const void*, size_t, const void*, size_t, void*) override;
    hk_status prove_batch(hk_ctx*, const hk_pk*, size_t, size_t, const ProveRow*, size_t) override;
    // verify.cuh
    hk_status vk_prepare(hk_ctx* ctx, const hk_vk_desc* d, hk_vk** out) override { return Verify::vk_prepare(ctx, d, out); }
    void vk_free(hk_vk* vk) override { Verify::vk_free(vk); }
    hk_status vk_alpha_beta(const hk_vk* vk, void* out) override { return Verify::vk_alpha_beta(vk, out); }
    hk_status verify_batch(hk_ctx* ctx, const hk_vk* vk, const void* a, const void* b, const void* c, const void* ds,
                           const void* inputs, size_t n, unsigned flags, const void* rand, unsigned char* verdicts) override {
        return Verify::verify_batch(ctx, vk, a, b, c, ds, inputs, n, flags, rand, verdicts);
    }
    hk_status points_check(hk_ctx* ctx, int group, const void* pts, size_t n, unsigned char* ok) override {
        return Verify::points_check(ctx, group, pts, n, ok);
    }
    // keygen.cuh
    hk_status qap_eval(hk_ctx*, const hk_csr*, const hk_csr*, const hk_csr*, size_t, size_t, size_t, const void*, void*,
                       void*, void*, void*, size_t*) override;
    hk_status keygen(hk_ctx*, const hk_keygen_desc*, const hk_keygen_out*, size_t*) override;
    // exec_tree.cuh
    hk_status exec_tree(hk_ctx*, const hk_exec_tree_desc*, const hk_exec_tree_out*) override;
    // stage1.cuh
    hk_status stage1_witness(hk_ctx*, const hk_stage1_desc*, const uint32_t*, size_t, size_t, void*) override;
    // trace_sort.cuh
    hk_status trace_sort(hk_ctx*, uint32_t, const void*, size_t, void*, uint32_t*) override;
    hk_status stage0_witness(hk_ctx*, const uint32_t*, uint32_t, uint32_t, const void*, const void*, const uint32_t*, size_t,
                             void*) override;
    // r1cs_check.cuh
    hk_status r1cs_check(hk_ctx*, const hk_csr*, const hk_csr*, const hk_csr*, const void*, size_t, size_t, hk_r1cs_verdict*,
                         uint32_t*, void*, size_t) override;
    hk_status pk_r1cs_check(hk_ctx*, const hk_pk*, const void*, size_t, size_t, hk_r1cs_verdict*, uint32_t*, void*, size_t) override;
    // sha_tree.cuh
    hk_status sha_tree(hk_ctx*, const void*, uint32_t, uint32_t, uint32_t, const hk_sha_tree_out*) override;
    hk_status sha_tree_inputs(hk_ctx*, const void*, const void*, uint32_t, uint32_t, const uint32_t*, size_t, uint32_t*) override;
    // ram_witness.cuh
    hk_status ram_stage0_witness(hk_ctx*, const uint32_t*, uint32_t, uint32_t, const void*, const void*, const uint32_t*, size_t,
                                 void*) override;
    hk_status ram_stage1_witness(hk_ctx*, const hk_ram_stage1_desc*, const uint32_t*, size_t, size_t, void*) override;
    // r1cs_job.cuh
    hk_status r1cs_job_trace(hk_ctx*, const hk_r1cs_job_desc*, void*) override;
    hk_status r1cs_job_witness(hk_ctx*, const hk_r1cs_job_desc*, const uint32_t*, size_t, size_t, size_t, void*) override;
    // vkd.cuh
    hk_status vkd_trace(hk_ctx*, const hk_vkd_desc*, void*, void*) override;
    hk_status vkd_witness(hk_ctx*, const hk_vkd_desc*, const uint32_t*, size_t, size_t, const hk_vkd_cols*, void*) override;
    // vkd_tree.cuh
    hk_status vkd_tree(hk_ctx*, const hk_vkd_tree_desc*, void*, void*, uint8_t*) override;
    // agg_scalars.cuh
    hk_status scalar_powers(hk_ctx*, const void*, size_t, size_t, void*) override;
    hk_status ipa_quotient(hk_ctx*, const void*, size_t, const void*, const void*, size_t, void*) override;
    // class_sums.cuh
    hk_status class_power_sums(hk_ctx*, const void*, const uint32_t*, size_t, size_t, void*) override;
    // point_codec.cuh
    hk_status field_sqrt(hk_ctx* ctx, int which, const void* in, size_t n, void* out, unsigned char* ok) override {
        return Codec::field_sqrt(ctx, which, in, n, out, ok);
    }
    hk_status points_decompress(hk_ctx* ctx, int group, const void* x_canon, const unsigned char* flags, size_t n, int check,
                                void* points_out, unsigned char* status) override {
        return Codec::points_decompress(ctx, group, x_canon, flags, n, check, points_out, status);
    }
    hk_status points_compress(hk_ctx* ctx, int group, const void* points, size_t n, void* x_canon_out,
                              unsigned char* flags_out) override {
        return Codec::points_compress(ctx, group, points, n, x_canon_out, flags_out);
    }
};

}  // namespace hk
