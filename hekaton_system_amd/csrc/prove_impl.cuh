// prove_impl.cuh — per-curve host orchestration of the CP-Groth16 hot path on one GPU: hk_commit, hk_commit_batch and
// hk_prove / hk_prove_batch over a resident proving key (pk.cuh) and the witness map (ntt_host.cuh).
//
// Reference path restated (all arithmetic on the device; this file only sequences launches):
//   CPGroth16::prove_last_stage            cp-groth16/src/prover.rs:78-155
//   CommitmentBuilder::{commit,prove}      cp-groth16/src/committer.rs:87-91, 112-114
//   LibsnarkReduction::witness_map         ark-groth16 0.4, called at prover.rs:123
//
// Fusion specific to this design: the O(1) fixed-base scalar multiplications of the reference
// (r*delta, s*delta, r*s*delta, kappa_i*delta_i — prover.rs:86,96,106,135; committer.rs:113) ride the
// big MSMs as extra (base, scalar) pairs appended to the assignment ("ext" slots), so only the two
// genuinely variable-base products s*A and r*B1 remain for the finish kernel.
#pragma once
#include "ntt_host.cuh"
#include "pk.cuh"

namespace hk {

// ---- small device helpers for the fused calls -------------------------------------------------------------
// ext[0] = r, ext[1] = s, ext[2] = r*s, ext[3+i] = kappa_i   (all Montgomery), for each of `batch` proofs: row b of ext
// starts ext_stride elements after row b - 1, row b of rs_kappas (r, s, kappas) rs_stride after.
// Also clears the bucket counters of the proofs' two digit sorts, z's and h's (arrays of `nb` u32 each, every proof's
// counters; every workgroup takes a share): they are accumulated with atomics by k_msm_hist, and this kernel precedes both
// sorts in stream order (the H stream waits for the event recorded behind it) - two memset launches less.
template <class Fr>
__global__ void k_prep_ext(Fr* __restrict__ ext, u32 ext_stride, const Fr* __restrict__ rs_kappas, u32 rs_stride,
                           u32 n_kappas, u32 batch, u32* __restrict__ c0, u32* __restrict__ c1, u32 nb0, u32 nb1) {
    u32 gt = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (u32 i = gt; i < nb0; i += stride) c0[i] = 0;
    for (u32 i = gt; i < nb1; i += stride) c1[i] = 0;
    if (gt >= batch) return;
    Fr* e = ext + (size_t)gt * ext_stride;
    const Fr* rk = rs_kappas + (size_t)gt * rs_stride;
    Fr r = fr_load(&rk[0]), s = fr_load(&rk[1]);
    fr_store(&e[0], r);
    fr_store(&e[1], s);
    fr_store(&e[2], Fr::mul(r, s));
    for (u32 i = 0; i < n_kappas; i++) fr_store(&e[3 + i], fr_load(&rk[2 + i]));
}

// Finish: A = MA + a_g[0] + alpha_g ; B = MB2 + b_h[0] + beta_h ; B1 = MB1 + b_g[0] + beta_g ;
//         C = s*A + r*B1 + ML' + MH   with ML' = L - rs*delta_g - sum kappa_i*delta_i   (see file header)
// (an evaluation-basis key, h_basis.cuh: ML' also carries -sum_{k>=1} z_k C^_k, the constant c1[4] = -C^_0 completes it, and
// MH = sum_j (a'_j b'_j) G^_j: the same C)
// (prover.rs:135-155 "Finish C" + into_affine, committer.rs:112-114).  Two kernels, so that the variable-base products
// do not wait for H: k_finish_ab needs only A, B1, B2 and L and leaves C without MH in part_c; k_finish_c adds MH once H is
// done and normalises C.  The sum is the one the single kernel formed, in the same order, and an affine point is unique.
// k_finish_ab: one lane per output point.  Grid (3, batch), proof = blockIdx.y: res_g1 holds 4 points per proof (MA, MB1,
// ML, MH; MH is not read here), res_g2 1 (MB2), rs rs_stride Fr per proof (r, s, kappas); one point per proof in each of
// out_a / out_b / part_c.
template <class Fr, class Fq, class Fq2>
__global__ void k_finish_ab(const XYZZ<Fq>* __restrict__ res_g1_all, const XYZZ<Fq2>* __restrict__ res_g2_all,
                            const Affine<Fq>* __restrict__ c1, const Affine<Fq2>* __restrict__ c2, const Fr* __restrict__ rs_all,
                            u32 rs_stride, Affine<Fq>* __restrict__ out_a_all, Affine<Fq2>* __restrict__ out_b_all,
                            XYZZ<Fq>* __restrict__ part_c_all, EndoSplit<2> E) {
    const size_t pr = blockIdx.y;
    const XYZZ<Fq>* __restrict__ res_g1 = res_g1_all + 4 * pr;
    const XYZZ<Fq2>* __restrict__ res_g2 = res_g2_all + pr;
    const Fr* __restrict__ rs = rs_all + pr * rs_stride;
    Affine<Fq>* __restrict__ out_a = out_a_all + pr;
    Affine<Fq2>* __restrict__ out_b = out_b_all + pr;
    XYZZ<Fq>* __restrict__ part_c = part_c_all + pr;
    if (blockIdx.x < 2 && threadIdx.x) return;
    if (blockIdx.x == 0) {
        XYZZ<Fq> A = ec_madd_ni(ec_madd_ni(ld_vec(&res_g1[0]), ld_vec(&c1[0])), ld_vec(&c1[1]));
        st_vec(out_a, ec_to_affine(A));
    } else if (blockIdx.x == 1) {
        XYZZ<Fq2> B = ec_madd_ni(ec_madd_ni(ld_vec(&res_g2[0]), ld_vec(&c2[0])), ld_vec(&c2[1]));
        st_vec(out_b, ec_to_affine(B));
    } else {
        // C = s*A + r*B1 + ML' + MH.  This kernel is the tail of every proof's latency, and its two variable-base products
        // were one lane's chain of 256 doublings + <= 128 additions (Straus over a joint table: 3 ms).  They now run as
        // the short element-wise sweeps do: A and B1 are normalised by lanes 0 and 1, then FOUR lanes take one GLV half
        // each (s = s0 + s1 lambda on A, r = r0 + r1 lambda on B1: <= 131 bits) with a table 1P .. 8P, built here straight
        // in LDS, and the sweeps' digit loop (split_window_digits, endo.cuh: its wave vote counts the lanes that are in
        // it, those of the four whose base is not at infinity); lane 0 joins the four partial products.
        __shared__ Affine<Fq> base[2];
        __shared__ Jac<Fq> tab[4][SPLIT_TABLE];
        __shared__ Jac<Fq> part[4];
        const u32 t = threadIdx.x;
        if (t < 2) {
            XYZZ<Fq> X = ec_madd_ni(ec_madd_ni(ld_vec(&res_g1[t]), ld_vec(&c1[2 * t])), ld_vec(&c1[2 * t + 1]));   // A | B1
            base[t] = ec_to_affine(X);
        }
        __syncthreads();
        if (t < 4) {
            constexpr int ND = SplitDigits<Fq>::ND;
            Fr k = Fr::from_mont(fr_load(&rs[(t >> 1) == 0 ? 1 : 0]));          // lanes 0, 1: s (on A);  lanes 2, 3: r (on B1)
            u32 c[8], mag[2][6];
            HK_UNROLL for (int l = 0; l < 8; l++) c[l] = l < Fr::N ? k.v[l] : 0u;
            u32 neg = endo_decompose<2>(c, E, mag);
            u32 m[6];
            HK_UNROLL for (int l = 0; l < 6; l++) m[l] = (t & 1u) ? mag[1][l] : mag[0][l];
            split_bias<ND>(m);
            Affine<Fq> q = base[t >> 1];
            Jac<Fq> acc = Jac<Fq>::inf();
            const bool q_inf = q.is_inf();
            if (!q_inf) {
                if (t & 1u) q = EndoOf<Fq>::apply(q);
                if ((neg >> (t & 1u)) & 1u) q.y = Fq::neg(q.y);
                Jac<Fq> e = Jac<Fq>::from_affine(q);
                tab[t][0] = e;
                HK_NOUNROLL for (int i = 2; i <= SPLIT_TABLE; i++) {
                    Jac<Fq> prev = (i & 1) ? tab[t][i - 2] : tab[t][i / 2 - 1];
                    e = (i & 1) ? jac_madd_ni(prev, q) : jac_dbl_ni(prev);
                    tab[t][i - 1] = e;
                }
                split_window_digits(false, m, SplitTabRow<Fq>{tab[t]}, acc);
            }
            part[t] = acc;
        }
        __syncthreads();
        if (t == 0) {
            Jac<Fq> sum = part[0];
            HK_NOUNROLL for (int i = 1; i < 4; i++) sum = jac_add_ni(sum, part[i]);
            // c1[4]: -C^_0 of an evaluation-basis key (z_0 = 1 is no ext scalar), infinity otherwise
            st_vec(part_c, ec_madd_ni(ec_add_ni(jac_to_xyzz(sum), ld_vec(&res_g1[2])), ld_vec(&c1[4])));
        }
    }
}

// k_finish_c: C = part_c + MH, to affine.  One lane per proof of the chunk, one wave.
static_assert(HK_PROVE_BATCH_CHUNK <= 64, "k_finish_c covers a chunk with one wave");
template <class Fq>
__global__ void __launch_bounds__(64) k_finish_c(const XYZZ<Fq>* __restrict__ part_c, const XYZZ<Fq>* __restrict__ res_g1_all,
                                                 Affine<Fq>* __restrict__ out_c, u32 batch) {
    const u32 pr = threadIdx.x;
    if (pr >= batch) return;
    XYZZ<Fq> Cc = ec_add_ni(ld_vec(&part_c[pr]), ld_vec(&res_g1_all[4 * (size_t)pr + 3]));
    st_vec(&out_c[pr], ec_to_affine(Cc));
}

template <class C>
hk_status Ops<C>::commit(hk_ctx* ctx, const hk_pk* h, size_t stage, const void* w, size_t n,
                         const void* kappa, void* out) {
    if (h->ctx != ctx) return HK_ERR_ARG;                  // a key lives on the context (device) that uploaded it
    PkImpl<C>* pk = (PkImpl<C>*)h->impl;
    if (stage >= pk->n_stages) return HK_ERR_ARG;          // "no more values left in committing key"
    if (n + 1 != pk->ck_n[stage]) return HK_ERR_LEN;       // committer.rs:83
    if (n && !w) return HK_ERR_ARG;
    // a short stage (the 16 stage-0 witnesses of a big-merkle subcircuit) takes no bucket pass: the one-row form of
    // hk_commit_batch - 17 element-wise products over the endomorphism and one sum, 1.4 ms instead of 2.2
    if ((n + 1) * EndoOf<Fq>::K <= SPLIT_MAX_LANES && !is_device_ptr(out) && !getenv("HK_MSM_NO_SMALL"))
        return commit_batch(ctx, h, stage, w, n, kappa, 1, out);
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    OneMsm<Fq> msm{false, &pk->plan_ck[stage], (u32)(n + 1)};
    Fr* sc;
    HK_TRY(L->carve([&](Carve& c) { sc = c.n<Fr>(n + 1); msm.carve(c); }));
    hipStream_t s = L->stream;
    bool prof = ctx->profiling;
    if (prof) HK_HIP(hipEventRecord(L->ev[0], s));
    if (n) HK_HIP(hipMemcpyAsync(sc, w, n * sizeof(Fr), h2d_kind(w), s));
    HK_HIP(hipMemcpyAsync(sc + n, kappa, sizeof(Fr), hipMemcpyHostToDevice, s));
    HK_TRY(msm.run(s, pk->ck_tab[stage], sc, 1, out, hipMemcpyDeviceToHost, prof ? L->ev[20] : nullptr, prof ? L->ev[21] : nullptr));
    if (prof) HK_HIP(hipEventRecord(L->ev[1], s));
    HK_TRY(L->settle());
    if (prof) {
        memset(&L->timings, 0, sizeof(L->timings));
        L->timings.total_ms = ev_ms(L->ev[0], L->ev[1]);
        L->timings.accum_kernel_ms = ev_ms(L->ev[20], L->ev[21]);
        L->timings.accum_kernel_launches = 1;
    }
    return HK_OK;
}

// `batch` commitments under one key and stage.  Short stages (batch (n + 1) K <= SPLIT_MAX_LANES: the 16 stage-0 witnesses
// of a big-merkle subcircuit) run as ONE set of launches - every term an element-wise product over the endomorphism on its
// own lanes, one workgroup's sum per commitment, one normalisation - instead of `batch` bucket passes of ten tiny launches
// each; longer stages fall back to hk_commit per row.
template <class C>
hk_status Ops<C>::commit_batch(hk_ctx* ctx, const hk_pk* h, size_t stage, const void* w, size_t n, const void* kappas,
                               size_t batch, void* out) {
    if (h->ctx != ctx) return HK_ERR_ARG;
    PkImpl<C>* pk = (PkImpl<C>*)h->impl;
    if (stage >= pk->n_stages) return HK_ERR_ARG;
    if (n + 1 != pk->ck_n[stage]) return HK_ERR_LEN;
    if (batch == 0) return HK_OK;
    if ((n && !w) || !kappas || !out) return HK_ERR_ARG;
    const size_t seg = n + 1, tot = seg * batch;
    if (tot * EndoOf<Fq>::K > SPLIT_MAX_LANES || is_device_ptr(kappas) || getenv("HK_MSM_NO_SMALL")) {
        if (is_device_ptr(kappas) || is_device_ptr(out)) return HK_ERR_ARG;
        for (size_t b = 0; b < batch; b++)
            HK_TRY(commit(ctx, h, stage, n ? (const char*)w + b * n * sizeof(Fr) : nullptr, n, (const char*)kappas + b * sizeof(Fr),
                          (char*)out + b * sizeof(Affine<Fq>)));
        return HK_OK;
    }
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    Fr* sc;
    XYZZ<Fq>*xy, *tab, *res;
    Fq* pref;
    Affine<Fq>* aff;
    HK_TRY(L->carve([&](Carve& c) {
        sc = c.n<Fr>(tot);                                     // [batch][n + 1]: a row's witnesses, then its kappa
        xy = c.n<XYZZ<Fq>>(tot);
        tab = (XYZZ<Fq>*)c.take(endo_tab_bytes<Fq>(tot));
        res = c.n<XYZZ<Fq>>(batch);
        pref = c.n<Fq>(batch);
        aff = c.n<Affine<Fq>>(batch);
    }));
    hipStream_t s = L->stream;
    bool prof = ctx->profiling;
    if (prof) HK_HIP(hipEventRecord(L->ev[0], s));
    if (n) HK_HIP(hipMemcpy2DAsync(sc, seg * sizeof(Fr), w, n * sizeof(Fr), n * sizeof(Fr), batch, h2d_kind(w), s));
    HK_HIP(hipMemcpy2DAsync(sc + n, seg * sizeof(Fr), kappas, sizeof(Fr), sizeof(Fr), batch, hipMemcpyHostToDevice, s));
    HK_TRY(MsmRun<Fq>::small_msm_rows(s, pk->ck_tab[stage], sc, (u32)seg, (u32)batch, tab, xy, res));   // group 0 of the table
    HK_TRY(MsmRun<Fq>::batch_affine(s, res, aff, pref, (u32)batch));
    HK_HIP(hipMemcpyAsync(out, aff, batch * sizeof(Affine<Fq>), is_device_ptr(out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (prof) HK_HIP(hipEventRecord(L->ev[1], s));
    HK_TRY(L->settle());
    if (prof) {
        memset(&L->timings, 0, sizeof(L->timings));
        L->timings.total_ms = ev_ms(L->ev[0], L->ev[1]);
    }
    return HK_OK;
}

// hk_prove_batch and hk_prove's coalesced batches (a lone hk_prove is a batch of one).  A batch runs in chunks of up to
// HK_PROVE_BATCH_CHUNK proofs, every stage one launch for the chunk (proof = grid.y, or grid.x for the one-workgroup
// stages), each proof on its own slice of the buffers; all read the key's shared shift tables.  Row b's inputs and outputs
// live wherever rows[b] points: a chunk may mix host and device assignments.
template <class C>
hk_status Ops<C>::prove_batch(hk_ctx* ctx, const hk_pk* h, size_t n_v, size_t n_kappas, const ProveRow* rows, size_t batch) {
    typedef QapHost<C> Q;
    if (h->ctx != ctx) return HK_ERR_ARG;
    PkImpl<C>* pk = (PkImpl<C>*)h->impl;
    if (!pk->has_qap) return HK_ERR_ARG;
    if (n_v != pk->n_v) return HK_ERR_LEN;
    if (n_kappas + 1 != pk->n_stages) return HK_ERR_LEN;   // committer.rs:112 assert
    if (batch == 0) return HK_OK;
    if (!rows) return HK_ERR_ARG;
    for (size_t b = 0; b < batch; b++) {
        const ProveRow& w = rows[b];
        if (!w.z || !w.r || !w.s || !w.a || !w.b || !w.c || (n_kappas && !w.kappas)) return HK_ERR_ARG;
    }
    // a prove lane first, before anything else that might wait: its holder never waits for a general lane
    LaneGuard g(ctx, ProveLaneTag{});
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    NttTables* T;
    HK_TRY(NttHost<C>::ensure(ctx, pk->log_m, &T));
    const MsmPlan &pz = pk->plan_z, &ph = pk->plan_h, &pa = pk->plan_a, &pb = pk->plan_b;
    const size_t m = (size_t)1 << pk->log_m, fr = sizeof(Fr), rs_stride = 2 + n_kappas;
    const size_t h_stride = (pk->h_eval ? 2 : 3) * m;                          // a proof's witness-map scratch, in Fr
    std::vector<char> z_dev(batch);
    bool any_host = false;
    for (size_t b = 0; b < batch; b++) {
        z_dev[b] = is_device_ptr(rows[b].z);
        any_host = any_host || !z_dev[b];
    }
    // the scratch of one chunk of `nb` proofs: every per-proof buffer times nb, the bucket pipelines sized by the lane plan
    // of the chunk (the chip's lanes split across it, so the boundary partials do not grow with nb)
    Fr *zext, *small, *zt, *abc;
    SortBufs sb, sbh, sba, sbb;                                               // z, h; the sub-lists of z for A and for B
    typename MsmRun<Fq>::Bufs rbA, rbB1, rbL, rbh;
    typename MsmRun<Fq2>::Bufs rb2;
    XYZZ<Fq>* res1;
    XYZZ<Fq2>* res2;
    Affine<Fq> *oa, *oc;
    Affine<Fq2>* ob;
    XYZZ<Fq>* pc;
    auto chunk_bufs = [&](Carve& c, u32 nb) {
        zext = c.n<Fr>((size_t)pk->n_ext * nb);                               // z[1..] | r | s | rs | kappas
        small = c.n<Fr>(rs_stride * nb);                                      // [nb][2 + n_kappas]
        zt = any_host ? c.n<Fr>(n_v * nb) : nullptr;                          // host rows of z, copied in (slot = row)
        MsmSort<Fr>::alloc(c, pz, &sb, nb);
        MsmSort<Fr>::alloc(c, ph, &sbh, nb);
        if (pk->a_compact) MsmSort<Fr>::alloc_sub(c, pz, pa, &sba, nb);
        if (pk->b_compact) MsmSort<Fr>::alloc_sub(c, pz, pb, &sbb, nb);
        MsmRun<Fq>::alloc(c, pa, &rbA, nb);
        MsmRun<Fq>::alloc(c, pb, &rbB1, nb);
        MsmRun<Fq>::alloc(c, pz, &rbL, nb);
        MsmRun<Fq>::alloc(c, ph, &rbh, nb);
        MsmRun<Fq2>::alloc(c, pb, &rb2, nb);
        res1 = c.n<XYZZ<Fq>>(4 * (size_t)nb);                                // [nb][A, B1, L, H]
        res2 = c.n<XYZZ<Fq2>>(nb);
        oa = c.n<Affine<Fq>>(nb);
        oc = c.n<Affine<Fq>>(nb);
        ob = c.n<Affine<Fq2>>(nb);
        pc = c.n<XYZZ<Fq>>(nb);                                               // C without MH (k_finish_ab -> k_finish_c)
        abc = c.n<Fr>(h_stride * nb);                                         // [nb][a | b | c], or [nb][a | b] (h_eval)
    };
    // chunk rule (hekaton.h): at most HK_PROVE_BATCH_CHUNK proofs, fewer when that many would not fit in free device memory
    // (the lane's own arena counts as free: reserve() replaces it)
    size_t chunk = batch < (size_t)HK_PROVE_BATCH_CHUNK ? batch : (size_t)HK_PROVE_BATCH_CHUNK;
    if (chunk > 1) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
        size_t avail = free_b + L->arena_cap;
        auto chunk_bytes = [&](size_t nb) { Carve c; chunk_bufs(c, (u32)nb); return c.off; };
        while (chunk > 1 && chunk_bytes(chunk) > avail) chunk--;
    }
    // r | s | kappas of every proof, one row each (k_prep_ext and k_finish_ab read them)
    std::vector<unsigned char> rsk(batch * rs_stride * fr);
    for (size_t b = 0; b < batch; b++) {
        unsigned char* row = rsk.data() + b * rs_stride * fr;
        memcpy(row, rows[b].r, fr);
        memcpy(row + fr, rows[b].s, fr);
        if (n_kappas) memcpy(row + 2 * fr, rows[b].kappas, n_kappas * fr);
    }
    // the chunk's proofs land here and go out row by row once the chunk has settled
    std::vector<Affine<Fq>> ha(chunk), hc(chunk);
    std::vector<Affine<Fq2>> hb(chunk);
    std::vector<const Fr*> zd(chunk);
    const bool prof = ctx->profiling;
    hipEvent_t* ev = L->ev;
    hk_timings acc;
    memset(&acc, 0, sizeof(acc));
    static const EndoSplit<2> endo_g1 = EndoOf<Fq>::split();
    // the five roles on the lane's streams (stream_plan.h): main on L->stream, the others where the role map puts them.
    // One stream (HK_SERIAL_STREAMS=1, or one hardware queue per lane) runs everything in submission order: clean
    // per-kernel times for profiling.  A fork or join between two roles on one stream is no event wait at all.
    hipStream_t rs[PROVE_ROLES];
    for (int r = 0; r < PROVE_ROLES; r++) rs[r] = L->stream_at(prove_role_stream(L->n_streams, (ProveRole)r));
    hipStream_t s = rs[ROLE_MAIN];
    auto wait = [](hipStream_t to, hipEvent_t e, hipStream_t from) -> hk_status {
        if (to != from) HK_HIP(hipStreamWaitEvent(to, e, 0));
        return HK_OK;
    };
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const u32 nb = (u32)std::min(chunk, batch - b0);
        HK_TRY(L->carve([&](Carve& c) { chunk_bufs(c, nb); }));
        // ev[0] marks the start of the call (total_ms runs from it to the last chunk's ev[8]), ev[9] that of a later chunk
        hipEvent_t ev_start = b0 ? ev[9] : ev[0];
        if (prof) HK_HIP(hipEventRecord(ev_start, s));
        // --- extended scalar vectors [nb][n_ext]: row j's z on the device (a host row through its zt slot), then z[1..]
        for (u32 j = 0; j < nb; j++) {
            if (z_dev[b0 + j]) zd[j] = (const Fr*)rows[b0 + j].z;
            else {
                HK_HIP(hipMemcpyAsync(zt + (size_t)j * n_v, rows[b0 + j].z, n_v * fr, hipMemcpyHostToDevice, s));
                zd[j] = zt + (size_t)j * n_v;
            }
            if (n_v > 1)
                HK_HIP(hipMemcpyAsync(zext + (size_t)j * pk->n_ext, zd[j] + 1, (n_v - 1) * fr, hipMemcpyDeviceToDevice, s));
        }
        HK_HIP(hipMemcpyAsync(small, rsk.data() + b0 * rs_stride * fr, nb * rs_stride * fr, hipMemcpyHostToDevice, s));
        // --- one digit sort per proof for the four assignment-indexed queries: L reads its list as it is, A and B too, or -
        // when they run over their non-infinity bases only - the sub-list of it that their rank table selects
        HK_LAUNCH((k_prep_ext<Fr>), dim3(64), dim3(256), 0, s, zext + (n_v - 1), pk->n_ext, (const Fr*)small,
                  (u32)rs_stride, (u32)n_kappas, nb, sb.count, sbh.count, pz.NB * nb, ph.NB * nb);
        // Fork: the five queries are independent once their scalars exist.  Streams let the latency-bound tails
        // (segmented levels, bucket reduction) of one query hide under the throughput-bound accumulation of another;
        // every launch covers the whole chunk.
        //   main : sort(z) -> A -> finish_ab -> finish_c     B1      B2 (G2)      L      H : witness map -> sort(h) -> H
        hipStream_t sB1 = rs[ROLE_B1], sB2 = rs[ROLE_B2], sL = rs[ROLE_L], sH = rs[ROLE_H];
        hipEvent_t ev_z = ev[16], ev_sorted = ev[17];
        HK_HIP(hipEventRecord(ev_z, s));                                       // z (and ext scalars) on device
        auto submit_h = [&]() -> hk_status {
            HK_TRY(wait(sH, ev_z, s));
            if (prof) HK_HIP(hipEventRecord(ev[5], sH));
            for (u32 j = 0; j < nb; j++) {                                      // witness map: one chain per proof
                if (pk->h_eval)
                    HK_TRY(Q::run_eval(sH, T, pk->csr[0], pk->csr[1], pk->n_inst, pk->n_c, zd[j], abc + j * h_stride, pk->log_m));
                else
                    HK_TRY(Q::run(sH, T, pk->csr[0], pk->csr[1], pk->csr[2], pk->n_inst, pk->n_c, zd[j],
                                  abc + j * h_stride, pk->log_m));
            }
            if (prof) HK_HIP(hipEventRecord(ev[6], sH));                       // witness map done
            HK_TRY(MsmSort<Fr>::run(sH, ph, (const u32*)abc, 1, sbh, true, nb, h_stride));
            HK_TRY(MsmRun<Fq>::run(sH, ph, pk->h_tab, (u32)m, 0, sbh, rbh, res1 + 3, prof ? ev[12] : nullptr,
                                   prof ? ev[13] : nullptr, nb, 4));
            HK_HIP(hipEventRecord(ev[7], sH));                                 // H done
            return HK_OK;
        };
        // Submitting the H chain's hundred-odd launches takes the host milliseconds, and a stream starts only once its
        // work is submitted.  H is the longest role when the queries have streams of their own, so it goes first; on
        // two streams the four queries in a row are longer than H (profiles/queues_*), so they go first there.
        const bool h_first = L->n_streams >= 3;
        if (h_first) HK_TRY(submit_h());
        HK_TRY(MsmSort<Fr>::run(s, pz, (const u32*)zext, 1, sb, true, nb, pk->n_ext));
        HK_HIP(hipEventRecord(ev_sorted, s));
        if (prof) HK_HIP(hipEventRecord(ev[1], s));                            // digits done
        HK_TRY(wait(sL, ev_sorted, s));
        const SortBufs *sbA = &sb, *sbB = &sb;
        HK_TRY(wait(sB1, ev_sorted, s));
        if (pk->b_compact) {
            // B1 / B2 over the non-infinity bases only: their entries of z's list, derived on B1's stream
            HK_TRY(MsmSort<Fr>::sublist(sB1, pz, sb, pb, pk->b_rank, sbb, nb));
            HK_HIP(hipEventRecord(ev[28], sB1));
            HK_TRY(wait(sB2, ev[28], sB1));
            sbB = &sbb;
        } else {
            HK_TRY(wait(sB2, ev_sorted, s));
        }
        HK_TRY(MsmRun<Fq2>::run(sB2, pb, pk->b2_tab, pk->b_n, 0, *sbB, rb2, res2, nullptr, nullptr, nb, 1));
        HK_HIP(hipEventRecord(ev[4], sB2));                                    // B2 done
        HK_TRY(MsmRun<Fq>::run(sB1, pb, pk->b1_tab, pk->b_n, 0, *sbB, rbB1, res1 + 1, prof ? ev[22] : nullptr,
                               prof ? ev[23] : nullptr, nb, 4));
        HK_HIP(hipEventRecord(ev[3], sB1));                                    // B1 done
        HK_TRY(MsmRun<Fq>::run(sL, pz, pk->l_tab, pk->l_n, pk->l_off, sb, rbL, res1 + 2, prof ? ev[24] : nullptr,
                               prof ? ev[25] : nullptr, nb, 4));
        HK_HIP(hipEventRecord(ev[18], sL));                                    // L done
        if (pk->a_compact) {
            // A likewise, on main: a base at infinity no longer takes a lane of the wave through the mixed add
            HK_TRY(MsmSort<Fr>::sublist(s, pz, sb, pa, pk->a_rank, sba, nb));
            sbA = &sba;
        }
        HK_TRY(MsmRun<Fq>::run(s, pa, pk->a_tab, pk->a_n, 0, *sbA, rbA, res1 + 0, prof ? ev[26] : nullptr,
                               prof ? ev[27] : nullptr, nb, 4));
        if (prof) HK_HIP(hipEventRecord(ev[2], s));                            // A done
        // Join the queries: A, B, and C without MH need nothing of H, so they no longer wait for it
        HK_TRY(wait(s, ev[3], sB1));
        HK_TRY(wait(s, ev[4], sB2));
        HK_TRY(wait(s, ev[18], sL));
        HK_LAUNCH((k_finish_ab<Fr, Fq, Fq2>), dim3(3, nb), dim3(64), 0, s, res1, res2, pk->consts_g1, pk->consts_g2,
                  (const Fr*)small, (u32)rs_stride, oa, ob, pc, endo_g1);
        if (!h_first) HK_TRY(submit_h());
        // Join H
        HK_TRY(wait(s, ev[7], sH));
        if (prof) HK_HIP(hipEventRecord(ev[19], s));                           // all queries and finish_ab done
        HK_LAUNCH((k_finish_c<Fq>), dim3(1), dim3(64), 0, s, (const XYZZ<Fq>*)pc, (const XYZZ<Fq>*)res1, oc, nb);
        HK_HIP(hipMemcpyAsync(ha.data(), oa, nb * sizeof(Affine<Fq>), hipMemcpyDeviceToHost, s));
        HK_HIP(hipMemcpyAsync(hb.data(), ob, nb * sizeof(Affine<Fq2>), hipMemcpyDeviceToHost, s));
        HK_HIP(hipMemcpyAsync(hc.data(), oc, nb * sizeof(Affine<Fq>), hipMemcpyDeviceToHost, s));
        if (prof) HK_HIP(hipEventRecord(ev[8], s));
        HK_TRY(L->settle());
        for (u32 j = 0; j < nb; j++) {
            memcpy(rows[b0 + j].a, &ha[j], sizeof(Affine<Fq>));
            memcpy(rows[b0 + j].b, &hb[j], sizeof(Affine<Fq2>));
            memcpy(rows[b0 + j].c, &hc[j], sizeof(Affine<Fq>));
        }
        if (prof) {
            // the five queries run concurrently where they have streams of their own: each figure is the elapsed time on
            // the query's stream since its fork point (they overlap, they do not add up to total_ms; roles that share a
            // stream include the work queued before them there); summed over the chunks.  finish_ms: k_finish_c and the
            // copies, from the moment H and k_finish_ab are both done.
            acc.digits_ms += ev_ms(ev_start, ev[1]);
            acc.msm_a_ms += ev_ms(ev[1], ev[2]);
            // every query forks from the shared sort (ev[1]), a compact one with its sub-list first: no figure is negative
            acc.msm_b_g1_ms += ev_ms(ev[1], ev[3]);
            acc.msm_b_g2_ms += ev_ms(ev[1], ev[4]);
            acc.msm_l_ms += ev_ms(ev[1], ev[18]);
            acc.witness_map_ms += ev_ms(ev[5], ev[6]);
            acc.msm_h_ms += ev_ms(ev[6], ev[7]);
            acc.finish_ms += ev_ms(ev[19], ev[8]);
            // the k_msm_accum0<Fq> launches of the chunk: H (dense) + A, B1, L (sparse)
            float kh = ev_ms(ev[12], ev[13]);
            acc.accum_h_ms += kh;
            acc.accum_kernel_ms += kh + ev_ms(ev[22], ev[23]) + ev_ms(ev[24], ev[25]) + ev_ms(ev[26], ev[27]);
            acc.accum_kernel_launches += 4;
        }
    }
    if (prof) {
        acc.total_ms = ev_ms(ev[0], ev[8]);
        acc.batch_proofs = (uint32_t)chunk;
        L->timings = acc;
    }
    return HK_OK;
}

}  // namespace hk
