// pk.cuh — the device-resident proving key: its tables (shift tables of every query, the compacted A and B queries, the
// h query - in the coset's evaluation basis, or bit-reversed in the coefficient basis - the matrices) and the one-time work
// that builds them.  Defines Ops<C>::pk_upload (hk_pk_upload) and
// Ops<C>::pk_free (hk_pk_free).
#pragma once
#include "ntt_host.cuh"
#include "csr.cuh"
#include "h_basis.cuh"

namespace hk {

// ---- device-resident proving key ------------------------------------------------------------------------
template <class C>
struct PkImpl {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    u32 n_v = 0, n_inst = 0, n_c = 0, n_stages = 0, n_ext = 0, n_extra = 0;
    MsmPlan plan_z;                        // the one digit sort of the assignment: A / B1 / B2 / L read its list
    Affine<Fq>* a_tab = nullptr;           // [F][n_ext]   a_g[1..] | delta_g | inf ...
    Affine<Fq>* b1_tab = nullptr;          // [F][n_ext]   b_g[1..] | inf | delta_g | inf ...
    Affine<Fq2>* b2_tab = nullptr;         // [F][n_ext]   b_h[1..] | inf | delta_h | inf ...
    // Query density (bellman's DensityTracker idea): a_g[i] is infinity for every variable that never occurs in A, b_g[i]
    // and b_h[i] for every one that never occurs in B.  When enough of a query's bases are (msm_compact_rule), it runs over
    // a compacted index list (ext indices of the non-infinity bases, then every ext slot): its tables then hold
    // [F][a_n] / [F][b_n] entries, plan_a / plan_b (msm_sub_plan of plan_z: same windows, same buckets) replaces plan_z
    // for it, and its entry list is the sub-list of z's sorted list that a_rank / b_rank - the inverse of the index list
    // over the n_ext scalars - selects (MsmSort::sublist).  A query that does not meet the rule reads z's list as it is.
    bool a_compact = false, b_compact = false;
    u32 a_n = 0, b_n = 0;
    u32 *a_rank = nullptr, *b_rank = nullptr;
    MsmPlan plan_a, plan_b;
    Affine<Fq>* l_tab = nullptr;           // [F][l_n]     ck_last | inf | inf | -delta_g | -delta_i ...
    u32 l_n = 0, l_off = 0;                // h_eval: every ext index (l_off = 0, l_n = n_ext), variable k holds -C^_k, a
                                           // last-stage witness ck_last_k - C^_k (h_basis.cuh)
    bool has_qap = false;
    // the H query in the coset's evaluation basis (h_basis.cuh; the default for a key with a QAP, HK_H_BASIS=coeff at upload
    // keeps the coefficient basis): the prover runs QapHost::run_eval - four transforms, no C pass - on 2 m Fr per proof
    bool h_eval = false;
    u32 log_m = 0;
    MsmPlan plan_h;
    Affine<Fq>* h_tab = nullptr;           // [F][m]  h_g in bit-reversed order (slot m-1 = inf); h_eval: G^_j / m^2, natural
    std::vector<MsmPlan> plan_ck;
    std::vector<Affine<Fq>*> ck_tab;       // [F][ck_len + 1]  ck[stage] | last_delta_g
    std::vector<u32> ck_n;
    Affine<Fq>* consts_g1 = nullptr;       // a_g[0], alpha_g, b_g[0], beta_g, -C^_0 (inf unless h_eval)
    Affine<Fq2>* consts_g2 = nullptr;      // b_h[0], beta_h
    CsrDev csr[3];
    std::vector<void*> owned;              // every hipMalloc of this key
    size_t bytes = 0;
};

template <class F>
static hk_status pk_alloc_table(std::vector<void*>& owned, size_t& total, size_t groups, size_t n,
                                Affine<F>** out) {
    size_t b = groups * n * sizeof(Affine<F>);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, b ? b : 16);
    if (e != hipSuccess) { (void)hipGetLastError(); return HK_ERR_NOMEM; }
    owned.push_back(p);
    total += b;
    *out = (Affine<F>*)p;
    return HK_OK;
}

// scatter h_g into bit-reversed order on the device: tab[bitrev(j)] = h_g[j], j < h_len; others inf
template <class F>
__global__ void k_pk_bitrev_copy(Affine<F>* __restrict__ tab, const Affine<F>* __restrict__ src, u32 h_len,
                                 u32 log_m) {
    u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >> log_m) return;
    u32 r = log_m ? (__brev(j) >> (32 - log_m)) : 0u;
    Affine<F> p = j < h_len ? ld_vec(&src[j]) : Affine<F>::inf();
    st_vec(&tab[r], p);
}

// flags[i] = 1 iff pts[i] is not the point at infinity
template <class F>
__global__ void k_mark_noninf(const Affine<F>* __restrict__ pts, u32* __restrict__ flags, u32 n) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = ld_vec(&pts[i]).is_inf() ? 0u : 1u;
}
// dst[k] = src[idx[k]] for idx[k] < n_src (ext slots beyond the source stay as they are), for the row of grid.y: dst rows
// n apart, src rows n_src apart, one index list
template <class T>
__global__ void k_gather(T* __restrict__ dst, const T* __restrict__ src, const u32* __restrict__ idx, u32 n, u32 n_src) {
    u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const size_t pr = blockIdx.y;
    u32 i = idx[k];
    if (i < n_src) st_vec(&dst[pr * n + k], ld_vec(&src[pr * n_src + i]));
}

// error exits of pk_upload: release everything allocated so far (fail()) and tell out-of-memory from other faults
#define PK_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            (void)hipGetLastError();                                                          \
            fprintf(stderr, "[hekaton] HIP error %s at %s:%d: %s\n", hipGetErrorName(_e), __FILE__, __LINE__, #expr); \
            return fail(_e == hipErrorOutOfMemory ? HK_ERR_NOMEM : HK_ERR_DEVICE);            \
        }                                                                                     \
    } while (0)
#define PK_TRY(expr)                               \
    do {                                           \
        hk_status _s = (expr);                     \
        if (_s != HK_OK) return fail(_s);          \
    } while (0)

template <class C>
hk_status Ops<C>::pk_upload(hk_ctx* ctx, const hk_pk_desc* d, hk_pk** out) {
    typedef PkImpl<C> PK;
    *out = nullptr;
    if (!d->a_g || !d->b_g || !d->b_h || !d->h_g || !d->deltas_g || !d->last_delta_h || !d->alpha_g ||
        !d->beta_g || !d->beta_h || d->n_stages == 0 || !d->ck_stage || !d->ck_len)
        return HK_ERR_ARG;
    size_t n_v = d->a_len;
    if (n_v < 1 || d->b_g_len != n_v || d->b_h_len != n_v) return HK_ERR_LEN;
    if (n_v + d->n_stages + 4 >= ((size_t)1 << MSM_ENTRY_GROUP_SHIFT)) return HK_ERR_ARG;   // sorted-entry index field
    size_t n_wit = 0;
    for (size_t s = 0; s < d->n_stages; s++) n_wit += d->ck_len[s];
    if (d->n_inst < 1 || d->n_inst + n_wit != n_v) return HK_ERR_LEN;   // instance || stage witnesses
    HK_HIP(hipSetDevice(ctx->device));
    PK* pk = new PK();
    hk_pk* h = new hk_pk{ctx->ops, ctx, pk};
    void *staging = nullptr, *hb_tmp = nullptr;       // transient: device copy of h_g; G and -C^ (freed on every exit)
    auto fail = [&](hk_status st) {
        if (staging) (void)hipFree(staging);
        if (hb_tmp) (void)hipFree(hb_tmp);
        Ops<C>::pk_free(h);
        return st;
    };
    const bool has_qap = d->A && d->B && d->C;
    pk->h_eval = has_qap && hb_eval_form(getenv("HK_H_BASIS"));
    pk->n_v = (u32)n_v; pk->n_inst = (u32)d->n_inst; pk->n_c = (u32)d->n_constraints;
    pk->n_stages = (u32)d->n_stages;
    u32 k = pk->n_stages - 1;
    pk->n_extra = 3 + k;                               // r, s, r*s, kappa_0..kappa_{k-1}
    pk->n_ext = (u32)(n_v - 1) + pk->n_extra;
    const char* wp_env = getenv("HK_MSM_WP");
    u32 WP = wp_env && atoi(wp_env) > 0 ? (u32)atoi(wp_env) : 1u;
    auto make_plan = [&](size_t n) {
        u32 c = msm_pick_c_tables(n, C::FR_BITS);
        if (WP > 1) { while (c > 5 && ((u64)WP << (c - 1)) > (u64)MSM_LDS_COUNTERS) c--; }
        return msm_make_plan((u32)n, C::FR_BITS, c, WP, ctx->max_lanes0, C::Fr::Params::MOD, C::Fr::Params::N);
    };
    pk->plan_z = make_plan(pk->n_ext);
    const MsmPlan& pz = pk->plan_z;
    hipStream_t s0 = 0;
    size_t g1 = sizeof(Affine<Fq>), g2 = sizeof(Affine<Fq2>);
    size_t nq = n_v - 1;                                // query[1..]
    Affine<Fq> inf1 = Affine<Fq>::inf();
    // --- A / B1 / B2 tables
    hk_status st;
    const char* a_g = (const char*)d->a_g; const char* b_g = (const char*)d->b_g; const char* b_h = (const char*)d->b_h;
    const char* deltas = (const char*)d->deltas_g;
    const char* delta_last_g = deltas + g1 * k;
    u32 shift = pz.c * pz.WP;
    {
        // A and B queries: full-size staging copies on the device, then either used as the tables' first group or
        // compacted to the non-infinity bases
        Affine<Fq>*sa = nullptr, *sb1 = nullptr; Affine<Fq2>* sb2 = nullptr; u32* flags = nullptr;
        std::vector<void*> tmp;
        auto cleanup = [&]() { for (void* q : tmp) (void)hipFree(q); tmp.clear(); };
        auto tfail = [&](hk_status e) { cleanup(); return fail(e); };
        auto talloc = [&](void** q, size_t b) { if (hipMalloc(q, b ? b : 16) != hipSuccess) { (void)hipGetLastError(); return false; } tmp.push_back(*q); return true; };
        if (!talloc((void**)&sa, g1 * (nq + 1)) || !talloc((void**)&sb1, g1 * (nq + 1)) || !talloc((void**)&sb2, g2 * (nq + 1)) ||
            !talloc((void**)&flags, 4 * (nq + 1)))
            return tfail(HK_ERR_NOMEM);
        if (nq) {
            if (hipMemcpy(sa, a_g + g1, g1 * nq, h2d_kind(a_g)) != hipSuccess) return tfail(HK_ERR_DEVICE);
            if (hipMemcpy(sb1, b_g + g1, g1 * nq, h2d_kind(b_g)) != hipSuccess) return tfail(HK_ERR_DEVICE);
            if (hipMemcpy(sb2, b_h + g2, g2 * nq, h2d_kind(b_h)) != hipSuccess) return tfail(HK_ERR_DEVICE);
        }
        static const char* dens_env = getenv("HK_B_COMPACT_BELOW");     // density threshold in percent; 0 disables
        double thr = dens_env ? atof(dens_env) / 100.0 : 0.75;
        // one query's selection from its staged G1 bases: compact or not, its length and plan, the index list (device,
        // transient: the table gathers read it) and the rank table (device, kept with the key)
        auto select = [&](const Affine<Fq>* staged, bool* compact, u32* n_out, MsmPlan* plan, u32** idx_d, u32** rank_d) -> hk_status {
            std::vector<u32> idx;
            if (nq) {
                HK_LAUNCH((k_mark_noninf<Fq>), dim3((u32)((nq + 255) / 256)), dim3(256), 0, s0, staged, flags, (u32)nq);
                std::vector<u32> hf(nq);
                if (hipMemcpy(hf.data(), flags, 4 * nq, hipMemcpyDeviceToHost) != hipSuccess) return HK_ERR_DEVICE;
                for (size_t i = 0; i < nq; i++) if (hf[i]) idx.push_back((u32)i);
            }
            *compact = msm_compact_rule(nq, idx.size(), thr);
            *idx_d = *rank_d = nullptr;
            if (!*compact) {
                *n_out = pk->n_ext;
                *plan = pz;
                return HK_OK;
            }
            for (u32 e = 0; e < pk->n_extra; e++) idx.push_back((u32)nq + e);
            *n_out = (u32)idx.size();
            *plan = msm_sub_plan(pz, *n_out, ctx->max_lanes0);
            std::vector<u32> rank(pk->n_ext);
            msm_rank_table(idx.data(), idx.size(), rank.data(), rank.size());
            if (!talloc((void**)idx_d, 4 * idx.size())) return HK_ERR_NOMEM;
            void* dr = nullptr;
            if (hipMalloc(&dr, 4 * rank.size()) != hipSuccess) { (void)hipGetLastError(); return HK_ERR_NOMEM; }
            pk->owned.push_back(dr);
            pk->bytes += 4 * rank.size();
            *rank_d = (u32*)dr;
            if (hipMemcpy(*idx_d, idx.data(), 4 * idx.size(), hipMemcpyHostToDevice) != hipSuccess) return HK_ERR_DEVICE;
            if (hipMemcpy(dr, rank.data(), 4 * rank.size(), hipMemcpyHostToDevice) != hipSuccess) return HK_ERR_DEVICE;
            return HK_OK;
        };
        u32 *a_idx = nullptr, *b_idx = nullptr;
        if ((st = select(sa, &pk->a_compact, &pk->a_n, &pk->plan_a, &a_idx, &pk->a_rank)) != HK_OK) return tfail(st);
        if ((st = select(sb1, &pk->b_compact, &pk->b_n, &pk->plan_b, &b_idx, &pk->b_rank)) != HK_OK) return tfail(st);
        if ((st = pk_alloc_table(pk->owned, pk->bytes, pz.F, pk->a_n, &pk->a_tab)) != HK_OK) return tfail(st);
        if ((st = pk_alloc_table(pk->owned, pk->bytes, pz.F, pk->b_n, &pk->b1_tab)) != HK_OK) return tfail(st);
        if ((st = pk_alloc_table(pk->owned, pk->bytes, pz.F, pk->b_n, &pk->b2_tab)) != HK_OK) return tfail(st);
        if (hipMemset(pk->a_tab, 0, g1 * pk->a_n) != hipSuccess || hipMemset(pk->b1_tab, 0, g1 * pk->b_n) != hipSuccess ||
            hipMemset(pk->b2_tab, 0, g2 * pk->b_n) != hipSuccess)
            return tfail(HK_ERR_DEVICE);
        if (pk->a_compact) {
            if (HK_LAUNCH_STATUS((k_gather<Affine<Fq>>), dim3((pk->a_n + 255) / 256), dim3(256), 0, s0, pk->a_tab, (const Affine<Fq>*)sa, (const u32*)a_idx, pk->a_n, (u32)nq) != HK_OK) return tfail(HK_ERR_DEVICE);
        } else if (nq) {
            if (hipMemcpy(pk->a_tab, sa, g1 * nq, hipMemcpyDeviceToDevice) != hipSuccess) return tfail(HK_ERR_DEVICE);
        }
        if (pk->b_compact) {
            u32 blocks = (pk->b_n + 255) / 256;
            if (HK_LAUNCH_STATUS((k_gather<Affine<Fq>>), dim3(blocks), dim3(256), 0, s0, pk->b1_tab, (const Affine<Fq>*)sb1, (const u32*)b_idx, pk->b_n, (u32)nq) != HK_OK) return tfail(HK_ERR_DEVICE);
            if (HK_LAUNCH_STATUS((k_gather<Affine<Fq2>>), dim3(blocks), dim3(256), 0, s0, pk->b2_tab, (const Affine<Fq2>*)sb2, (const u32*)b_idx, pk->b_n, (u32)nq) != HK_OK) return tfail(HK_ERR_DEVICE);
        } else if (nq) {
            if (hipMemcpy(pk->b1_tab, sb1, g1 * nq, hipMemcpyDeviceToDevice) != hipSuccess) return tfail(HK_ERR_DEVICE);
            if (hipMemcpy(pk->b2_tab, sb2, g2 * nq, hipMemcpyDeviceToDevice) != hipSuccess) return tfail(HK_ERR_DEVICE);
        }
        u32 r_slot = pk->a_n - pk->n_extra + 0, s_slot = pk->b_n - pk->n_extra + 1;              // ext slots of r (in A), s (in B)
        if (hipMemcpy(pk->a_tab + r_slot, delta_last_g, g1, h2d_kind(deltas)) != hipSuccess) return tfail(HK_ERR_DEVICE);      // r * delta_g
        if (hipMemcpy(pk->b1_tab + s_slot, delta_last_g, g1, h2d_kind(deltas)) != hipSuccess) return tfail(HK_ERR_DEVICE);     // s * delta_g
        if (hipMemcpy(pk->b2_tab + s_slot, d->last_delta_h, g2, h2d_kind(d->last_delta_h)) != hipSuccess) return tfail(HK_ERR_DEVICE);   // s * delta_h
        if (hipDeviceSynchronize() != hipSuccess) return tfail(HK_ERR_DEVICE);
        cleanup();
        PK_TRY(MsmRun<Fq>::build_tables(s0, pk->a_tab, pk->a_n, pz.F, shift));
        PK_TRY(MsmRun<Fq>::build_tables(s0, pk->b1_tab, pk->b_n, pz.F, shift));
        PK_TRY(MsmRun<Fq2>::build_tables(s0, pk->b2_tab, pk->b_n, pz.F, shift));
    }
    // --- L table: last-stage committer key, then the negated deltas that fold -rs*delta and -kappa_i*delta_i
    // (an evaluation-basis key: over every ext index, its variable rows filled and its shift tables built with the QAP below)
    size_t n1 = d->ck_len[k];
    const size_t l_rows = pk->h_eval ? n_v - 1 : n1;    // rows in front of r | s | rs | kappa
    pk->l_n = (u32)l_rows + pk->n_extra;
    pk->l_off = (u32)(n_v - 1 - l_rows);                // ext index of the table's first row
    if ((st = pk_alloc_table(pk->owned, pk->bytes, pz.F, pk->l_n, &pk->l_tab)) != HK_OK) return fail(st);
    PK_HIP(hipMemset(pk->l_tab, 0, g1 * pk->l_n));
    if (n1 && !pk->h_eval) PK_HIP(hipMemcpy(pk->l_tab, d->ck_stage[k], g1 * n1, h2d_kind(d->ck_stage[k])));
    {
        std::vector<Affine<Fq>> dh(k + 1);
        PK_HIP(hipMemcpy(dh.data(), deltas, g1 * (k + 1), is_device_ptr(deltas) ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
        std::vector<Affine<Fq>> neg(1 + k);
        neg[0] = dh[k].is_inf() ? dh[k] : ec_neg(dh[k]);                       // -delta_g  (scalar r*s)
        for (u32 i = 0; i < k; i++) neg[1 + i] = dh[i].is_inf() ? dh[i] : ec_neg(dh[i]);   // -delta_i (kappa_i)
        PK_HIP(hipMemcpy(pk->l_tab + l_rows + 2, neg.data(), g1 * (1 + k), hipMemcpyHostToDevice));
    }
    if (!pk->h_eval) PK_TRY(MsmRun<Fq>::build_tables(s0, pk->l_tab, pk->l_n, pz.F, shift));
    // --- per-stage commitment tables: ck[stage] | last_delta_g (scalar kappa)
    for (u32 sidx = 0; sidx < pk->n_stages; sidx++) {
        size_t n = d->ck_len[sidx] + 1;
        MsmPlan p = make_plan(n);
        Affine<Fq>* tab;
        if ((st = pk_alloc_table(pk->owned, pk->bytes, p.F, n, &tab)) != HK_OK) return fail(st);
        if (n > 1) PK_HIP(hipMemcpy(tab, d->ck_stage[sidx], g1 * (n - 1), h2d_kind(d->ck_stage[sidx])));
        PK_HIP(hipMemcpy(tab + n - 1, delta_last_g, g1, h2d_kind(deltas)));
        PK_TRY(MsmRun<Fq>::build_tables(s0, tab, (u32)n, p.F, p.c * p.WP));
        pk->plan_ck.push_back(p);
        pk->ck_tab.push_back(tab);
        pk->ck_n.push_back((u32)n);
    }
    // --- constants for the finish kernel
    {
        void* p1; void* p2;
        PK_HIP(hipMalloc(&p1, g1 * 5)); pk->owned.push_back(p1);
        PK_HIP(hipMalloc(&p2, g2 * 2)); pk->owned.push_back(p2);
        pk->consts_g1 = (Affine<Fq>*)p1; pk->consts_g2 = (Affine<Fq2>*)p2;
        PK_HIP(hipMemset(pk->consts_g1 + 4, 0, g1));
        PK_HIP(hipMemcpy(pk->consts_g1 + 0, a_g, g1, h2d_kind(a_g)));
        PK_HIP(hipMemcpy(pk->consts_g1 + 1, d->alpha_g, g1, h2d_kind(d->alpha_g)));
        PK_HIP(hipMemcpy(pk->consts_g1 + 2, b_g, g1, h2d_kind(b_g)));
        PK_HIP(hipMemcpy(pk->consts_g1 + 3, d->beta_g, g1, h2d_kind(d->beta_g)));
        PK_HIP(hipMemcpy(pk->consts_g2 + 0, b_h, g2, h2d_kind(b_h)));
        PK_HIP(hipMemcpy(pk->consts_g2 + 1, d->beta_h, g2, h2d_kind(d->beta_h)));
    }
    // --- QAP: matrices + H-query, in the coset's evaluation basis or bit-reversed in the coefficient basis
    if (has_qap) {
        if (d->A->n_rows != d->n_constraints || d->B->n_rows != d->n_constraints ||
            d->C->n_rows != d->n_constraints)
            return fail(HK_ERR_LEN);
        pk->log_m = QapHost<C>::domain_log(d->n_constraints, d->n_inst);
        if (pk->log_m > C::TWO_ADICITY || pk->log_m > (u32)MSM_ENTRY_GROUP_SHIFT) return fail(HK_ERR_DOMAIN_TOO_LARGE);
        size_t m = (size_t)1 << pk->log_m;
        if (d->h_len + 1 != m) return fail(HK_ERR_LEN);                 // prover.rs:128 assert
        const hk_csr* Ms[3] = {d->A, d->B, d->C};
        if (!csr_host_ok(d->A) || !csr_host_ok(d->B) || !csr_host_ok(d->C)) return fail(HK_ERR_ARG);
        for (int i = 0; i < 3; i++) {
            void *rp, *cl, *vl;
            PK_HIP(hipMalloc(&rp, 8 * (Ms[i]->n_rows + 1))); pk->owned.push_back(rp);
            PK_HIP(hipMalloc(&cl, 4 * Ms[i]->nnz + 16)); pk->owned.push_back(cl);
            PK_HIP(hipMalloc(&vl, sizeof(Fr) * Ms[i]->nnz + 16)); pk->owned.push_back(vl);
            PK_HIP(hipMemcpy(rp, Ms[i]->row_ptr, 8 * (Ms[i]->n_rows + 1), h2d_kind(Ms[i]->row_ptr)));
            if (Ms[i]->nnz) {
                PK_HIP(hipMemcpy(cl, Ms[i]->col, 4 * Ms[i]->nnz, h2d_kind(Ms[i]->col)));
                PK_HIP(hipMemcpy(vl, Ms[i]->val_mont, sizeof(Fr) * Ms[i]->nnz, h2d_kind(Ms[i]->val_mont)));
            }
            pk->csr[i] = {(const u64*)rp, (const u32*)cl, vl, Ms[i]->n_rows, Ms[i]->nnz};
            pk->bytes += 8 * (Ms[i]->n_rows + 1) + (4 + sizeof(Fr)) * Ms[i]->nnz;
        }
        {
            // a malformed matrix (column >= n_v, row_ptr not monotone / not ending at nnz) is HK_ERR_ARG here,
            // not an out-of-bounds read in every later hk_prove
            void* flag = nullptr;
            PK_HIP(hipMalloc(&flag, 256)); pk->owned.push_back(flag);
            PK_TRY(r1cs_validate(s0, pk->csr, n_v, (u32*)flag));
        }
        pk->plan_h = make_plan(m);
        if ((st = pk_alloc_table(pk->owned, pk->bytes, pk->plan_h.F, m, &pk->h_tab)) != HK_OK) return fail(st);
        const Affine<Fq>* src = (const Affine<Fq>*)d->h_g;
        if (!is_device_ptr(d->h_g)) {
            PK_HIP(hipMalloc(&staging, g1 * (d->h_len ? d->h_len : 1)));
            PK_HIP(hipMemcpy(staging, d->h_g, g1 * d->h_len, hipMemcpyHostToDevice));
            src = (const Affine<Fq>*)staging;
        }
        NttTables* T;
        PK_TRY(NttHost<C>::ensure(ctx, pk->log_m, &T));
        if (pk->h_eval) {
            // h_tab = G^ / m^2 in natural order; G, then -C^ (+ the last stage's committer key) behind it, are transient
            PK_HIP(hipMalloc(&hb_tmp, g1 * (m + n_v)));
            Affine<Fq>*gd = (Affine<Fq>*)hb_tmp, *cd = gd + m;
            PK_TRY(HBasis<C>::transform(ctx, T, src, (u32)d->h_len, pk->log_m, pk->h_tab, gd));
            PK_TRY(HBasis<C>::c_columns(ctx, pk->csr[2], n_v, pk->log_m, gd, d->ck_stage[k], n1, cd));
            if (nq) PK_HIP(hipMemcpy(pk->l_tab, cd + 1, g1 * nq, hipMemcpyDeviceToDevice));
            PK_HIP(hipMemcpy(pk->consts_g1 + 4, cd, g1, hipMemcpyDeviceToDevice));      // z_0 = 1: -C^_0 joins C's constants
            (void)hipFree(hb_tmp); hb_tmp = nullptr;
            PK_TRY(MsmRun<Fq>::build_tables(s0, pk->l_tab, pk->l_n, pz.F, shift));
        } else {
            PK_TRY(HK_LAUNCH_STATUS((k_pk_bitrev_copy<Fq>), dim3((u32)((m + 255) / 256)), dim3(256), 0, s0, pk->h_tab,
                                    src, (u32)d->h_len, pk->log_m));
            PK_HIP(hipDeviceSynchronize());
        }
        if (staging) { (void)hipFree(staging); staging = nullptr; }
        PK_TRY(MsmRun<Fq>::build_tables(s0, pk->h_tab, (u32)m, pk->plan_h.F, pk->plan_h.c * pk->plan_h.WP));
        pk->has_qap = true;
    }
    PK_HIP(hipDeviceSynchronize());
    *out = h;
    return HK_OK;
}

#undef PK_HIP
#undef PK_TRY

template <class C>
void Ops<C>::pk_free(hk_pk* h) {
    if (!h) return;
    PkImpl<C>* pk = (PkImpl<C>*)h->impl;
    (void)hipSetDevice(h->ctx->device);
    (void)hipDeviceSynchronize();
    for (void* p : pk->owned) (void)hipFree(p);
    delete pk;
    delete h;
}

}  // namespace hk
