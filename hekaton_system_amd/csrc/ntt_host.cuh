// ntt_host.cuh — host side of the scalar-field transforms: the context's twiddle / coset tables, the launch sequences of
// ntt.cuh's kernels (NttHost), the witness map over device-resident CSR matrices (QapHost), and the release of what a
// context caches on the device.  Defines Ops<C>::ntt (hk_ntt), Ops<C>::witness_map (hk_witness_map), Ops<C>::ctx_release.
#pragma once
#include "curve_ops_impl.cuh"
#include "ntt.cuh"
#include "ntt_plan.h"
#include "csr.cuh"

namespace hk {

// ---- small host helpers on Montgomery values (setup constants only) -------------------------------
template <class Fr>
static Fr host_halve(const Fr& a) {          // a/2 in the field (works on Montgomery residues too)
    u32 t[Fr::N + 1];
    u64 c = 0;
    bool odd = a.v[0] & 1;
    for (int i = 0; i < Fr::N; i++) {
        c += (u64)a.v[i] + (odd ? Fr::Params::MOD[i] : 0u);
        t[i] = (u32)c;
        c >>= 32;
    }
    t[Fr::N] = (u32)c;
    Fr r;
    for (int i = 0; i < Fr::N; i++) r.v[i] = (t[i] >> 1) | (t[i + 1] << 31);
    return r;
}
template <class Fr>
static Fr host_from_limbs(const u32* l) {
    Fr r;
    for (int i = 0; i < Fr::N; i++) r.v[i] = l[i];
    return r;
}

// ---- twiddle / coset tables (one set per context) ---------------------------------------------------
struct NttTables {
    std::mutex mu;
    u32 log_table = 0;
    void* tw_fwd = nullptr;      // per-stage tables of w (k_stage_tables), 2^log_table - 1 entries; stage s always uses the
                                 // 2^(s+1)-th roots, so every transform size <= 2^log_table shares them
    void* tw_inv = nullptr;      // same for w^-1
    void* pw_g = nullptr;        // 3 x POW_TABLE_SIZE powers of F::GENERATOR
    void* pw_ginv = nullptr;
    std::vector<void*> retired;  // superseded tables stay alive until the context dies
};

template <class C>
struct NttHost {
    typedef typename C::Fr Fr;

    static hk_status ensure(hk_ctx* ctx, u32 log_m, NttTables** out) {
        if (log_m > C::TWO_ADICITY) return HK_ERR_DOMAIN_TOO_LARGE;
        std::unique_lock<std::mutex> lk(ctx->mu);
        if (!ctx->ntt) ctx->ntt = new NttTables();
        NttTables* T = ctx->ntt;
        lk.unlock();
        std::unique_lock<std::mutex> tl(T->mu);
        *out = T;
        if (T->log_table >= log_m && T->tw_fwd) return HK_OK;
        u32 L = log_m < 16 ? 16 : log_m;
        if (L > C::TWO_ADICITY) L = C::TWO_ADICITY;
        HK_HIP(hipSetDevice(ctx->device));
        // host: w_M = ROOT^(2^(s-L)); sq[k] = w_M^(2^k); w_M^-1 = prod_k sq[k]
        std::vector<Fr> sq(32), sqi(32);
        Fr w = host_from_limbs<Fr>(C::ROOT);
        for (u32 k = 0; k < C::TWO_ADICITY - L; k++) w = Fr::sqr(w);
        Fr winv = Fr::one();
        for (u32 k = 0; k < L; k++) {
            sq[k] = w;
            winv = Fr::mul(winv, w);
            w = Fr::sqr(w);
        }
        Fr t = winv;
        for (u32 k = 0; k < L; k++) { sqi[k] = t; t = Fr::sqr(t); }
        const u32 NG = 3 * POW_TABLE_BITS;
        std::vector<Fr> gs(NG), gis(NG);
        Fr g = host_from_limbs<Fr>(C::GEN), gi = host_from_limbs<Fr>(C::GEN_INV);
        for (u32 k = 0; k < NG; k++) { gs[k] = g; gis[k] = gi; g = Fr::sqr(g); gi = Fr::sqr(gi); }
        Fr *d_sq = nullptr, *tmp = nullptr, *tf = nullptr, *ti = nullptr, *pg = nullptr, *pgi = nullptr;
        size_t half = (size_t)1 << (L - 1), full = (size_t)1 << L;
        HK_HIP(hipMalloc((void**)&d_sq, sizeof(Fr) * (64 + 2 * NG)));
        HK_HIP(hipMalloc((void**)&tmp, sizeof(Fr) * half));
        HK_HIP(hipMalloc((void**)&tf, sizeof(Fr) * full));
        HK_HIP(hipMalloc((void**)&ti, sizeof(Fr) * full));
        HK_HIP(hipMalloc((void**)&pg, sizeof(Fr) * 3 * POW_TABLE_SIZE));
        HK_HIP(hipMalloc((void**)&pgi, sizeof(Fr) * 3 * POW_TABLE_SIZE));
        HK_HIP(hipMemcpy(d_sq, sq.data(), sizeof(Fr) * 32, hipMemcpyHostToDevice));
        HK_HIP(hipMemcpy(d_sq + 32, sqi.data(), sizeof(Fr) * 32, hipMemcpyHostToDevice));
        HK_HIP(hipMemcpy(d_sq + 64, gs.data(), sizeof(Fr) * NG, hipMemcpyHostToDevice));
        HK_HIP(hipMemcpy(d_sq + 64 + NG, gis.data(), sizeof(Fr) * NG, hipMemcpyHostToDevice));
        u32 blocks = (u32)((half + 255) / 256), blocks_full = (u32)((full + 255) / 256);
        // w_M^i for i < M/2 (scratch), regrouped into one contiguous table per butterfly stage
        HK_LAUNCH((k_pow_table<Fr>), dim3(blocks), dim3(256), 0, 0, tmp, d_sq, (u32)half, L - 1);
        HK_LAUNCH((k_stage_tables<Fr>), dim3(blocks_full), dim3(256), 0, 0, tf, tmp, L);
        HK_LAUNCH((k_pow_table<Fr>), dim3(blocks), dim3(256), 0, 0, tmp, d_sq + 32, (u32)half, L - 1);
        HK_LAUNCH((k_stage_tables<Fr>), dim3(blocks_full), dim3(256), 0, 0, ti, tmp, L);
        for (u32 lvl = 0; lvl < 3; lvl++) {
            HK_LAUNCH((k_pow_table<Fr>), dim3(POW_TABLE_SIZE / 256), dim3(256), 0, 0, pg + POW_TABLE_SIZE * lvl,
                      d_sq + 64 + POW_TABLE_BITS * lvl, (u32)POW_TABLE_SIZE, (u32)POW_TABLE_BITS);
            HK_LAUNCH((k_pow_table<Fr>), dim3(POW_TABLE_SIZE / 256), dim3(256), 0, 0, pgi + POW_TABLE_SIZE * lvl,
                      d_sq + 64 + NG + POW_TABLE_BITS * lvl, (u32)POW_TABLE_SIZE, (u32)POW_TABLE_BITS);
        }
        HK_HIP(hipDeviceSynchronize());
        HK_HIP(hipFree(d_sq));
        HK_HIP(hipFree(tmp));
        for (void* p : {T->tw_fwd, T->tw_inv, T->pw_g, T->pw_ginv})
            if (p) T->retired.push_back(p);
        T->tw_fwd = tf; T->tw_inv = ti; T->pw_g = pg; T->pw_ginv = pgi;
        T->log_table = L;
        return HK_OK;
    }

    static Fr size_inv(u32 log_m) {               // (2^log_m)^-1, Montgomery
        Fr x = Fr::one();
        for (u32 k = 0; k < log_m; k++) x = host_halve(x);
        return x;
    }
    static Fr vanishing_inv_on_coset(u32 log_m) {  // (g^m - 1)^-1  (SURVEY.md A.1 `zinv`)
        Fr g = host_from_limbs<Fr>(C::GEN);
        for (u32 k = 0; k < log_m; k++) g = Fr::sqr(g);
        return fp_inv(Fr::sub(g, Fr::one()));
    }

    // fused epilogue of the last pass (k_ntt_pass4): which steps, on how many of the batched vectors, operands
    struct Post {
        int post = 0;
        u32 nvec = 0xffffffffu;
        const Fr* scale = nullptr;    // post & 1
        const Fr* pw = nullptr;       // post & 2
        const Fr* sub = nullptr;      // post & 4
        const Fr* kc = nullptr;
    };

    // all butterfly stages of a size-2^logn transform, `batch` vectors `stride` elements apart.
    // tws: per-stage twiddle tables.
    static hk_status passes(hipStream_t s, Fr* data, size_t stride, u32 batch, u32 logn, const Fr* tws, int dit,
                            const Post& ep = Post()) {
        if (logn == 0) return HK_OK;
        // bottom pass: the low min(logn, 11) stages on contiguous tiles; the rest in passes of at most
        // `upper_max` stages whose tiles are 2^nst rows of 2^(11 - nst) contiguous elements (ntt_plan.h)
        static const u32 tile_log = [] {
            const char* e = getenv("HK_NTT_TILE_LOG");
            return ntt_plan_tile_log(e ? (u32)atoi(e) : NTT_PLAN_TILE_LOG);
        }();
        static const u32 upper_max = [] {
            const char* e = getenv("HK_NTT_UPPER_MAX");
            return ntt_plan_upper_max(e ? (u32)atoi(e) : NTT_PLAN_UPPER_MAX, tile_log);
        }();
        const u32 threads = 1u << (tile_log - 2);                    // one radix-4 quad per thread
        NttPass ps[NTT_PLAN_MAX_PASSES];
        int np = ntt_pass_plan(logn, tile_log, upper_max, ps);
        Fr one = Fr::one();
        for (int k = 0; k < np; k++) {
            const NttPass& p = dit ? ps[k] : ps[np - 1 - k];
            u32 tile_log = p.nst + p.cols_bits;
            dim3 grid(1u << (logn - tile_log), batch);
            size_t lds = sizeof(Fr) << tile_log;
            bool last = k == np - 1;
            int pp = last ? ep.post : 0;
            const Fr& sc = (pp & 1) ? *ep.scale : one;
            const Fr& kc = (pp & 4) ? *ep.kc : one;
            if (dit)
                HK_LAUNCH((k_ntt_pass4<Fr, 1>), grid, dim3(threads), lds, s, data, stride, tws, logn, p.lo,
                          p.nst, p.cols_bits, pp, ep.nvec, sc, ep.pw, ep.sub, kc);
            else
                HK_LAUNCH((k_ntt_pass4<Fr, 0>), grid, dim3(threads), lds, s, data, stride, tws, logn, p.lo,
                          p.nst, p.cols_bits, pp, ep.nvec, sc, ep.pw, ep.sub, kc);
        }
        return HK_OK;
    }

    static hk_status scale(hipStream_t s, Fr* data, size_t stride, u32 batch, u32 logn, const Fr* pw,
                           const Fr& sc, int bitrev_index, int use_pow) {
        size_t n = (size_t)1 << logn;
        HK_LAUNCH((k_scale_pow<Fr>), dim3((u32)((n + 255) / 256), batch), dim3(256), 0, s, data,
                  stride, pw, sc, logn, bitrev_index, use_pow);
        return HK_OK;
    }
    static hk_status bitrev(hipStream_t s, Fr* data, u32 logn) {
        size_t n = (size_t)1 << logn;
        HK_LAUNCH((k_bitrev<Fr>), dim3((u32)((n + 255) / 256)), dim3(256), 0, s, data, logn);
        return HK_OK;
    }
};

template <class C>
hk_status Ops<C>::ntt(hk_ctx* ctx, void* data, unsigned log_m, int inverse, int coset) {
    typedef NttHost<C> N;
    NttTables* T;
    HK_TRY(N::ensure(ctx, log_m, &T));
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    size_t n = (size_t)1 << log_m;
    Fr* stage;
    HK_TRY(L->carve([&](Carve& c) { stage = c.n<Fr>(n); }));
    bool dev = is_device_ptr(data);
    Fr* d = (Fr*)data;
    if (!dev) {
        d = stage;
        HK_HIP(hipMemcpyAsync(d, data, n * sizeof(Fr), hipMemcpyHostToDevice, L->stream));
    }
    hipStream_t s = L->stream;
    if (!inverse) {
        // coset FFT: coeff j *= g^j, then FFT (A.2).  DIF then un-permute.
        if (coset) HK_TRY(N::scale(s, d, n, 1, log_m, (const Fr*)T->pw_g, Fr::one(), 0, 1));
        HK_TRY(N::passes(s, d, n, 1, log_m, (const Fr*)T->tw_fwd, 0));
        HK_TRY(N::bitrev(s, d, log_m));
    } else {
        // iFFT: DIF with w^-1, scale by 1/m (and g^-j for the coset form), un-permute
        Fr minv = N::size_inv(log_m);
        typename N::Post ep;
        ep.post = coset ? 3 : 1;
        ep.scale = &minv;
        ep.pw = (const Fr*)T->pw_ginv;
        HK_TRY(N::passes(s, d, n, 1, log_m, (const Fr*)T->tw_inv, 0, ep));
        HK_TRY(N::bitrev(s, d, log_m));
    }
    if (!dev) HK_HIP(hipMemcpyAsync(data, d, n * sizeof(Fr), hipMemcpyDeviceToHost, s));
    return L->settle();
}

// ---- witness map on device buffers --------------------------------------------------------------------
template <class C>
struct QapHost {
    typedef typename C::Fr Fr;
    typedef NttHost<C> N;

    static u32 domain_log(size_t n_c, size_t n_inst) {
        size_t need = n_c + n_inst;
        u32 lg = 0;
        while (((size_t)1 << lg) < need) lg++;
        return lg;
    }
    // abc: 3*m Fr scratch (a | b | c).  On return a[0..m) = h in BIT-REVERSED order.
    static hk_status run(hipStream_t s, NttTables* T, const CsrDev& A, const CsrDev& B, const CsrDev& Cm,
                         size_t n_inst, size_t n_c, const Fr* z, Fr* abc, u32 log_m) {
        size_t m = (size_t)1 << log_m;
        const CsrDev* Ms[3] = {&A, &B, &Cm};
        for (int k = 0; k < 3; k++) {
            // every row of the m-element vector is written: matrix rows, the instance copy behind them (a only:
            // a[n_c + j] = z[j]), zeros - no memset of the 3 m x 32 B (a 201 MB fill at m = 2^21)
            HK_LAUNCH((k_spmv<Fr>), dim3((u32)((m + 255) / 256)), dim3(256), 0, s,
                      Ms[k]->row_ptr, Ms[k]->col, (const Fr*)Ms[k]->val, z, abc + k * m,
                      (u32)n_c, k == 0 ? (u32)n_inst : 0u, (u32)m);
        }
        // With Z constant on the coset (Z(g w^i) = g^m - 1) and the transforms linear,
        //     h = zinv * (coset_ifft(a_coset o b_coset) - ifft(c))
        // which is bit for bit what A.1 computes with its seventh transform (c's coset fft) left out.
        // Every inverse transform here is UNSCALED (m times too large); the powers of 1/m are folded into k, kc.
        const Fr* tinv = (const Fr*)T->tw_inv;
        const Fr* tfwd = (const Fr*)T->tw_fwd;
        typename N::Post e1;                                   // ifft (DIF) of a, b, c; "* g^j" on a and b only
        e1.post = 2;
        e1.nvec = 2;
        e1.pw = (const Fr*)T->pw_g;
        HK_TRY(N::passes(s, abc, m, 3, log_m, tinv, 0, e1));
        HK_TRY(N::passes(s, abc, m, 2, log_m, tfwd, 1));       // coset fft (DIT) of a, b
        HK_LAUNCH((k_mul_pointwise<Fr>), dim3((u32)((m + 255) / 256)), dim3(256), 0, s, abc, abc + m, m);
        Fr minv = N::size_inv(log_m);
        Fr mm = fp_inv(Fr::mul(minv, minv));                                                    // m^2
        Fr k = Fr::mul(N::vanishing_inv_on_coset(log_m), Fr::mul(minv, Fr::mul(minv, minv)));   // zinv / m^3
        typename N::Post e2;                                   // coset ifft (DIF): (x * g^-j - c' * m^2) * zinv/m^3
        e2.post = 2 | 4 | 1;
        e2.pw = (const Fr*)T->pw_ginv;
        e2.sub = abc + 2 * m;
        e2.kc = &mm;
        e2.scale = &k;
        HK_TRY(N::passes(s, abc, m, 1, log_m, tinv, 0, e2));
        return HK_OK;
    }
    // The map for a key whose H query is held in the coset's evaluation basis (h_basis.cuh): four transforms, no C pass.
    // ab: 2*m Fr scratch (a | b).  On return a[j] = m^2 a'_j b'_j, j < m in NATURAL order: the unscaled inverse transform
    // leaves m times the coefficients, the forward transform keeps that factor on each of a' and b', and the key's table
    // G^ / m^2 takes the m^2 back - no scaling product here.  The C part of h is linear in z and rides the L query.
    static hk_status run_eval(hipStream_t s, NttTables* T, const CsrDev& A, const CsrDev& B, size_t n_inst, size_t n_c,
                              const Fr* z, Fr* ab, u32 log_m) {
        size_t m = (size_t)1 << log_m;
        const CsrDev* Ms[2] = {&A, &B};
        for (int k = 0; k < 2; k++)
            HK_LAUNCH((k_spmv<Fr>), dim3((u32)((m + 255) / 256)), dim3(256), 0, s,
                      Ms[k]->row_ptr, Ms[k]->col, (const Fr*)Ms[k]->val, z, ab + k * m,
                      (u32)n_c, k == 0 ? (u32)n_inst : 0u, (u32)m);
        typename N::Post e1;                                   // ifft (DIF) of a, b with "* g^j", as in run()
        e1.post = 2;
        e1.nvec = 2;
        e1.pw = (const Fr*)T->pw_g;
        HK_TRY(N::passes(s, ab, m, 2, log_m, (const Fr*)T->tw_inv, 0, e1));
        HK_TRY(N::passes(s, ab, m, 2, log_m, (const Fr*)T->tw_fwd, 1));       // coset fft (DIT) of a, b
        HK_LAUNCH((k_mul_pointwise<Fr>), dim3((u32)((m + 255) / 256)), dim3(256), 0, s, ab, ab + m, m);
        return HK_OK;
    }
};

template <class C>
hk_status Ops<C>::witness_map(hk_ctx* ctx, const hk_csr* A, const hk_csr* B, const hk_csr* Cm, size_t n_inst,
                              size_t n_c, const void* z, size_t n_v, void* h_out, size_t h_cap,
                              size_t* m_out) {
    typedef QapHost<C> Q;
    if (A->n_rows != n_c || B->n_rows != n_c || Cm->n_rows != n_c || n_inst > n_v || n_inst < 1) return HK_ERR_ARG;
    if (!csr_host_ok(A) || !csr_host_ok(B) || !csr_host_ok(Cm)) return HK_ERR_ARG;
    u32 log_m = Q::domain_log(n_c, n_inst);
    if (log_m > C::TWO_ADICITY) return HK_ERR_DOMAIN_TOO_LARGE;
    size_t m = (size_t)1 << log_m;
    if (m_out) *m_out = m;
    if (h_cap < m) return HK_ERR_LEN;
    NttTables* T;
    HK_TRY(NttHost<C>::ensure(ctx, log_m, &T));
    R1csStage stage(A, B, Cm, n_v, sizeof(Fr));
    Staged zin = staged(z, n_v * sizeof(Fr));
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    Fr* abc;
    HK_TRY(L->carve([&](Carve& c) {
        stage.carve(c);
        stage_carve(c, &zin, 1);
        abc = c.n<Fr>(3 * m);
    }));
    CsrDev D[3];
    HK_TRY(stage.upload(L, D));
    HK_TRY(stage_upload(L, &zin, 1));
    HK_TRY(Q::run(L->stream, T, D[0], D[1], D[2], n_inst, n_c, (const Fr*)zin.p, abc, log_m));
    HK_TRY(NttHost<C>::bitrev(L->stream, abc, log_m));         // API returns natural order
    HK_HIP(hipMemcpyAsync(h_out, abc, m * sizeof(Fr),
                          is_device_ptr(h_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, L->stream));
    return L->settle();
}

template <class C>
void Ops<C>::ctx_release(hk_ctx* ctx) {
    for (auto& e : ctx->fb_cache)
        if (e.table) (void)hipFree(e.table);
    ctx->fb_cache.clear();
    if (!ctx->ntt) return;
    NttTables* T = ctx->ntt;
    for (void* p : {T->tw_fwd, T->tw_inv, T->pw_g, T->pw_ginv})
        if (p) (void)hipFree(p);
    for (void* p : T->retired) (void)hipFree(p);
    delete T;
    ctx->ntt = nullptr;
}

}  // namespace hk
