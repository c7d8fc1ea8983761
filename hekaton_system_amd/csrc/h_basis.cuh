// h_basis.cuh — the one-time work of a proving key that holds its H query in the coset's evaluation basis (pk.cuh,
// DESIGN.md section 4t).  With h = u - v, u the interpolant of zinv a'_j b'_j on the coset and v = zinv C(X):
//     sum_i h_i H_i = sum_j (a'_j b'_j) G^_j - sum_k z_k C^_k,
//     G^_j = (zinv / m) sum_i g^-i w^-ij H_i,   G_j = (zinv / m) sum_i w^-ij H_i,   C^_k = sum_row C[row, k] G_row,
// with H_{m-1} = O, so the dropped coefficient h_{m-1} stays dropped.  Both vectors are the same inverse DFT of group
// elements (HBasis::transform); C^ = C^T G needs the transpose of the class's C matrix (HBasis::c_columns).  The prover
// then multiplies the pointwise product of the two coset transforms - m^2 times too large, their inverse transforms being
// unscaled (QapHost::run_eval) - against G^ / m^2, and the assignment against tables that carry -C^.  Only the key's
// public points enter; nothing here runs per proof.
#pragma once
#include "ntt_host.cuh"
#include "csr.cuh"
#include "endo.cuh"
#include "h_basis_plan.h"

namespace hk {

// s * P over the curve's endomorphism: s = k_0 + k_1 lambda (endo_decompose), one chain of EndoOf::STEPS doublings that
// adds +-P, +-phi(P) or their sum.  Leading zero columns cost nothing, so a matrix coefficient of +-1 is two additions.
template <class Fr, class F>
__device__ XYZZ<F> hb_mul(const XYZZ<F>& p, const Fr& s_mont, const EndoSplit<2>& E) {
    XYZZ<F> acc = XYZZ<F>::inf();
    if (p.is_inf()) return acc;
    Fr k = Fr::from_mont(s_mont);
    u32 c[8], mag[2][6];
    HK_UNROLL for (int l = 0; l < 8; l++) c[l] = l < Fr::N ? k.v[l] : 0u;
    u32 neg = endo_decompose<2>(c, E, mag);
    XYZZ<F> t[3];                                                   // +-P, +-phi(P), their sum
    Affine<F> q;
    q.x = p.x; q.y = p.y;
    t[0] = p;
    t[1] = p;
    t[1].x = EndoOf<F>::apply(q).x;
    if (neg & 1u) t[0].y = F::neg(p.y);
    if (neg & 2u) t[1].y = F::neg(p.y);
    t[2] = ec_add_ni(t[0], t[1]);
    HK_NOUNROLL for (int b = EndoOf<F>::STEPS - 1; b >= 0; b--) {
        u32 m = ((mag[0][b >> 5] >> (b & 31)) & 1u) | (((mag[1][b >> 5] >> (b & 31)) & 1u) << 1);
        if (m == 0 && acc.is_inf()) continue;
        acc = ec_dbl_ni(acc);
        if (m) acc = ec_add_ni(acc, t[m - 1]);
    }
    return acc;
}

// x[v m + bitrev(i)] = s_vi * H_i for the two input vectors of the transform: s_0i = c0 g^-i, s_1i = c1; H_i = O from
// h_len on.  grid (ceil(m / 64), 2).
template <class Fr, class F>
__global__ void __launch_bounds__(64)
k_hb_load(const Affine<F>* __restrict__ h_g, u32 h_len, u32 log_m, const Fr* __restrict__ pw_ginv, Fr c0, Fr c1,
          EndoSplit<2> E, XYZZ<F>* __restrict__ x) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >> log_m) return;
    const u32 v = blockIdx.y;
    u32 r = log_m ? (__brev(i) >> (32 - log_m)) : 0u;
    XYZZ<F> o = XYZZ<F>::inf();
    if (i < h_len) {
        Fr s = v ? c1 : Fr::mul(c0, pow_from_tables(pw_ginv, i, log_m));
        o = hb_mul(XYZZ<F>::from_affine(ld_vec(&h_g[i])), s, E);
    }
    st_vec(&x[((size_t)v << log_m) + r], o);
}

// stage s (span 2^s) of the decimation-in-time transform over w^-1, in place: (U, V) -> (U + w V, U - w V), one lane per
// butterfly, w from the per-stage twiddle tables (k_stage_tables); a unit twiddle takes no product.  grid (ceil(m / 128), 2).
template <class Fr, class F>
__global__ void __launch_bounds__(64)
k_hb_stage(XYZZ<F>* __restrict__ x, const Fr* __restrict__ tws, u32 s, u32 log_m, EndoSplit<2> E) {
    u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >> (log_m - 1)) return;
    XYZZ<F>* vec = x + ((size_t)blockIdx.y << log_m);
    const u32 half = 1u << s, pos = t & (half - 1u);
    const size_t i0 = ((size_t)(t >> s) << (s + 1)) | pos, i1 = i0 + half;
    XYZZ<F> u = ld_vec(&vec[i0]), w = ld_vec(&vec[i1]);
    if (pos) w = hb_mul(w, fr_load(&tws[(half - 1u) + pos]), E);
    st_vec(&vec[i0], ec_add_ni(u, w));
    st_vec(&vec[i1], ec_add_ni(u, ec_neg(w)));
}

// out[k] = -C^_k (+ ck_last[k - first_last] for the last stage's witnesses), one lane per variable k < n_v:
// C^_k = sum over the column's entries of val * G_row, or heavy[hv[k] - 1] where the column went through the bases MSM.
template <class Fr, class F>
__global__ void __launch_bounds__(64)
k_hb_ccols(const u64* __restrict__ col_ptr, const u32* __restrict__ row, const u32* __restrict__ src,
           const Fr* __restrict__ val, const Affine<F>* __restrict__ g, const u32* __restrict__ hv,
           const Affine<F>* __restrict__ heavy, const Affine<F>* __restrict__ ck_last, u32 first_last, u32 n_v,
           EndoSplit<2> E, XYZZ<F>* __restrict__ out) {
    u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_v) return;
    XYZZ<F> acc = XYZZ<F>::inf();
    if (hv[k]) {
        acc = XYZZ<F>::from_affine(ld_vec(&heavy[hv[k] - 1]));
    } else {
        HK_NOUNROLL for (u64 e = col_ptr[k]; e < col_ptr[k + 1]; e++)
            acc = ec_add_ni(acc, hb_mul(XYZZ<F>::from_affine(ld_vec(&g[row[e]])), fr_load(&val[src[e]]), E));
    }
    acc = ec_neg(acc);
    if (k >= first_last) acc = ec_madd_ni(acc, ld_vec(&ck_last[k - first_last]));
    st_vec(&out[k], acc);
}

template <class C>
struct HBasis {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef NttHost<C> N;

    // hat[j] = G^_j / m^2 and g[j] = G_j, j < m, natural order (device, m affine points each) from the key's h_g (device,
    // h_len = m - 1 points)
    static hk_status transform(hk_ctx* ctx, NttTables* T, const Affine<Fq>* h_g, u32 h_len, u32 log_m, Affine<Fq>* hat,
                               Affine<Fq>* g) {
        const size_t m = (size_t)1 << log_m;
        LaneGuard lg(ctx);
        Lane* L = lg.lane;
        if (!L) return HK_ERR_DEVICE;
        XYZZ<Fq>* x;
        Fq* pref;
        HK_TRY(L->carve([&](Carve& c) { x = c.n<XYZZ<Fq>>(2 * m); pref = c.n<Fq>(2 * m); }));
        hipStream_t s = L->stream;
        static const EndoSplit<2> E = EndoOf<Fq>::split();
        // QapHost::run_eval hands the H MSM m^2 a'_j b'_j (both of its inverse transforms are unscaled), the C part reads
        // the rows c_j as they are: zinv / m^3 on the first vector, zinv / m on the second
        Fr minv = N::size_inv(log_m), zinv = N::vanishing_inv_on_coset(log_m);
        Fr c1 = Fr::mul(zinv, minv), c0 = Fr::mul(c1, Fr::mul(minv, minv));
        HK_LAUNCH((k_hb_load<Fr, Fq>), dim3((u32)((m + 63) / 64), 2), dim3(64), 0, s, h_g, h_len, log_m,
                  (const Fr*)T->pw_ginv, c0, c1, E, x);
        for (u32 st = 0; st < log_m; st++)
            HK_LAUNCH((k_hb_stage<Fr, Fq>), dim3((u32)((m / 2 + 63) / 64), 2), dim3(64), 0, s, x, (const Fr*)T->tw_inv,
                      st, log_m, E);
        HK_TRY(MsmRun<Fq>::batch_affine(s, x, hat, pref, (u32)m));
        HK_TRY(MsmRun<Fq>::batch_affine(s, x + m, g, pref + m, (u32)m));
        return L->settle();
    }

    // out[k] = -C^_k, plus ck_last[k - (n_v - n1)] for the n1 last-stage witnesses, k < n_v (device, affine).  Cm: the key's
    // validated C matrix on the device; g: G (device, m points); ck_last: host or device.
    static hk_status c_columns(hk_ctx* ctx, const CsrDev& Cm, size_t n_v, u32 log_m, const Affine<Fq>* g, const void* ck_last,
                               size_t n1, Affine<Fq>* out) {
        const size_t m = (size_t)1 << log_m, nnz = Cm.nnz;
        std::vector<u64> rp(Cm.n_rows + 1), col_ptr;
        std::vector<u32> cl(nnz), row, src;
        HK_HIP(hipMemcpy(rp.data(), Cm.row_ptr, 8 * rp.size(), hipMemcpyDeviceToHost));
        if (nnz) HK_HIP(hipMemcpy(cl.data(), Cm.col, 4 * nnz, hipMemcpyDeviceToHost));
        if (Cm.n_rows > m || !hb_transpose(rp.data(), cl.data(), Cm.n_rows, n_v, col_ptr, row, src)) return HK_ERR_ARG;
        // heavy columns: one MSM each over the bases G, the column as a dense scalar vector (equal rows summed)
        const u32 thr = hb_heavy_threshold(getenv("HK_H_BASIS_HEAVY_COL"));
        std::vector<u32> hv(n_v, 0);
        std::vector<Affine<Fq>> heavy;
        for (size_t k = 0; k < n_v; k++)
            if (hb_col_is_heavy(col_ptr[k + 1] - col_ptr[k], thr)) hv[k] = 1;
        if (std::find(hv.begin(), hv.end(), 1u) != hv.end()) {
            std::vector<Fr> vals(nnz), dense(m, Fr::zero());
            HK_HIP(hipMemcpy(vals.data(), Cm.val, sizeof(Fr) * nnz, hipMemcpyDeviceToHost));
            hk_bases* bh = nullptr;
            HK_TRY(ctx->ops->bases_upload(ctx, 1, g, m, &bh));
            hk_status st = HK_OK;
            for (size_t k = 0; k < n_v && st == HK_OK; k++) {
                if (!hv[k]) continue;
                for (u64 e = col_ptr[k]; e < col_ptr[k + 1]; e++) dense[row[e]] = Fr::add(dense[row[e]], vals[src[e]]);
                Affine<Fq> pt;
                st = ctx->ops->msm_bases(ctx, bh, dense.data(), m, 1, 1, &pt);
                for (u64 e = col_ptr[k]; e < col_ptr[k + 1]; e++) dense[row[e]] = Fr::zero();
                heavy.push_back(pt);
                hv[k] = (u32)heavy.size();
            }
            ctx->ops->bases_free(bh);
            HK_TRY(st);
        }
        Staged in[6] = {staged(col_ptr.data(), 8 * col_ptr.size()), staged(row.data(), 4 * nnz), staged(src.data(), 4 * nnz),
                        staged(hv.data(), 4 * n_v), staged(heavy.data(), sizeof(Affine<Fq>) * heavy.size()),
                        staged(n1 ? ck_last : nullptr, sizeof(Affine<Fq>) * n1)};
        LaneGuard lg(ctx);
        Lane* L = lg.lane;
        if (!L) return HK_ERR_DEVICE;
        XYZZ<Fq>* xy;
        Fq* pref;
        HK_TRY(L->carve([&](Carve& c) { stage_carve(c, in, 6); xy = c.n<XYZZ<Fq>>(n_v); pref = c.n<Fq>(n_v); }));
        HK_TRY(stage_upload(L, in, 6));
        static const EndoSplit<2> E = EndoOf<Fq>::split();
        HK_LAUNCH((k_hb_ccols<Fr, Fq>), dim3((u32)((n_v + 63) / 64)), dim3(64), 0, L->stream, (const u64*)in[0].p,
                  (const u32*)in[1].p, (const u32*)in[2].p, (const Fr*)Cm.val, g, (const u32*)in[3].p,
                  (const Affine<Fq>*)in[4].p, (const Affine<Fq>*)in[5].p, (u32)(n_v - n1), (u32)n_v, E, xy);
        HK_TRY(MsmRun<Fq>::batch_affine(L->stream, xy, out, pref, (u32)n_v));
        return L->settle();
    }
};

}  // namespace hk
