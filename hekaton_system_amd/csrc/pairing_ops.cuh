// pairing_ops.cuh — pairing products and GT powers over caller-supplied vectors (PairRun, msm_driver.cuh).  Defines
// Ops<C>::pairing_products (hk_pairing_products, hk_multi_pairing), pairing_pairs (hk_pairing_pairs), gt_pow (hk_gt_pow,
// hk_gt_pow_prod, hk_fq12_pow) and gt_check (hk_gt_check).
#pragma once
#include "curve_ops_impl.cuh"
#include "group_ops.cuh"      // GatherRows, k_gather_rows

namespace hk {

// ---- multi-pairings (pairing.cuh) ------------------------------------------------------------------------------
template <class C>
hk_status Ops<C>::pairing_products(hk_ctx* ctx, const void* const* lhs, size_t n_lhs, const void* const* rhs,
                                   size_t n_rhs, size_t n, void* out) {
    return pairing_pairs(ctx, lhs, n_lhs, rhs, n_rhs, nullptr, nullptr, 0, n, out);
}

// pair_lhs == nullptr: every (lhs, rhs) pair, out[a * n_rhs + b]; else out[p] for the n_pairs listed pairs
template <class C>
hk_status Ops<C>::pairing_pairs(hk_ctx* ctx, const void* const* lhs, size_t n_lhs, const void* const* rhs, size_t n_rhs,
                                const uint32_t* pair_lhs, const uint32_t* pair_rhs, size_t n_pairs, size_t n, void* out) {
    typedef typename Fq::Params P;
    typedef Fp12<P> GT;
    PairList pl;
    pl.n = 0;
    if (pair_lhs || pair_rhs) {
        if (!pair_lhs || !pair_rhs || n_pairs == 0 || n_pairs > (size_t)PAIR_LIST_MAX || n_lhs > 255 || n_rhs > 255) return HK_ERR_ARG;
        for (size_t k = 0; k < n_pairs; k++) {
            if (pair_lhs[k] >= n_lhs || pair_rhs[k] >= n_rhs) return HK_ERR_ARG;
            pl.a[k] = (unsigned char)pair_lhs[k];
            pl.b[k] = (unsigned char)pair_rhs[k];
        }
        pl.n = (u32)n_pairs;
    }
    size_t count = pl.n ? pl.n : n_lhs * n_rhs;
    if (count == 0 || count > 4096 || n_lhs == 0 || n_rhs == 0 || !out) return HK_ERR_ARG;
    if (n * count >= ((size_t)1 << 31)) return HK_ERR_ARG;
    // the per-step product trees run as grid (groups, count * steps): grid.y is a 16-bit quantity
    if (count * PairRun<P>::steps() > 65535 || n_rhs > 65535) return HK_ERR_ARG;
    if (n == 0) {                                                  // empty product: 1 (final_exponentiation(1) = 1)
        GT one = f12_one<P>();
        HK_HIP(hipSetDevice(ctx->device));
        for (size_t k = 0; k < count; k++)                        // `out` may be a device pointer, as on the n > 0 path
            HK_HIP(hipMemcpy((char*)out + k * sizeof(GT), &one, sizeof(GT), is_device_ptr(out) ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
        return HK_OK;
    }
    for (size_t a = 0; a < n_lhs; a++) if (!lhs[a]) return HK_ERR_ARG;
    for (size_t b = 0; b < n_rhs; b++) if (!rhs[b]) return HK_ERR_ARG;
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    size_t g1b = sizeof(Affine<Fq>), g2b = sizeof(Affine<Fq2>);
    size_t mbytes = PairRun<P>::scratch_bytes((u32)n, (u32)count, (u32)n_rhs);
    Affine<Fq>* d1;
    Affine<Fq2>* d2;
    GT *miller, *prod, *res;
    HK_TRY(L->carve([&](Carve& c) {
        d1 = c.n<Affine<Fq>>(n_lhs * n);
        d2 = c.n<Affine<Fq2>>(n_rhs * n);
        miller = (GT*)c.take(mbytes);                     // lines + per-step tree buffers (or the serial path's Miller values)
        prod = c.n<GT>(count);
        res = c.n<GT>(count);
    }));
    hipStream_t s = L->stream;
    bool packed = false;
    if (n_lhs + n_rhs <= (size_t)GatherRows::MAX && n * g2b < ((size_t)1 << 32)) {
        GatherRows gr;
        u32 most = 0;
        bool ok = true;
        for (size_t k = 0; ok && k < n_lhs + n_rhs; k++) {
            const void* src = k < n_lhs ? lhs[k] : rhs[k - n_lhs];
            ok = ((uintptr_t)src & 15) == 0 && is_device_ptr(src);
            gr.src[k] = (const uint4*)src;
            gr.dst[k] = k < n_lhs ? (uint4*)(d1 + k * n) : (uint4*)(d2 + (k - n_lhs) * n);
            gr.vecs[k] = (u32)(n * (k < n_lhs ? g1b : g2b) / 16);
            if (gr.vecs[k] > most) most = gr.vecs[k];
        }
        if (ok) {
            u32 gx = (most + 255) / 256;
            if (gx > 1024) gx = 1024;
            HK_LAUNCH((k_gather_rows<Fr>), dim3(gx, (u32)(n_lhs + n_rhs)), dim3(256), 0, s, gr);
            packed = true;
        }
    }
    if (!packed) {
        for (size_t a = 0; a < n_lhs; a++) HK_HIP(hipMemcpyAsync(d1 + a * n, lhs[a], n * g1b, h2d_kind(lhs[a]), s));
        for (size_t b = 0; b < n_rhs; b++) HK_HIP(hipMemcpyAsync(d2 + b * n, rhs[b], n * g2b, h2d_kind(rhs[b]), s));
    }
    HK_TRY(PairRun<P>::run(s, d1, d2, (u32)n, (u32)n_lhs, (u32)n_rhs, miller, prod, res, pl.n ? &pl : nullptr));
    HK_HIP(hipMemcpyAsync(out, res, count * sizeof(GT), is_device_ptr(out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    return L->settle();
}

template <class C>
hk_status Ops<C>::gt_pow(hk_ctx* ctx, const void* gt_in, const void* scalars, size_t n, void* gt_out, int in_gt, size_t group_len) {
    typedef typename Fq::Params P;
    typedef Fp12<P> GT;
    if (n == 0) return HK_OK;
    if (n >= (1u << 20)) return HK_ERR_ARG;
    // group_len > 1: out[g] = prod_{j < group_len} in[g * group_len + j]^scalars[...] (a verifier's multi-exponentiations)
    if (group_len == 0 || n % group_len != 0 || n / group_len > 65535) return HK_ERR_ARG;
    size_t n_out = n / group_len;
    Staged in[2] = {staged(gt_in, n * sizeof(GT)), staged(scalars, n * sizeof(Fr))}, to = staged(gt_out, n_out * sizeof(GT));
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    GT* pw;                                                        // the n powers: the output itself when group_len == 1
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, in, 2);
        pw = c.n<GT>(group_len > 1 ? n : 0);
        stage_carve(c, &to, 1);
    }));
    if (group_len == 1) pw = (GT*)to.p;
    HK_TRY(stage_upload(L, in, 2));
    HK_TRY(PairRun<P>::gt_pow(L->stream, (const GT*)in[0].p, in[1].p, (u32)n, pw, in_gt != 0));
    if (group_len > 1) HK_TRY(PairRun<P>::gt_prod(L->stream, pw, (u32)group_len, (u32)n_out, (GT*)to.p));
    HK_TRY(stage_download(L, &to, 1));
    return L->settle();
}

// hk_gt_check: ok[i] = 1 iff fq12_in[i] is an element of GT (k_gt_check, one wavefront per element)
template <class C>
hk_status Ops<C>::gt_check(hk_ctx* ctx, const void* fq12_in, size_t n, unsigned char* ok) {
    typedef typename Fq::Params P;
    typedef Fp12<P> GT;
    if (n == 0) return HK_OK;
    if (n >= ((size_t)1 << 31)) return HK_ERR_ARG;                 // one workgroup per element: grid.x
    Staged io[2] = {staged(fq12_in, n * sizeof(GT)), staged(ok, n)};
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    HK_TRY(L->carve([&](Carve& c) { stage_carve(c, io, 2); }));
    HK_TRY(stage_upload(L, io, 1));
    HK_TRY(PairRun<P>::gt_check(L->stream, (const GT*)io[0].p, (u32)n, (unsigned char*)io[1].p));
    HK_TRY(stage_download(L, io + 1, 1));
    return L->settle();
}

}  // namespace hk
