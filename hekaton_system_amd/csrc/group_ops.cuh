// group_ops.cuh — group operations over caller-supplied points: resident base sets and their MSMs, fixed-base sweeps with
// the context's window-table cache, and the aggregator's element-wise ops (scalar pairing, linear combinations, folds), plus
// field conversion.  Defines Ops<C>::bases_upload / bases_free / msm_bases (hk_bases_*, hk_msm_bases), fixed_base
// (hk_fixed_base_*), scalar_pairing (hk_scalar_pairing_*), points_lincomb (hk_points_lincomb_*), points_fold /
// points_fold_many (hk_points_fold_*), field_convert (hk_field_convert).
#pragma once
#include <string>
#include "curve_ops_impl.cuh"
#include "fixed_base.cuh"

namespace hk {

// ---- MSM over a resident base set (hk_bases_*) -------------------------------------------------------------
struct BasesImpl {
    int group = 1;
    u32 n = 0;
    MsmPlan plan;
    void* tab = nullptr;        // [F][n] Affine<Fq> or Affine<Fq2>; [1][n] when the set never needs its shift tables
    size_t bytes = 0;
    bool has_tables = true;     // false: a short G2 set - every MSM over it runs as MsmRun::small_msm
};

template <class C>
hk_status Ops<C>::bases_upload(hk_ctx* ctx, int group, const void* bases, size_t n, hk_bases** out) {
    *out = nullptr;
    if (n >= ((size_t)1 << MSM_ENTRY_GROUP_SHIFT)) return HK_ERR_ARG;
    HK_HIP(hipSetDevice(ctx->device));
    BasesImpl* b = new BasesImpl();
    b->group = group;
    b->n = (u32)n;
    hk_bases* h = new hk_bases{ctx->ops, ctx, b};
    if (n == 0) { *out = h; return HK_OK; }
    b->plan = msm_make_plan((u32)n, C::FR_BITS, msm_pick_c_tables(n, C::FR_BITS), 1u, ctx->max_lanes0, C::Fr::Params::MOD, C::Fr::Params::N);
    auto build = [&](auto ftag) -> hk_status {
        typedef decltype(ftag) F;
        // a short set goes without shift tables (msm_bases then runs n element-wise endomorphism products + one sum): their
        // construction is 15 x (16 doublings + one inversion) per base - 6 ms per G1 set, 10 ms per G2 set, most of
        // `tipa.setup`, whose four sets are multiplied ONCE per aggregation - against 0.3 - 0.5 ms saved per G1 product
        // (1.0 - 1.3 ms with tables, 1.4 - 1.8 ms without; G2 is quicker without).  HK_BASES_TABLES=1: tables for G1 sets of
        // any length, for a caller that multiplies one set many times
        const bool g2 = sizeof(F) > sizeof(Fq);
        const bool short_set = g2 ? n <= 2048 : (n <= 8192 && !getenv("HK_BASES_TABLES"));
        b->has_tables = !(short_set && !getenv("HK_MSM_NO_SMALL"));
        size_t bytes = (size_t)(b->has_tables ? b->plan.F : 1u) * n * sizeof(Affine<F>);
        if (hipMalloc(&b->tab, bytes) != hipSuccess) { (void)hipGetLastError(); return HK_ERR_NOMEM; }
        b->bytes = bytes;
        HK_HIP(hipMemcpy(b->tab, bases, n * sizeof(Affine<F>), h2d_kind(bases)));
        if (!b->has_tables) return HK_OK;
        return MsmRun<F>::build_tables(0, (Affine<F>*)b->tab, (u32)n, b->plan.F, b->plan.c * b->plan.WP);
    };
    hk_status st = group == 1 ? build(Fq()) : build(Fq2());
    if (st == HK_OK && hipDeviceSynchronize() != hipSuccess) st = HK_ERR_DEVICE;
    if (st != HK_OK) { Ops<C>::bases_free(h); return st; }
    *out = h;
    return HK_OK;
}

template <class C>
void Ops<C>::bases_free(hk_bases* h) {
    if (!h) return;
    BasesImpl* b = (BasesImpl*)h->impl;
    (void)hipSetDevice(h->ctx->device);
    (void)hipDeviceSynchronize();
    if (b->tab) (void)hipFree(b->tab);
    delete b;
    delete h;
}

template <class C>
hk_status Ops<C>::msm_bases(hk_ctx* ctx, const hk_bases* h, const void* scalars, size_t n_scalars, int mont,
                            int checked, void* out) {
    const BasesImpl* b = (const BasesImpl*)h->impl;
    if (checked && n_scalars != b->n) return HK_ERR_LEN;            // ark `msm`: Err(min_len)
    size_t n = n_scalars < b->n ? n_scalars : b->n;                 // ark `msm_unchecked`: zip
    auto run = [&](auto ftag) -> hk_status {
        typedef decltype(ftag) F;
        if (n == 0) { memset(out, 0, sizeof(Affine<F>)); return HK_OK; }
        if (!scalars) return HK_ERR_ARG;
        // a short G2 MSM: even with the tables' bucket pass free of a Horner tail, n element-wise products over psi + one sum
        // are quicker (1.9 - 2.4 ms against 2.3 - 3.0; G1 stays with the tables: 1.0 - 1.2 ms against 1.4 - 1.5)
        const bool small = !b->has_tables || (sizeof(F) > sizeof(Fq) && n <= 2048 && !getenv("HK_MSM_NO_SMALL"));
        Staged in = staged(small ? scalars : nullptr, n * sizeof(Fr));   // the bucket pass copies into a buffer of its own
        LaneGuard g(ctx);
        Lane* L = g.lane;
        if (!L) return HK_ERR_DEVICE;
        OneMsm<F> msm{small, &b->plan, small ? (u32)n : b->n};     // the bucket pass is planned for b->n scalars
        Fr* sc;
        HK_TRY(L->carve([&](Carve& c) { stage_carve(c, &in, 1); sc = c.n<Fr>(small ? 0 : msm.n); msm.carve(c); }));
        hipStream_t s = L->stream;
        HK_TRY(stage_upload(L, &in, 1));
        if (!small) {                                                // the tail reads zeros
            HK_HIP(hipMemcpyAsync(sc, scalars, n * sizeof(Fr), h2d_kind(scalars), s));
            if (n < b->n) HK_HIP(hipMemsetAsync(sc + n, 0, (b->n - n) * sizeof(Fr), s));
        }
        HK_TRY(msm.run(s, (const Affine<F>*)b->tab, small ? in.p : sc, mont, out,    // group 0 of the table = the bases
                       is_device_ptr(out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
        return L->settle();
    };
    return b->group == 1 ? run(Fq()) : run(Fq2());
}

// The window table of a fixed-base call's base, from the context's cache (hk_fixed_base): `base` (host bytes, or nullptr for a
// device base, which is never cached) found there ready -> table, build = false; found while another call builds it, or
// no free slot -> table = nullptr (the call builds into its own scratch); else a new slot is claimed -> table, build = true,
// and publish() after the call's settle marks it ready.  A call that fails after claiming a slot retires it: the entry
// never matches again (its base may claim another).
struct FbCacheUse {
    hk_ctx* c;
    int slot = -1;
    bool done = false;
    void* table = nullptr;
    bool build = true;
    FbCacheUse(hk_ctx* ctx, int group, const void* base, size_t base_bytes, size_t tbytes) : c(ctx) {
        if (!base || getenv("HK_FB_NO_CACHE")) return;
        std::string key((const char*)base, base_bytes);
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (auto& e : ctx->fb_cache)
            if (e.group == group && e.base == key) {
                if (e.ready) { table = e.table; build = false; }
                slot = -2;                                       // present (ready, or being built by another call)
                break;
            }
        if (slot == -1 && ctx->fb_cache.size() < (size_t)hk_ctx::FB_CACHE_MAX) {
            void* t = nullptr;
            if (hipMalloc(&t, tbytes) == hipSuccess) {
                ctx->fb_cache.push_back({group, key, t, false});
                slot = (int)ctx->fb_cache.size() - 1;
                table = t;
            } else {
                (void)hipGetLastError();
            }
        }
    }
    void publish() {
        if (slot >= 0) {
            std::lock_guard<std::mutex> lk(c->mu);
            c->fb_cache[slot].ready = true;
        }
        done = true;
    }
    ~FbCacheUse() {
        if (slot < 0 || done) return;
        std::lock_guard<std::mutex> lk(c->mu);
        c->fb_cache[slot].group = -1;
    }
};

template <class C>
hk_status Ops<C>::fixed_base(hk_ctx* ctx, int group, const void* base, const void* scalars, size_t n, int mont,
                             void* out) {
    if (n == 0) return HK_OK;
    if (n >= (1u << 30)) return HK_ERR_ARG;
    const size_t pt = group == 1 ? g1_bytes : g2_bytes;
    Staged in[2] = {staged(base, pt), staged(scalars, n * sizeof(Fr))}, to = staged(out, n * pt);
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    auto run = [&](auto ftag) -> hk_status {
        typedef decltype(ftag) F;
        Affine<F>* tab_s;
        XYZZ<F>* xy;
        F* pref;
        HK_TRY(L->carve([&](Carve& c) {
            stage_carve(c, in, 2);
            tab_s = c.n<Affine<F>>(FB_WINDOWS * 256);
            xy = c.n<XYZZ<F>>(n);
            pref = c.n<F>(n);
            stage_carve(c, &to, 1);
        }));
        // the base's window table: from the context's cache when this base has been multiplied before (host bases only: the
        // key is the base's bytes), else built now - into a cache slot when one is free, into the lane's scratch otherwise
        const size_t tbytes = sizeof(Affine<F>) * FB_WINDOWS * 256;
        FbCacheUse claimed(ctx, group, in[0].scratch ? base : nullptr, sizeof(Affine<F>), tbytes);
        Affine<F>* table = (Affine<F>*)claimed.table;
        bool build = claimed.build;
        HK_TRY(stage_upload(L, in, 2));
        if (!table) table = tab_s;
        HK_TRY(MsmRun<F>::fixed_base(L->stream, (const Affine<F>*)in[0].p, in[1].p, mont, (u32)n, table, xy, pref,
                                     (Affine<F>*)to.p, build));
        HK_TRY(stage_download(L, &to, 1));
        HK_TRY(L->settle());
        claimed.publish();                                       // the table is complete: later calls may read it
        return HK_OK;
    };
    return group == 1 ? run(Fq()) : run(Fq2());
}

template <class C>
hk_status Ops<C>::scalar_pairing(hk_ctx* ctx, int group, const void* points, const void* scalars, size_t n,
                                 void* out) {
    if (n == 0) return HK_OK;
    if (n >= (1u << 28)) return HK_ERR_ARG;
    const size_t pt = group == 1 ? g1_bytes : g2_bytes;
    Staged in[2] = {staged(points, n * pt), staged(scalars, n * sizeof(Fr))}, to = staged(out, n * pt);
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    auto run = [&](auto ftag) -> hk_status {
        typedef decltype(ftag) F;
        XYZZ<F>*xy, *tab;
        F* pref;
        HK_TRY(L->carve([&](Carve& c) {
            stage_carve(c, in, 2);
            xy = c.n<XYZZ<F>>(n);
            pref = c.n<F>(n);
            tab = (XYZZ<F>*)c.take(endo_tab_bytes<F>(n));            // the chains' tables (endo.cuh)
            stage_carve(c, &to, 1);
        }));
        HK_TRY(stage_upload(L, in, 2));
        HK_TRY(MsmRun<F>::scalar_mul_each(L->stream, (const Affine<F>*)in[0].p, in[1].p, (u32)n, xy, pref, (Affine<F>*)to.p, tab));
        HK_TRY(stage_download(L, &to, 1));
        return L->settle();
    };
    return group == 1 ? run(Fq()) : run(Fq2());
}

template <class C>
hk_status Ops<C>::points_lincomb(hk_ctx* ctx, int group, const void* const* vecs, const void* coeffs, size_t k,
                                 size_t n, void* out) {
    if (n == 0) return HK_OK;
    if (k == 0 || k > (size_t)LINCOMB_MAX || n >= (1u << 28)) return HK_ERR_ARG;
    for (size_t j = 0; j < k; j++) if (!vecs[j]) return HK_ERR_ARG;
    const size_t pt = group == 1 ? g1_bytes : g2_bytes;
    Staged in[LINCOMB_MAX + 1], to = staged(out, n * pt);         // the k vectors, then the coefficients
    for (size_t j = 0; j < k; j++) in[j] = staged(vecs[j], n * pt);
    in[k] = staged(coeffs, k * sizeof(Fr));
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    auto run = [&](auto ftag) -> hk_status {
        typedef decltype(ftag) F;
        const Affine<F>* dv[LINCOMB_MAX];
        XYZZ<F>* xy;
        F* pref;
        HK_TRY(L->carve([&](Carve& c) {
            stage_carve(c, in, k + 1);
            xy = c.n<XYZZ<F>>(n);
            pref = c.n<F>(n);
            stage_carve(c, &to, 1);
        }));
        for (size_t j = 0; j < k; j++) dv[j] = (const Affine<F>*)in[j].p;
        HK_TRY(stage_upload(L, in, k + 1));
        HK_TRY(MsmRun<F>::lincomb(L->stream, dv, in[k].p, (u32)k, (u32)n, xy, pref, (Affine<F>*)to.p));
        HK_TRY(stage_download(L, &to, 1));
        return L->settle();
    };
    return group == 1 ? run(Fq()) : run(Fq2());
}

// device-resident input vectors are packed next to each other by ONE launch (a round of the aggregator's recursion hands
// over twelve windows of its arena: twelve 5 us copies in a row, and their twelve API calls, were 0.1 ms of a 4 ms call)
struct GatherRows {
    enum { MAX = 32 };
    const uint4* src[MAX];
    uint4* dst[MAX];
    u32 vecs[MAX];
};
template <class Tag>
__global__ void k_gather_rows(GatherRows g) {
    u32 r = blockIdx.y;
    const uint4* s = g.src[r];
    uint4* d = g.dst[r];
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < g.vecs[r]; i += gridDim.x * blockDim.x) d[i] = s[i];
}

// out_y[i] = lo_y[i] + c * hi_y[i] for k <= FOLD_MAX vector pairs and ONE scalar c, split by the caller along the group's
// endomorphism into K magnitudes and a sign mask (G2: four ~64-bit parts along psi, G1: two ~128-bit parts along phi): the
// folds of one TIPA round that share a challenge go out as one launch and one normalisation
template <class C>
template <class F>
hk_status Ops<C>::points_fold(hk_ctx* ctx, size_t k, const void* const* lo, const void* const* hi, const void* coeffs,
                              unsigned neg_mask, size_t n, void* const* out) {
    constexpr int K = EndoOf<F>::K;
    if (n == 0 || k == 0) return HK_OK;
    if (!lo || !hi || !coeffs || !out || k > (size_t)FOLD_MAX || n >= (1u << 28) / FOLD_MAX || neg_mask >= (1u << K)) return HK_ERR_ARG;
    for (size_t y = 0; y < k; y++) if (!lo[y] || !hi[y] || !out[y]) return HK_ERR_ARG;
    Staged in[2 * FOLD_MAX];                                        // lo_0, hi_0, lo_1, hi_1, ...
    for (size_t y = 0; y < k; y++) {
        in[2 * y] = staged(lo[y], n * sizeof(Affine<F>));
        in[2 * y + 1] = staged(hi[y], n * sizeof(Affine<F>));
    }
    const bool coeffs_dev = is_device_ptr(coeffs);
    // one vector into a device buffer is normalised in place; otherwise into one array that is then handed out
    const bool direct = k == 1 && is_device_ptr(out[0]);
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    const Affine<F>*lod[FOLD_MAX], *hid[FOLD_MAX];
    Fr* cd;
    XYZZ<F>*tab, *xy;
    F* pref;
    Affine<F>* out_s;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, in, 2 * k);
        cd = c.n<Fr>(K);
        tab = (XYZZ<F>*)c.take(endo_tab_bytes<F>(n, k));
        xy = c.n<XYZZ<F>>(k * n);
        pref = c.n<F>(k * n);
        out_s = c.n<Affine<F>>(direct ? 0 : k * n);
    }));
    for (size_t y = 0; y < k; y++) {
        lod[y] = (const Affine<F>*)in[2 * y].p;
        hid[y] = (const Affine<F>*)in[2 * y + 1].p;
    }
    HK_TRY(stage_upload(L, in, 2 * k));
    HK_HIP(hipMemcpyAsync(cd, coeffs, K * sizeof(Fr), coeffs_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, L->stream));
    // the K-lane form of short vectors reads a magnitude up to 0x77..7 over ND nibbles (endo.cuh); a host caller's longer
    // one goes to the one-lane kernel, which is right for any magnitude.  Device-resident magnitudes are not inspected: the
    // bound is the caller's (include/hekaton.h)
    bool long_mags = false;
    if (!coeffs_dev) {
        HK_HIP(hipStreamSynchronize(L->stream));                              // a pageable caller buffer: done with it now
        for (int j = 0; j < K; j++) {
            Fr m;
            memcpy(&m, (const char*)coeffs + j * sizeof(Fr), sizeof(Fr));
            m = Fr::from_mont(m);
            if (!split_mag_fits<SplitDigits<F>::ND>(m.v)) long_mags = true;
        }
    }
    Affine<F>* od = direct ? (Affine<F>*)out[0] : out_s;
    HK_TRY(MsmRun<F>::fold_endo(L->stream, (u32)k, lod, hid, cd, neg_mask, (u32)n, tab, xy, pref, od, long_mags));
    if (!direct) {
        GatherRows gr;
        bool ok = n * sizeof(Affine<F>) < ((size_t)1 << 32);
        for (size_t y = 0; ok && y < k; y++) {
            ok = ((uintptr_t)out[y] & 15) == 0 && is_device_ptr(out[y]);
            gr.src[y] = (const uint4*)(od + y * n);
            gr.dst[y] = (uint4*)out[y];
            gr.vecs[y] = (u32)(n * sizeof(Affine<F>) / 16);
        }
        if (ok) {                                                   // the folded vectors go to their windows in one launch
            u32 gx = (gr.vecs[0] + 255) / 256;
            HK_LAUNCH((k_gather_rows<Fr>), dim3(gx > 1024 ? 1024 : gx, (u32)k), dim3(256), 0, L->stream, gr);
        } else {
            for (size_t y = 0; y < k; y++)
                HK_HIP(hipMemcpyAsync(out[y], od + y * n, n * sizeof(Affine<F>),
                                      is_device_ptr(out[y]) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, L->stream));
        }
    }
    return L->settle();
}

template <class C>
hk_status Ops<C>::points_fold_many(hk_ctx* ctx, int group, size_t k, const void* const* lo, const void* const* hi,
                                   const void* coeffs, unsigned neg_mask, size_t n, void* const* out) {
    return group == 1 ? points_fold<Fq>(ctx, k, lo, hi, coeffs, neg_mask, n, out)
                      : points_fold<Fq2>(ctx, k, lo, hi, coeffs, neg_mask, n, out);
}

// out[i] = in[i] * R (to_mont) or in[i] / R; memory canonical either way
template <class F>
__global__ void k_field_convert(const F* __restrict__ in, F* __restrict__ out, size_t n, int to_mont) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F x = ld_vec(&in[i]);
    st_vec(&out[i], to_mont ? F::to_mont(x) : F::from_mont(x));
}

template <class C>
hk_status Ops<C>::field_convert(hk_ctx* ctx, int which, const void* in, void* out, size_t n, int to_mont) {
    if (n == 0) return HK_OK;
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    auto run = [&](auto ftag) -> hk_status {
        typedef decltype(ftag) F;
        const size_t CH = (size_t)1 << 24;                       // host buffers go through the lane in chunks
        bool in_dev = is_device_ptr(in), out_dev = is_device_ptr(out);
        for (size_t off = 0; off < n; off += CH) {
            size_t k = std::min(CH, n - off);
            F *t, *u;
            HK_TRY(L->carve([&](Carve& c) { t = c.n<F>(k); u = c.n<F>(k); }));
            const F* src = (const F*)in + off;
            F* dst = (F*)out + off;
            const F* sd = src;
            if (!in_dev) {
                HK_HIP(hipMemcpyAsync(t, src, k * sizeof(F), hipMemcpyHostToDevice, L->stream));
                sd = t;
            }
            F* dd = out_dev ? dst : u;
            HK_LAUNCH(k_field_convert<F>, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, L->stream, sd, dd, k, to_mont);
            if (!out_dev) HK_HIP(hipMemcpyAsync(dst, dd, k * sizeof(F), hipMemcpyDeviceToHost, L->stream));
            HK_TRY(L->settle());
        }
        return HK_OK;
    };
    return which == 0 ? run(Fr()) : run(Fq());
}

}  // namespace hk
