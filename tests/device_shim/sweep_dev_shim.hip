// Device-compiled view of the PRODUCT's group sweeps over caller-supplied points, ONE kernel launch per call (hipcc, gfx950):
// k_fb_table, k_fb_mul, k_points_lincomb, k_scalar_mul_each (fixed_base.cuh), k_scalar_mul_endo, k_points_fold_endo,
// k_points_mul_split in every form, k_points_sum_seg at both sizes (endo.cuh).  Through the library these kernels are
// reached only behind MsmRun's choices (the form by n, the window table from the base, the normalisation behind each); here a
// test hands a kernel the table, the vectors, the form and the launch shape it wants and reads back what the kernel stored.
// Test-only; never part of libhekaton.
//
// One translation unit per group (-DSHIM_GROUP=0..3: the ladder of shim_common.cuh, as ec_dev_shim.hip), linked into one
// library; group 0's unit also holds the extern "C" entry points.  Built as shipped only
// (see the header of the Makefile next to it).  The kernels keep their product names: the library is linked -Bsymbolic and
// loaded RTLD_LOCAL, as the other shims are.
//
// Operands and results are the bytes the kernels read and write: affine points and Fr scalars in memory form, XYZZ results
// as stored (x, y, zz, zzz; zz = 0: infinity).  Every HIP status is returned to the caller; the shim allocates and frees its
// own buffers (scratch and outputs start as 0xA5) and never touches an hk_ctx.
#include "../../hekaton_system_amd/csrc/msm_driver_impl.cuh"
#ifndef SHIM_GROUP
#error "compile with -DSHIM_GROUP=0..3"
#endif
#define SHIM_PREFIX sweep_shim
#include "shim_common.cuh"

namespace {

constexpr size_t SWEEP_MAX_N = 1u << 16;

template <class F> struct QuadOf { typedef F type; static constexpr bool has = false; };
template <class P> struct QuadOf<Fp2<P>> { typedef Fp2Q<P> type; static constexpr bool has = true; };

template <class F>
int fb_table(const void* base, void* table_out) {
    DevBufs d;
    const size_t tb = sizeof(Affine<F>) * FB_WINDOWS * 256;
    const Affine<F>* b;
    Affine<F>* t;
    SHIM_GET(&b, sizeof(Affine<F>), base);
    SHIM_GET(&t, tb, nullptr);
    hipLaunchKernelGGL((k_fb_table<F>), dim3(FB_WINDOWS * 256 / 64), dim3(64), 0, 0, b, t);
    return finish(table_out, t, tb);
}

template <class Fr, class F>
int fb_mul(const void* table, const void* scalars, int is_mont, unsigned n, void* out) {
    DevBufs d;
    const Affine<F>* t;
    const Fr* s;
    XYZZ<F>* o;
    SHIM_GET(&t, sizeof(Affine<F>) * FB_WINDOWS * 256, table);
    SHIM_GET(&s, (size_t)n * sizeof(Fr), scalars);
    SHIM_GET(&o, (size_t)n * sizeof(XYZZ<F>), nullptr);
    hipLaunchKernelGGL((k_fb_mul<Fr, F>), dim3((n + 63) / 64), dim3(64), 0, 0, t, s, is_mont, n, o);
    return finish(out, o, (size_t)n * sizeof(XYZZ<F>));
}

template <class Fr, class F>
int lincomb(const void* vecs, const void* coeffs, unsigned k, unsigned n, void* out) {
    DevBufs d;
    const Affine<F>* v;
    const Fr* c;
    XYZZ<F>* o;
    SHIM_GET(&v, (size_t)k * n * sizeof(Affine<F>), vecs);
    SHIM_GET(&c, (size_t)k * sizeof(Fr), coeffs);
    SHIM_GET(&o, (size_t)n * sizeof(XYZZ<F>), nullptr);
    LincombVecs<F> lv;
    for (unsigned j = 0; j < (unsigned)LINCOMB_MAX; j++) lv.v[j] = j < k ? v + (size_t)j * n : nullptr;
    hipLaunchKernelGGL((k_points_lincomb<Fr, F>), dim3((n + 63) / 64), dim3(64), 0, 0, lv, c, k, n, o);
    return finish(out, o, (size_t)n * sizeof(XYZZ<F>));
}

// kind 0: k_scalar_mul_each (the plain ladder), 1: k_scalar_mul_endo
template <class Fr, class F>
int mul_each(int kind, const void* pts, const void* scalars, unsigned n, void* out) {
    DevBufs d;
    const Affine<F>* p;
    const Fr* s;
    XYZZ<F>* o;
    SHIM_GET(&p, (size_t)n * sizeof(Affine<F>), pts);
    SHIM_GET(&s, (size_t)n * sizeof(Fr), scalars);
    SHIM_GET(&o, (size_t)n * sizeof(XYZZ<F>), nullptr);
    if (kind == 0) {
        hipLaunchKernelGGL((k_scalar_mul_each<Fr, F>), dim3((n + 63) / 64), dim3(64), 0, 0, p, s, n, o);
    } else {
        XYZZ<F>* tab;
        SHIM_GET(&tab, ((size_t)1 << EndoOf<F>::K) * n * sizeof(XYZZ<F>), nullptr);
        hipLaunchKernelGGL((k_scalar_mul_endo<Fr, F>), dim3((n + 63) / 64), dim3(64), 0, 0, p, s, n, EndoOf<F>::split(), tab, o);
    }
    return finish(out, o, (size_t)n * sizeof(XYZZ<F>));
}

template <class Fr, class F>
int fold_endo(const void* lo, const void* hi, const void* coeffs, unsigned neg, unsigned n, void* out) {
    DevBufs d;
    const Affine<F> *l, *h;
    const Fr* c;
    XYZZ<F> *tab, *o;
    SHIM_GET(&l, (size_t)n * sizeof(Affine<F>), lo);
    SHIM_GET(&h, (size_t)n * sizeof(Affine<F>), hi);
    SHIM_GET(&c, (size_t)EndoOf<F>::K * sizeof(Fr), coeffs);
    SHIM_GET(&tab, ((size_t)1 << EndoOf<F>::K) * n * sizeof(XYZZ<F>), nullptr);
    SHIM_GET(&o, (size_t)n * sizeof(XYZZ<F>), nullptr);
    hipLaunchKernelGGL((k_points_fold_endo<Fr, F>), dim3((n + 63) / 64), dim3(64), 0, 0, l, h, c, neg, n, tab, o);
    return finish(out, o, (size_t)n * sizeof(XYZZ<F>));
}

// FK: the field type the kernel is instantiated with (F, or its quad form: same memory layout)
template <class Fr, class F, class FK, bool UNIFORM>
void launch_split(const Affine<F>* lo, const Affine<F>* pts, unsigned n_pts, const Fr* scalars, unsigned neg_all, unsigned n,
                  unsigned pts_mod, unsigned vectors, int scalars_mont, void* tab, XYZZ<F>* out) {
    constexpr unsigned per_wg = 64 / (LanesPerValue<FK>::value * EndoOf<FK>::K);
    SplitVecs<FK> v = {};
    for (unsigned y = 0; y < vectors; y++) {
        v.lo[y] = lo ? (const Affine<FK>*)(lo + (size_t)y * n) : nullptr;
        v.pts[y] = (const Affine<FK>*)(pts + (size_t)y * n_pts);
    }
    v.pts_mod = pts_mod;
    hipLaunchKernelGGL((k_points_mul_split<Fr, FK, UNIFORM>), dim3((n + per_wg - 1) / per_wg, vectors), dim3(64), 0, 0, v, scalars,
                       neg_all, n, EndoOf<F>::split(), (Jac<FK>*)tab, (XYZZ<FK>*)out, scalars_mont);
}

// lo: vectors x n affine points or null; pts: vectors x (pts_mod ? pts_mod : n); scalars: K magnitudes (uniform) or n Fr;
// out: vectors x n XYZZ
template <class Fr, class F>
int mul_split(int quad, int uniform, const void* lo, const void* pts, const void* scalars, unsigned neg_all, unsigned n,
              unsigned pts_mod, unsigned vectors, int scalars_mont, void* out) {
    typedef typename QuadOf<F>::type Q;
    if (quad && !QuadOf<F>::has) return -(int)hipErrorNotSupported;
    DevBufs d;
    const unsigned n_pts = pts_mod ? pts_mod : n;
    const Affine<F> *l = nullptr, *p;
    const Fr* s;
    void* tab;
    XYZZ<F>* o;
    if (lo) SHIM_GET(&l, (size_t)vectors * n * sizeof(Affine<F>), lo);
    SHIM_GET(&p, (size_t)vectors * n_pts * sizeof(Affine<F>), pts);
    SHIM_GET(&s, (size_t)(uniform ? (unsigned)EndoOf<F>::K : n) * sizeof(Fr), scalars);
    SHIM_GET(&tab, (size_t)vectors * split_tab_bytes<F>(n), nullptr);
    SHIM_GET(&o, (size_t)vectors * n * sizeof(XYZZ<F>), nullptr);
    if (quad && uniform) launch_split<Fr, F, Q, true>(l, p, n_pts, s, neg_all, n, pts_mod, vectors, scalars_mont, tab, o);
    else if (quad) launch_split<Fr, F, Q, false>(l, p, n_pts, s, neg_all, n, pts_mod, vectors, scalars_mont, tab, o);
    else if (uniform) launch_split<Fr, F, F, true>(l, p, n_pts, s, neg_all, n, pts_mod, vectors, scalars_mont, tab, o);
    else launch_split<Fr, F, F, false>(l, p, n_pts, s, neg_all, n, pts_mod, vectors, scalars_mont, tab, o);
    return finish(out, o, (size_t)vectors * n * sizeof(XYZZ<F>));
}

template <class F, int T>
int points_sum_seg(const void* in, unsigned seg, unsigned batch, void* out) {
    DevBufs d;
    const XYZZ<F>* i;
    XYZZ<F>* o;
    SHIM_GET(&i, (size_t)seg * batch * sizeof(XYZZ<F>), in);
    SHIM_GET(&o, (size_t)batch * sizeof(XYZZ<F>), nullptr);
    hipLaunchKernelGGL((k_points_sum_seg<F, T>), dim3(batch), dim3(T), 0, 0, i, seg, o);
    return finish(out, o, (size_t)batch * sizeof(XYZZ<F>));
}

}  // namespace

// ---- per-group entry points (C++ linkage inside the library) ---------------------------------------------------------
int SHIM_FN(fb_table)(const void* base, void* table_out) { return fb_table<ShimF>(base, table_out); }
int SHIM_FN(fb_mul)(const void* table, const void* scalars, int is_mont, unsigned n, void* out) {
    return fb_mul<ShimFr, ShimF>(table, scalars, is_mont, n, out);
}
int SHIM_FN(lincomb)(const void* vecs, const void* coeffs, unsigned k, unsigned n, void* out) {
    return lincomb<ShimFr, ShimF>(vecs, coeffs, k, n, out);
}
int SHIM_FN(mul_each)(int kind, const void* pts, const void* scalars, unsigned n, void* out) {
    return mul_each<ShimFr, ShimF>(kind, pts, scalars, n, out);
}
int SHIM_FN(fold_endo)(const void* lo, const void* hi, const void* coeffs, unsigned neg, unsigned n, void* out) {
    return fold_endo<ShimFr, ShimF>(lo, hi, coeffs, neg, n, out);
}
int SHIM_FN(mul_split)(int quad, int uniform, const void* lo, const void* pts, const void* scalars, unsigned neg_all, unsigned n,
                       unsigned pts_mod, unsigned vectors, int scalars_mont, void* out) {
    return mul_split<ShimFr, ShimF>(quad, uniform, lo, pts, scalars, neg_all, n, pts_mod, vectors, scalars_mont, out);
}
int SHIM_FN(points_sum)(const void* in, unsigned n, void* out) { return points_sum_seg<ShimF, PointsSum<ShimF>::THREADS>(in, n, 1, out); }
int SHIM_FN(points_sum_seg)(const void* in, unsigned seg, unsigned batch, void* out) { return points_sum_seg<ShimF, 64>(in, seg, batch, out); }
int SHIM_FN(sum_threads)() { return PointsSum<ShimF>::THREADS; }
int SHIM_FN(split_elems)(int quad) {
    if (quad) return QuadOf<ShimF>::has ? 64 / (4 * EndoOf<ShimF>::K) : 0;
    return 64 / EndoOf<ShimF>::K;
}
int SHIM_FN(split_nd)() { return SplitDigits<ShimF>::ND; }
int SHIM_FN(split_steps)() { return EndoOf<ShimF>::STEPS; }

#if SHIM_GROUP == 0
#define SHIM_DECL(g)                                                                                                        \
    int sweep_shim_g##g##_fb_table(const void*, void*);                                                                    \
    int sweep_shim_g##g##_fb_mul(const void*, const void*, int, unsigned, void*);                                          \
    int sweep_shim_g##g##_lincomb(const void*, const void*, unsigned, unsigned, void*);                                    \
    int sweep_shim_g##g##_mul_each(int, const void*, const void*, unsigned, void*);                                        \
    int sweep_shim_g##g##_fold_endo(const void*, const void*, const void*, unsigned, unsigned, void*);                     \
    int sweep_shim_g##g##_mul_split(int, int, const void*, const void*, const void*, unsigned, unsigned, unsigned, unsigned, \
                                    int, void*);                                                                           \
    int sweep_shim_g##g##_points_sum(const void*, unsigned, void*);                                                        \
    int sweep_shim_g##g##_points_sum_seg(const void*, unsigned, unsigned, void*);                                          \
    int sweep_shim_g##g##_sum_threads();                                                                                   \
    int sweep_shim_g##g##_split_elems(int);                                                                                \
    int sweep_shim_g##g##_split_nd();                                                                                      \
    int sweep_shim_g##g##_split_steps();
SHIM_DECL(1) SHIM_DECL(2) SHIM_DECL(3)

static bool n_ok(unsigned n) { return n != 0 && n <= SWEEP_MAX_N; }

extern "C" {
// group: 0 bn254 G1, 1 bn254 G2, 2 bls G1, 3 bls G2 throughout.  Every call returns 0 or minus the first failing hipError_t
// (hipErrorInvalidValue for arguments outside a kernel's contract: nothing is launched then).
// PointsSum<F>::THREADS: the workgroup of k_points_sum_seg over one segment (the small MSM's sum)
int dshim_sweep_sum_threads(int group) { SHIM_DISPATCH(group, sum_threads()) }
// elements per 64-lane workgroup of k_points_mul_split: quad = 0 the K-lane form, 1 the quad form (0 for a G1 group)
int dshim_sweep_split_elems(int group, int quad) { SHIM_DISPATCH(group, split_elems(quad)) }
// SplitDigits<F>::ND and EndoOf<F>::STEPS
int dshim_sweep_split_nd(int group) { SHIM_DISPATCH(group, split_nd()) }
int dshim_sweep_split_steps(int group) { SHIM_DISPATCH(group, split_steps()) }
// base: one affine point -> table_out: 32 x 256 affine points
int dshim_fb_table(int group, const void* base, void* table_out) {
    if (!base || !table_out) return -(int)hipErrorInvalidValue;
    SHIM_DISPATCH(group, fb_table(base, table_out))
}
// table: 32 x 256 affine points (the caller's, not necessarily a window table); scalars: n Fr -> out: n XYZZ
int dshim_fb_mul(int group, const void* table, const void* scalars, int is_mont, unsigned n, void* out) {
    if (!table || !scalars || !out || !n_ok(n)) return -(int)hipErrorInvalidValue;
    SHIM_DISPATCH(group, fb_mul(table, scalars, is_mont, n, out))
}
// vecs: k x n affine points, vector j at j * n; coeffs: k Fr (Montgomery) -> out: n XYZZ
int dshim_points_lincomb(int group, const void* vecs, const void* coeffs, unsigned k, unsigned n, void* out) {
    if (!vecs || !coeffs || !out || !n_ok(n) || k == 0 || k > (unsigned)LINCOMB_MAX) return -(int)hipErrorInvalidValue;
    SHIM_DISPATCH(group, lincomb(vecs, coeffs, k, n, out))
}
// kind 0: k_scalar_mul_each, 1: k_scalar_mul_endo; pts: n affine; scalars: n Fr (Montgomery) -> out: n XYZZ
int dshim_scalar_mul(int group, int kind, const void* pts, const void* scalars, unsigned n, void* out) {
    if (!pts || !scalars || !out || !n_ok(n) || kind < 0 || kind > 1) return -(int)hipErrorInvalidValue;
    SHIM_DISPATCH(group, mul_each(kind, pts, scalars, n, out))
}
// k_points_fold_endo: lo, hi: n affine; coeffs: K Fr magnitudes (Montgomery); neg: their sign mask -> out: n XYZZ
int dshim_points_fold_endo(int group, const void* lo, const void* hi, const void* coeffs, unsigned neg, unsigned n, void* out) {
    if (!lo || !hi || !coeffs || !out || !n_ok(n) || neg >= 16u) return -(int)hipErrorInvalidValue;
    SHIM_DISPATCH(group, fold_endo(lo, hi, coeffs, neg, n, out))
}
// k_points_mul_split: quad = 1 the quad-lane form (G2 groups only: hipErrorNotSupported otherwise); uniform = 1: scalars = K
// magnitudes (Montgomery) + neg_all, else n Fr (Montgomery when scalars_mont); lo: vectors x n affine or null; pts: vectors x
// (pts_mod ? pts_mod : n) affine; out: vectors x n XYZZ
int dshim_points_mul_split(int group, int quad, int uniform, const void* lo, const void* pts, const void* scalars,
                           unsigned neg_all, unsigned n, unsigned pts_mod, unsigned vectors, int scalars_mont, void* out) {
    if (!pts || !scalars || !out || !n_ok(n) || vectors == 0 || vectors > (unsigned)FOLD_MAX || pts_mod > n || neg_all >= 16u)
        return -(int)hipErrorInvalidValue;
    SHIM_DISPATCH(group, mul_split(quad, uniform, lo, pts, scalars, neg_all, n, pts_mod, vectors, scalars_mont, out))
}
// in: n XYZZ -> out: 1 XYZZ
int dshim_points_sum(int group, const void* in, unsigned n, void* out) {
    if (!in || !out || !n_ok(n)) return -(int)hipErrorInvalidValue;
    SHIM_DISPATCH(group, points_sum(in, n, out))
}
// in: batch x seg XYZZ -> out: batch XYZZ
int dshim_points_sum_seg(int group, const void* in, unsigned seg, unsigned batch, void* out) {
    if (!in || !out || !n_ok(seg) || batch == 0 || batch > 1024u || (size_t)seg * batch > SWEEP_MAX_N) return -(int)hipErrorInvalidValue;
    SHIM_DISPATCH(group, points_sum_seg(in, seg, batch, out))
}
}
#endif
