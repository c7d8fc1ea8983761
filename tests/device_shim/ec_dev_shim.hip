// Device-compiled view of the PRODUCT's ec.cuh (group law on XYZZ coordinates), of k_batch_affine (fixed_base.cuh) and of
// the MSM launch sequence of msm_driver_impl.cuh under a plan the CALLER forces (hipcc, gfx950).  The host build of
// tests/host_shim/field_shim.cpp compiles the canonical C++ only; here the exceptional cases of the group law meet the lazy
// [0, 2p) representatives and the inline assembly the kernels really run, one lane per case, and every window size c = 3 .. 16
// runs the product's sort, accumulate, level chain and reductions on vectors that no caller-visible plan would give it.
// Test-only; never part of libhekaton.
//
// One translation unit per group (-DSHIM_GROUP=0..3: the ladder of shim_common.cuh), linked into one library; group 0's
// unit also holds the extern "C" entry points.  Built twice by the Makefile next to it:
// as shipped, and with -DHK_NO_ASM_MUL -DEC_SHIM_NO_MSM (the C++ fallback under the same lazy representation; group law
// and batch inversion only).  Only forms the product ships are instantiated: ec_madd<F, AccumInlineCorner<F>::value> is
// the accumulate loop's, so the inlined P == Q corner of a 12-limb G2 does not exist here either.
//
// Operands enter as raw limbs; every HIP status is returned to the caller; the shim allocates and frees its own buffers
// and never touches an hk_ctx.
#include "../../hekaton_system_amd/csrc/msm_driver_impl.cuh"
#ifndef SHIM_GROUP
#error "compile with -DSHIM_GROUP=0..3"
#endif
#define SHIM_PREFIX ec_shim
#include "shim_common.cuh"

enum GroupOp { G_MADD = 0, G_MADD_NI, G_ADD, G_ADD_NI, G_DBL, G_DBL_NI, G_DBL_AFFINE, G_NEG, G_TO_AFFINE, G_MUL_SMALL,
               G_MUL_LIMBS, G_MADD_CHAIN, G_NOPS };

// Both variants (and libhekaton) get loaded into one test process, and each library must launch its own kernels.  The
// kernels with product names (k_batch_affine<...>, k_msm_*<...>) are the same symbols in all three: what keeps them apart is
// the -Bsymbolic link of the shim Makefile (a library's launches bind to its own kernel handles) together with a loader
// that does not merge the libraries' symbols (ctypes: RTLD_LOCAL).  k_group_op exists in the two shim builds only and
// carries VARIANT in its name as well, so that a kernel trace tells them apart.

// one lane per case.  a: n XYZZ points (x, y, zz, zzz), b: n slots of the same size - an XYZZ point, an affine point in its
// first half, or the 8 limbs of a canonical scalar (G_MUL_LIMBS); out: n slots: the XYZZ registers as they stand (raw) or
// through the product's st_vec; affine results fill the first half, the rest is zero.  k: the factor of G_MUL_SMALL, the
// number of mixed adds of G_MADD_CHAIN.
template <class F, int OP, int V>
__global__ void __launch_bounds__(64)
k_group_op(const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out, u32 n, int raw, u32 k) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int W = 4 * F::N;                      // words per slot
    const u32* pa = a + (size_t)i * W;
    const u32* pb = b + (size_t)i * W;
    u32* po = out + (size_t)i * W;
    XYZZ<F> A, B, R;
    Affine<F> Q;
    ld_raw(A.x, pa); ld_raw(A.y, pa + F::N); ld_raw(A.zz, pa + 2 * F::N); ld_raw(A.zzz, pa + 3 * F::N);
    ld_raw(B.x, pb); ld_raw(B.y, pb + F::N); ld_raw(B.zz, pb + 2 * F::N); ld_raw(B.zzz, pb + 3 * F::N);
    Q.x = B.x; Q.y = B.y;
    if constexpr (OP == G_TO_AFFINE) {
        Affine<F> r = ec_to_affine(A);
        if (raw) { st_raw(po, r.x); st_raw(po + F::N, r.y); }
        else st_vec(reinterpret_cast<Affine<F>*>(po), r);
        for (int j = 2 * F::N; j < W; j++) po[j] = 0;
        return;
    } else if constexpr (OP == G_MADD) R = ec_madd<F, AccumInlineCorner<F>::value>(A, Q);     // the accumulate loop's form
    else if constexpr (OP == G_MADD_NI) R = ec_madd_ni(A, Q);
    else if constexpr (OP == G_ADD) R = ec_add(A, B);
    else if constexpr (OP == G_ADD_NI) R = ec_add_ni(A, B);
    else if constexpr (OP == G_DBL) R = ec_dbl(A);
    else if constexpr (OP == G_DBL_NI) R = ec_dbl_ni(A);
    else if constexpr (OP == G_DBL_AFFINE) R = ec_dbl_affine(Q);
    else if constexpr (OP == G_NEG) R = ec_neg(A);
    else if constexpr (OP == G_MUL_SMALL) R = ec_mul_small(A, k);
    else if constexpr (OP == G_MUL_LIMBS) {
        u32 s[8];
        for (int j = 0; j < 8; j++) s[j] = pb[j];
        R = ec_mul_limbs(A, s);
    } else {                                         // G_MADD_CHAIN: nothing canonicalised between the steps
        R = A;
        HK_NOUNROLL for (u32 j = 0; j < k; j++) R = ec_madd<F, AccumInlineCorner<F>::value>(R, Q);
    }
    if (raw) { st_raw(po, R.x); st_raw(po + F::N, R.y); st_raw(po + 2 * F::N, R.zz); st_raw(po + 3 * F::N, R.zzz); }
    else st_vec(reinterpret_cast<XYZZ<F>*>(po), R);
}

// ---- host side ---------------------------------------------------------------------------------------------------
namespace {

// The C++ fallback of the Montgomery product is several times the size of the assembly, and two flavours of the group law
// outgrow the code-object bounds with it (tools/kernel_meta.py --check refuses the library): every
// form that adds two points in 8-limb G2 (ec_add_ni alone is 160 KB there), and the INLINED mixed add of 12-limb G1.  The
// -DHK_NO_ASM_MUL build leaves those out and answers hipErrorNotSupported for them; the as-shipped build holds every op.
constexpr bool op_built(int op) {
#if defined(HK_NO_ASM_MUL) && SHIM_GROUP == 1
    return op == G_DBL || op == G_DBL_NI || op == G_DBL_AFFINE || op == G_NEG || op == G_TO_AFFINE;
#elif defined(HK_NO_ASM_MUL) && SHIM_GROUP == 2
    return op != G_MADD && op != G_MADD_CHAIN;
#else
    return op >= 0;
#endif
}

template <class F, int OP>
bool launch_op(const u32* a, const u32* b, u32* out, u32 n, int raw, u32 k) {
    if constexpr (op_built(OP)) {
        hipLaunchKernelGGL((k_group_op<F, OP, VARIANT>), dim3((n + 63) / 64), dim3(64), 0, 0, a, b, out, n, raw, k);
        return true;
    }
    return false;
}

template <class F>
int group_op(int op, const void* a, const void* b, void* out, size_t n, int raw, unsigned k) {
    if (!op_built(op)) return -(int)hipErrorNotSupported;
    size_t bytes = n * sizeof(XYZZ<F>);
    DevBufs d;
    const u32 *da, *db;
    u32* dout;
    SHIM_GET(&da, bytes, a);
    SHIM_GET(&db, bytes, b ? b : a);
    SHIM_GET(&dout, bytes, nullptr);
    switch (op) {
        case G_MADD: launch_op<F, G_MADD>(da, db, dout, (u32)n, raw, k); break;
        case G_MADD_NI: launch_op<F, G_MADD_NI>(da, db, dout, (u32)n, raw, k); break;
        case G_ADD: launch_op<F, G_ADD>(da, db, dout, (u32)n, raw, k); break;
        case G_ADD_NI: launch_op<F, G_ADD_NI>(da, db, dout, (u32)n, raw, k); break;
        case G_DBL: launch_op<F, G_DBL>(da, db, dout, (u32)n, raw, k); break;
        case G_DBL_NI: launch_op<F, G_DBL_NI>(da, db, dout, (u32)n, raw, k); break;
        case G_DBL_AFFINE: launch_op<F, G_DBL_AFFINE>(da, db, dout, (u32)n, raw, k); break;
        case G_NEG: launch_op<F, G_NEG>(da, db, dout, (u32)n, raw, k); break;
        case G_TO_AFFINE: launch_op<F, G_TO_AFFINE>(da, db, dout, (u32)n, raw, k); break;
        case G_MUL_SMALL: launch_op<F, G_MUL_SMALL>(da, db, dout, (u32)n, raw, k); break;
        case G_MUL_LIMBS: launch_op<F, G_MUL_LIMBS>(da, db, dout, (u32)n, raw, k); break;
        default: launch_op<F, G_MADD_CHAIN>(da, db, dout, (u32)n, raw, k); break;
    }
    return finish(out, dout, bytes);
}

// the product's k_batch_affine with the caller's chunk (MsmRun::batch_affine derives it from n: 1 up to 65 536 points)
template <class F>
int batch_affine(const void* in, void* out, size_t n, unsigned chunk) {
    DevBufs d;
    const XYZZ<F>* pts;
    Affine<F>* aff;
    F* tmp;
    SHIM_GET(&pts, n * sizeof(XYZZ<F>), in);
    SHIM_GET(&aff, n * sizeof(Affine<F>), nullptr);
    SHIM_GET(&tmp, n * sizeof(F), nullptr);
    u32 lanes = (u32)((n + chunk - 1) / chunk);
    hipLaunchKernelGGL((k_batch_affine<F>), dim3((lanes + 63) / 64), dim3(64), 0, 0, pts, aff, tmp, (u32)n, (u32)chunk);
    return finish(out, aff, n * sizeof(Affine<F>));
}

#if !defined(EC_SHIM_NO_MSM)
// `batch` MSMs of n scalars each over ONE table of n_bases bases (base j goes with scalar j + idx_off), under the plan
// (c, WP): the product's own sequence - plan, shift tables, digit sort, bucket pass, normalisation - on one hipMalloc.
// plan_out (optional, 9 words): W, F, NB, n_levels, T[0], T[1], Lmin0, K of the lane plan MsmRun::run derives, and the
// lanes that plan may use at most (AccumOcc<F>::waves x 65 536 / batch).
template <class C, class F>
int msm(unsigned c, unsigned WP, unsigned batch, unsigned n, unsigned n_bases, unsigned idx_off, const void* bases,
        const void* scalars, int mont, void* out, unsigned* plan_out) {
    typedef typename C::Fr Fr;
    MsmPlan p = msm_make_plan(n, C::FR_BITS, c, WP, 262144u, Fr::Params::MOD, Fr::Params::N);
    if (plan_out) {
        MsmPlan lp = msm_lane_plan<F>(p, batch);
        plan_out[0] = lp.W; plan_out[1] = lp.F; plan_out[2] = lp.NB; plan_out[3] = lp.n_levels; plan_out[4] = lp.T[0];
        plan_out[5] = lp.n_levels > 1 ? lp.T[1] : 0; plan_out[6] = lp.Lmin0; plan_out[7] = lp.K;
        plan_out[8] = (u32)AccumOcc<F>::waves * 65536u / batch;
    }
    Affine<F>* table = nullptr;
    u32* sc = nullptr;
    XYZZ<F>* res = nullptr;
    Affine<F>* aff = nullptr;
    SortBufs sb;
    typename MsmRun<F>::Bufs rb;
    const size_t tab_n = (size_t)p.F * (n_bases ? n_bases : 1u);
    auto carve = [&](Carve& cv) {
        table = cv.n<Affine<F>>(tab_n);
        sc = (u32*)cv.take((size_t)batch * n * sizeof(Fr));
        MsmSort<Fr>::alloc(cv, p, &sb, batch);
        MsmRun<F>::alloc(cv, p, &rb, batch);
        res = cv.n<XYZZ<F>>(batch);
        aff = cv.n<Affine<F>>(batch);
    };
    Carve count;
    carve(count);
    DevBufs d;
    Carve real;
    SHIM_GET(&real.base, count.off + 256, nullptr);                // 0xA5: no stage may rely on cleared scratch
    carve(real);
    if (n_bases) SHIM_TRY(hipMemcpy(table, bases, (size_t)n_bases * sizeof(Affine<F>), hipMemcpyHostToDevice));
    SHIM_TRY(hipMemcpy(sc, scalars, (size_t)batch * n * sizeof(Fr), hipMemcpyHostToDevice));
    hk_status st = HK_OK;
    if (p.F > 1) st = MsmRun<F>::build_tables(0, table, n_bases, p.F, p.c * p.WP);
    if (st == HK_OK) st = MsmSort<Fr>::run(0, p, sc, mont, sb, false, batch, n);
    if (st == HK_OK) st = MsmRun<F>::run(0, p, table, n_bases, idx_off, sb, rb, res, nullptr, nullptr, batch, 1);
    if (st == HK_OK) st = MsmRun<F>::to_affine(0, res, aff, batch);
    SHIM_TRY(hipDeviceSynchronize());
    if (st != HK_OK) return (int)st;
    SHIM_TRY(hipMemcpy(out, aff, (size_t)batch * sizeof(Affine<F>), hipMemcpyDeviceToHost));
    return 0;
}
#endif

}  // namespace

// ---- per-group entry points (C++ linkage inside the library) ---------------------------------------------------------
int SHIM_FN(group_op)(int op, const void* a, const void* b, void* out, size_t n, int raw, unsigned k) {
    return group_op<ShimF>(op, a, b, out, n, raw, k);
}
int SHIM_FN(op_built)(int op) { return op_built(op) ? 1 : 0; }
int SHIM_FN(batch_affine)(const void* in, void* out, size_t n, unsigned chunk) { return batch_affine<ShimF>(in, out, n, chunk); }
#if !defined(EC_SHIM_NO_MSM)
int SHIM_FN(msm)(unsigned c, unsigned WP, unsigned batch, unsigned n, unsigned n_bases, unsigned idx_off, const void* bases,
                 const void* scalars, int mont, void* out, unsigned* plan_out) {
    return msm<ShimCurve, ShimF>(c, WP, batch, n, n_bases, idx_off, bases, scalars, mont, out, plan_out);
}
#endif

#if SHIM_GROUP == 0
#define SHIM_DECL(g)                                                                                                        \
    int ec_shim_g##g##_group_op(int, const void*, const void*, void*, size_t, int, unsigned);                              \
    int ec_shim_g##g##_op_built(int);                                                                                      \
    int ec_shim_g##g##_batch_affine(const void*, void*, size_t, unsigned);                                                 \
    int ec_shim_g##g##_msm(unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, const void*, const void*, int, void*, \
                           unsigned*);
SHIM_DECL(1) SHIM_DECL(2) SHIM_DECL(3)

extern "C" {
int dshim_ec_uses_asm(void) { return VARIANT; }
// 1 when dshim_msm is part of this build
int dshim_ec_has_msm(void) {
#if defined(EC_SHIM_NO_MSM)
    return 0;
#else
    return 1;
#endif
}
// 1 when this build holds `op` for `group` (see op_built), else 0
int dshim_ec_op_built(int group, int op) {
    if (op < 0 || op >= G_NOPS || group < 0 || group > 3) return 0;
    SHIM_DISPATCH(group, op_built(op))
}
// group: 0 bn254 G1, 1 bn254 G2, 2 bls G1, 3 bls G2 (as shim_group_op); op: GroupOp; a, b, out: n slots of 4 coordinate-field
// elements, raw limbs (see k_group_op); raw: store the registers as they stand instead of through st_vec.
// Returns 0, or minus the first failing hipError_t (hipErrorInvalidValue for an unknown group, as every entry point below).
int dshim_group_op(int group, int op, const void* a, const void* b, void* out, size_t n, int raw, unsigned k) {
    if (op < 0 || op >= G_NOPS || n == 0 || n > (1u << 20) || !a || !out) return -(int)hipErrorInvalidValue;
    if (op == G_MADD_CHAIN && k > 4096) return -(int)hipErrorInvalidValue;
    SHIM_DISPATCH(group, group_op(op, a, b, out, n, raw, k))
}
// in: n XYZZ points as they lie in memory, out: n affine points; chunk: points per lane (one inversion per lane)
int dshim_batch_affine(int group, const void* in, void* out, size_t n, unsigned chunk) {
    if (n == 0 || n > (1u << 20) || chunk == 0 || chunk > 4096 || !in || !out) return -(int)hipErrorInvalidValue;
    SHIM_DISPATCH(group, batch_affine(in, out, n, chunk))
}
// bases: n_bases affine points (memory form: canonical Montgomery); scalars: batch x n Fr (Montgomery when mont); out: batch
// affine points.  Returns 0, the product's hk_status (> 0) unchanged, or minus the hipError_t of one of the shim's own calls.
int dshim_msm(int group, unsigned c, unsigned WP, unsigned batch, unsigned n, unsigned n_bases, unsigned idx_off,
              const void* bases, const void* scalars, int mont, void* out, unsigned* plan_out) {
#if defined(EC_SHIM_NO_MSM)
    return -(int)hipErrorNotSupported;
#else
    if (c < 3 || c > 16 || WP == 0 || batch == 0 || batch > 8 || n == 0 || n > (1u << 20) || n_bases > (1u << 20) ||
        idx_off > (1u << 20) || !scalars || !out || (n_bases && !bases))
        return -(int)hipErrorInvalidValue;
    SHIM_DISPATCH(group, msm(c, WP, batch, n, n_bases, idx_off, bases, scalars, mont, out, plan_out))
#endif
}
}
#endif
