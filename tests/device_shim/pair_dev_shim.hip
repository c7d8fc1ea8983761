// Device-compiled view of the PRODUCT's multi-pairing pipeline, stage by stage (hipcc, gfx950): the quad-lane Fq2 of endo.cuh
// (Fp2Q: DPP quad broadcast, role pick, the three- and two-product recombinations), k_pair_lines in BOTH of its forms (one
// lane per G2 point, a quad of lanes per point), k_pair_tree_lines, k_pair_tree and k_pair_horner of pairing_wave.cuh.
// PairRun<P>::run (pairing_driver_impl.cuh) chains them with n, n_r and the group size it derives itself; here the caller
// chooses the form, the sizes and the data - hand-made lines, G1 entries that are no curve points, Fq12 values that are no
// Miller products - so that every seam of the pipeline is compared with integers alone.  Test-only; never part of libhekaton.
//
// Built as shipped only by the Makefile next to it (with -DHK_NO_ASM_MUL the quad-lane addition step of BLS12-381 outgrows
// the code-object bounds: see the Makefile's header).  The kernels are the product's own templates under their product
// names; what keeps this library's launches on its own code objects is the -Bsymbolic link of the Makefile and a loader that
// does not merge the libraries' symbols (ctypes: RTLD_LOCAL), as for ec_dev_shim.hip.  k_f2q_op exists here only and carries
// the variant in its name.
//
// Operands of k_f2q_op enter as raw limbs; the pipeline kernels read memory through the product's ld_vec, as they do in the
// product.  Every HIP status is returned to the caller; the shim allocates and frees its own buffers and never touches an
// hk_ctx.
#include "../../hekaton_system_amd/csrc/pairing_driver_impl.cuh"
#include "shim_common.cuh"

enum F2qOp { Q_MUL = 0, Q_SQR, Q_MUL_BY_CHAR, Q_PSI, Q_NOPS };

// the quad-lane forms of shim_common.cuh's raw access: this shim alone includes endo.cuh's Fp2Q
template <class P> __device__ __forceinline__ void ld_raw(Fp2Q<P>& f, const u32* p) { ld_raw(f.c0, p); ld_raw(f.c1, p + P::N); }
template <class P> __device__ __forceinline__ void st_canon(u32* p, const Fp2Q<P>& f) {
    Fp<P> c0 = Fp<P>::canon(f.c0), c1 = Fp<P>::canon(f.c1);
    HK_UNROLL for (int i = 0; i < P::N; i++) { p[i] = c0.v[i]; p[P::N + i] = c1.v[i]; }
}

// element i on lanes 4 i .. 4 i + 3 of 64-lane blocks (the last block partly filled, as in k_pair_lines<Fp2Q<P>>).
// a, b: n Fq2 of raw limbs - the factors of Q_MUL, the argument of Q_SQR (b unused), the x and y of the point of
// Q_MUL_BY_CHAR / Q_PSI.  out: what EACH lane holds, canonical: n x 4 Fq2 (Q_MUL, Q_SQR) or n x 4 x (x, y) (the point ops).
template <class P, int V>
__global__ void __launch_bounds__(64)
k_f2q_op(int op, const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out, u32 n) {
    typedef Fp2Q<P> F;
    u32 t = blockIdx.x * blockDim.x + threadIdx.x, i = t / 4;
    if (i >= n) return;
    constexpr int W = 2 * P::N;                      // words per Fq2
    F x, y;
    ld_raw(x, a + (size_t)i * W);
    ld_raw(y, b + (size_t)i * W);
    if (op == Q_MUL) st_canon(out + (size_t)t * W, F::mul(x, y));
    else if (op == Q_SQR) st_canon(out + (size_t)t * W, F::sqr(x));
    else {
        Affine<F> q, r;
        q.x = x; q.y = y;
        if (op == Q_MUL_BY_CHAR) r = pair_mul_by_char(q);
        else r = EndoOf<F>::apply(q);
        st_canon(out + (size_t)t * 2 * W, r.x);
        st_canon(out + (size_t)t * 2 * W + W, r.y);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
namespace {

template <class P> size_t lds_tree() { return sizeof(WaveArea<P>) + 2 * WV_SLOT * sizeof(Fp<P>); }                 // as PairRun::run
template <class P> size_t lds_fin() { return sizeof(WaveArea<P>) + WV_FINISH_SLOTS * WV_SLOT * sizeof(Fp<P>); }
template <class P> PairSteps steps_of() { return pair_steps(PairLoopOf<P>::get(), TowerParams<P>::TWIST_IS_D); }

template <class P>
int f2q_op(int op, const void* a, const void* b, void* out, size_t n) {
    if (op == Q_MUL_BY_CHAR && !TowerParams<P>::TWIST_IS_D) return -(int)hipErrorInvalidValue;    // ark has it on BN only
    size_t in_bytes = n * 2 * sizeof(Fp<P>), out_bytes = n * 4 * (op >= Q_MUL_BY_CHAR ? 2 : 1) * 2 * sizeof(Fp<P>);
    DevBufs d;
    const u32 *da, *db;
    u32* dout;
    SHIM_GET(&da, in_bytes, a);
    SHIM_GET(&db, in_bytes, b ? b : a);
    SHIM_GET(&dout, out_bytes, nullptr);
    hipLaunchKernelGGL((k_f2q_op<P, VARIANT>), dim3((unsigned)((4 * n + 63) / 64)), dim3(64), 0, 0, op, da, db, dout, (u32)n);
    return finish(out, dout, out_bytes);
}

// g2: n_r vectors of n affine G2 points (memory form) -> the raw lines [(b * S + s) * n + i], the grids of PairRun::run
template <class P>
int pair_lines(int form, const void* g2, unsigned n, unsigned n_r, void* lines_out, unsigned* S_out) {
    PairLoop loop = PairLoopOf<P>::get();
    u32 S = (u32)steps_of<P>().n;
    size_t in_bytes = (size_t)n_r * n * sizeof(Affine<Fp2<P>>), out_bytes = (size_t)n_r * S * n * sizeof(Line6<P>);
    DevBufs d;
    const Affine<Fp2<P>>* pts;
    Line6<P>* lines;
    SHIM_GET(&pts, in_bytes, g2);
    SHIM_GET(&lines, out_bytes, nullptr);                          // 0xA5: a line the kernel does not write is no line
    if (form == 1)
        hipLaunchKernelGGL((k_pair_lines<Fp2Q<P>>), dim3((4 * n + 63) / 64, n_r), dim3(64), 0, 0, (const Affine<Fp2Q<P>>*)pts, n,
                           n_r, loop, S, lines);
    else
        hipLaunchKernelGGL((k_pair_lines<Fp2<P>>), dim3((n + 63) / 64, n_r), dim3(64), 0, 0, pts, n, n_r, loop, S, lines);
    int st = finish(lines_out, lines, out_bytes);
    if (st == 0) *S_out = S;
    return st;
}

// lines: [n_r][S][n] raw lines, g1: [n_l][n] affine points; out: [count][S][ceil(n / c)] Fq12, count = n_pairs or n_l n_r
template <class P>
int pair_tree_lines(const void* lines, const void* g1, unsigned n, unsigned c, unsigned n_l, unsigned n_r, unsigned S,
                    const PairList& pl, void* out) {
    u32 count = pl.n ? pl.n : n_l * n_r, groups = (n + c - 1) / c;
    if ((size_t)count * S > 65535) return -(int)hipErrorInvalidValue;            // grid.y
    size_t lb = (size_t)n_r * S * n * sizeof(Line6<P>), gb = (size_t)n_l * n * sizeof(Affine<Fp<P>>);
    size_t ob = (size_t)count * S * groups * sizeof(Fp12<P>);
    DevBufs d;
    const Line6<P>* d_lines;
    const Affine<Fp<P>>* d_g1;
    Fp12<P>* d_out;
    SHIM_GET(&d_lines, lb, lines);
    SHIM_GET(&d_g1, gb, g1);
    SHIM_GET(&d_out, ob, nullptr);
    hipLaunchKernelGGL((k_pair_tree_lines<P>), dim3(groups, count * S), dim3(64), lds_tree<P>(), 0, d_lines, d_g1, n, c, n_r, S, pl,
                       d_out);
    return finish(out, d_out, ob);
}

// in: [count][n] canonical Fq12 -> out: [count][ceil(n / c)]
template <class P>
int pair_tree(const void* in, unsigned n, unsigned c, unsigned count, void* out) {
    u32 groups = (n + c - 1) / c;
    size_t ib = (size_t)count * n * sizeof(Fp12<P>), ob = (size_t)count * groups * sizeof(Fp12<P>);
    DevBufs d;
    const Fp12<P>* d_in;
    Fp12<P>* d_out;
    SHIM_GET(&d_in, ib, in);
    SHIM_GET(&d_out, ob, nullptr);
    hipLaunchKernelGGL((k_pair_tree<P>), dim3(groups, count), dim3(64), lds_tree<P>(), 0, d_in, n, c, d_out);
    return finish(out, d_out, ob);
}

// L: [count][S] canonical Fq12 (S = the steps of the curve's loop) -> out: [count]
template <class P>
int pair_horner(const void* L, unsigned count, void* out) {
    PairSteps st = steps_of<P>();
    size_t ib = (size_t)count * st.n * sizeof(Fp12<P>), ob = (size_t)count * sizeof(Fp12<P>);
    DevBufs d;
    const Fp12<P>* d_in;
    Fp12<P>* d_out;
    SHIM_GET(&d_in, ib, L);
    SHIM_GET(&d_out, ob, nullptr);
    hipLaunchKernelGGL((k_pair_horner<P>), dim3(count), dim3(64), lds_fin<P>(), 0, d_in, st, d_out);
    return finish(out, d_out, ob);
}

}  // namespace

extern "C" {
int dshim_pair_uses_asm(void) { return VARIANT; }
// line steps of the curve's Miller loop (the S of the entry points below), 0 for an unknown curve
unsigned dshim_pair_steps(int curve) {
    return curve == 0 ? (unsigned)steps_of<Bn254FqP>().n : curve == 1 ? (unsigned)steps_of<Bls381FqP>().n : 0u;
}
// Every entry point: curve 0 bn254, 1 bls12-381; returns 0, or minus the first failing hipError_t.
//
// op: F2qOp on Fp2Q<P>; a, b: n Fq2 of raw limbs (b may be null for Q_SQR); out: n x 4 Fq2 (Q_MUL, Q_SQR) or n x 4 x 2 Fq2
// (Q_MUL_BY_CHAR - bn254 only - and Q_PSI: a holds x, b holds y), canonical, one entry per LANE of the element's quad
int dshim_f2q_op(int curve, int op, const void* a, const void* b, void* out, size_t n) {
    if (op < 0 || op >= Q_NOPS || n == 0 || n > (1u << 20) || !a || !out || (!b && op != Q_SQR)) return -(int)hipErrorInvalidValue;
    if (curve == 0) return f2q_op<Bn254FqP>(op, a, b, out, n);
    if (curve == 1) return f2q_op<Bls381FqP>(op, a, b, out, n);
    return -(int)hipErrorInvalidValue;
}
// form: 0 k_pair_lines<Fp2<P>> (a lane per point), 1 k_pair_lines<Fp2Q<P>> (a quad per point); g2: n_r x n affine points;
// lines_out: n_r x S x n Line6 (6 Fq each), S_out: S
int dshim_pair_lines(int curve, int form, const void* g2, unsigned n, unsigned n_r, void* lines_out, unsigned* S_out) {
    if (form < 0 || form > 1 || n == 0 || n > (1u << 16) || n_r == 0 || n_r > 64 || !g2 || !lines_out || !S_out)
        return -(int)hipErrorInvalidValue;
    if (curve == 0) return pair_lines<Bn254FqP>(form, g2, n, n_r, lines_out, S_out);
    if (curve == 1) return pair_lines<Bls381FqP>(form, g2, n, n_r, lines_out, S_out);
    return -(int)hipErrorInvalidValue;
}
// lines: n_r x S x n raw Line6; g1: n_l x n affine points; c: values per group; pair_a / pair_b: n_pairs (lhs, rhs) vector
// indices, or null with n_pairs = 0 for the whole n_l x n_r grid; out: count x S x ceil(n / c) Fq12
int dshim_pair_tree_lines(int curve, const void* lines, const void* g1, unsigned n, unsigned c, unsigned n_l, unsigned n_r,
                          unsigned S, const unsigned* pair_a, const unsigned* pair_b, unsigned n_pairs, void* out) {
    if (n == 0 || n > (1u << 16) || c == 0 || n_l == 0 || n_l > 64 || n_r == 0 || n_r > 64 || S == 0 || S > 100 || !lines || !g1 ||
        !out || n_pairs > (unsigned)PAIR_LIST_MAX || (n_pairs && (!pair_a || !pair_b)))
        return -(int)hipErrorInvalidValue;
    PairList pl;
    pl.n = n_pairs;
    for (unsigned k = 0; k < n_pairs; k++) {
        if (pair_a[k] >= n_l || pair_b[k] >= n_r) return -(int)hipErrorInvalidValue;
        pl.a[k] = (unsigned char)pair_a[k];
        pl.b[k] = (unsigned char)pair_b[k];
    }
    if (curve == 0) return pair_tree_lines<Bn254FqP>(lines, g1, n, c, n_l, n_r, S, pl, out);
    if (curve == 1) return pair_tree_lines<Bls381FqP>(lines, g1, n, c, n_l, n_r, S, pl, out);
    return -(int)hipErrorInvalidValue;
}
// in: count x n canonical Fq12; out: count x ceil(n / c)
int dshim_pair_tree(int curve, const void* in, unsigned n, unsigned c, unsigned count, void* out) {
    if (n == 0 || n > (1u << 16) || c == 0 || count == 0 || count > 65535 || !in || !out) return -(int)hipErrorInvalidValue;
    if (curve == 0) return pair_tree<Bn254FqP>(in, n, c, count, out);
    if (curve == 1) return pair_tree<Bls381FqP>(in, n, c, count, out);
    return -(int)hipErrorInvalidValue;
}
// L: count x S canonical Fq12, S = dshim_pair_steps(curve); out: count Fq12
int dshim_pair_horner(int curve, const void* L, unsigned count, void* out) {
    if (count == 0 || count > 4096 || !L || !out) return -(int)hipErrorInvalidValue;
    if (curve == 0) return pair_horner<Bn254FqP>(L, count, out);
    if (curve == 1) return pair_horner<Bls381FqP>(L, count, out);
    return -(int)hipErrorInvalidValue;
}
}
