// Device-compiled view of the fused two-product primitive of the PRODUCT's field.cuh (Fp::mul2, mulsub, neg_operand; Fp2::mul2,
// mulsub, mul) operand by operand, and of ec_madd as the G1 accumulate loop instantiates it, step by step with nothing
// canonicalised in between.  Test-only; never part of libhekaton.  Built twice by the Makefile next to it: as shipped and with
// -DHK_NO_ASM_MUL (the sum of two products).  Operands enter and results leave as raw limbs.
#include "../../../hekaton_system_amd/csrc/ec.cuh"
#include "../shim_common.cuh"

enum Mul2Op { M_MUL2 = 0, M_MULSUB, M_MUL, M_NOPS };

// one lane per tuple; a, b, c, d, out: n x F::N limbs.  One kernel per operation, so that each stands in the code the way a
// caller's single use of it does
template <class F, int OP, int V>
__global__ void __launch_bounds__(64)
k_mul2_op(const u32* __restrict__ a, const u32* __restrict__ b, const u32* __restrict__ c, const u32* __restrict__ d,
          u32* __restrict__ out, u32 n) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F x, y, z, w, r;
    ld_raw(x, a + (size_t)i * F::N);
    ld_raw(y, b + (size_t)i * F::N);
    ld_raw(z, c + (size_t)i * F::N);
    ld_raw(w, d + (size_t)i * F::N);
    if constexpr (OP == M_MUL2) r = F::mul2(x, y, z, w);
    else if constexpr (OP == M_MULSUB) r = F::mulsub(x, y, z, w);
    else r = F::mul(x, y);
    st_raw(out + (size_t)i * F::N, r);
}

// one lane per case: acc <- ec_madd(acc, bases[step]) for `steps` steps, the registers stored as they stand after every step.
// acc: n x 4 N limbs (x, y, zz, zzz), bases: n x steps x 2 N, out: n x steps x 4 N
template <class F, int V>
__global__ void __launch_bounds__(64)
k_madd_chain(const u32* __restrict__ acc, const u32* __restrict__ bases, u32* __restrict__ out, u32 n, u32 steps) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    XYZZ<F> A;
    const u32* pa = acc + (size_t)i * 4 * F::N;
    ld_raw(A.x, pa); ld_raw(A.y, pa + F::N); ld_raw(A.zz, pa + 2 * F::N); ld_raw(A.zzz, pa + 3 * F::N);
    HK_NOUNROLL for (u32 s = 0; s < steps; s++) {
        Affine<F> Q;
        const u32* pq = bases + ((size_t)i * steps + s) * 2 * F::N;
        ld_raw(Q.x, pq); ld_raw(Q.y, pq + F::N);
        A = ec_madd<F, true>(A, Q);                  // the inline P == Q corner, as k_msm_accum0 asks for it in G1
        u32* po = out + ((size_t)i * steps + s) * 4 * F::N;
        st_raw(po, A.x); st_raw(po + F::N, A.y); st_raw(po + 2 * F::N, A.zz); st_raw(po + 3 * F::N, A.zzz);
    }
}

namespace {

template <class F>
int mul2_op(int op, const void* a, const void* b, const void* c, const void* e, void* out, size_t n) {
    size_t bytes = n * F::N * sizeof(u32);
    DevBufs d;
    const u32 *da, *db, *dc, *de;
    u32* dout;
    SHIM_GET(&da, bytes, a);
    SHIM_GET(&db, bytes, b);
    SHIM_GET(&dc, bytes, c);
    SHIM_GET(&de, bytes, e);
    SHIM_GET(&dout, bytes, nullptr);
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    if (op == M_MUL2) hipLaunchKernelGGL((k_mul2_op<F, M_MUL2, VARIANT>), grid, block, 0, 0, da, db, dc, de, dout, (u32)n);
    else if (op == M_MULSUB) hipLaunchKernelGGL((k_mul2_op<F, M_MULSUB, VARIANT>), grid, block, 0, 0, da, db, dc, de, dout, (u32)n);
    else hipLaunchKernelGGL((k_mul2_op<F, M_MUL, VARIANT>), grid, block, 0, 0, da, db, dc, de, dout, (u32)n);
    return finish(out, dout, bytes);
}

// the -DHK_NO_ASM_MUL mixed add of a 12-limb field outgrows the code-object bounds (op_built in ../ec_dev_shim.hip)
template <class F>
constexpr bool chain_built() {
#if defined(HK_NO_ASM_MUL)
    return F::N <= 8;
#else
    return true;
#endif
}

template <class F>
int madd_chain(const void* acc, const void* bases, void* out, size_t n, unsigned steps) {
    if constexpr (chain_built<F>()) {
        size_t pt = 4 * F::N * sizeof(u32);
        DevBufs d;
        const u32 *dacc, *dbases;
        u32* dout;
        SHIM_GET(&dacc, n * pt, acc);
        SHIM_GET(&dbases, n * steps * (pt / 2), bases);
        SHIM_GET(&dout, n * steps * pt, nullptr);
        hipLaunchKernelGGL((k_madd_chain<F, VARIANT>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, dacc, dbases, dout, (u32)n, steps);
        return finish(out, dout, n * steps * pt);
    }
    return -(int)hipErrorNotSupported;
}

}  // namespace

extern "C" {
// 1 when the arithmetic was compiled with the inline assembly of mont_asm.h, 0 for the -DHK_NO_ASM_MUL build
int dshim_mul2_uses_asm(void) { return VARIANT; }
// field: 0 bn254 Fr, 1 bn254 Fq, 2 bls Fr, 3 bls Fq, 4 bn254 Fq2, 5 bls Fq2; op: Mul2Op (M_MUL takes a and b only, and
// exists for the extensions only); a, b, c, e, out: n elements of raw limbs.  Returns 0 or minus the first failing hipError_t.
int dshim_mul2_op(int field, int op, const void* a, const void* b, const void* c, const void* e, void* out, size_t n) {
    if (op < 0 || op >= M_NOPS || n == 0 || n > (1u << 20) || !a || !b || !c || !e || !out) return -(int)hipErrorInvalidValue;
    if (op == M_MUL && field < 4) return -(int)hipErrorInvalidValue;
    switch (field) {
        case 0: return mul2_op<Fp<Bn254FrP>>(op, a, b, c, e, out, n);
        case 1: return mul2_op<Fp<Bn254FqP>>(op, a, b, c, e, out, n);
        case 2: return mul2_op<Fp<Bls381FrP>>(op, a, b, c, e, out, n);
        case 3: return mul2_op<Fp<Bls381FqP>>(op, a, b, c, e, out, n);
        case 4: return mul2_op<Fp2<Bn254FqP>>(op, a, b, c, e, out, n);
        case 5: return mul2_op<Fp2<Bls381FqP>>(op, a, b, c, e, out, n);
    }
    return -(int)hipErrorInvalidValue;
}
// curve: 0 bn254 G1, 1 bls12-381 G1; acc: n XYZZ points, bases: n x steps affine points, out: n x steps XYZZ points, raw limbs.
// Returns 0, minus hipErrorNotSupported where this build leaves the chain out, or minus the first failing hipError_t.
int dshim_madd_chain(int curve, const void* acc, const void* bases, void* out, size_t n, unsigned steps) {
    if (n == 0 || n > 4096 || steps == 0 || steps > 4096 || !acc || !bases || !out) return -(int)hipErrorInvalidValue;
    if (curve == 0) return madd_chain<Fp<Bn254FqP>>(acc, bases, out, n, steps);
    if (curve == 1) return madd_chain<Fp<Bls381FqP>>(acc, bases, out, n, steps);
    return -(int)hipErrorInvalidValue;
}
}
