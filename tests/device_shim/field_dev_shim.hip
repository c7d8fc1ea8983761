// Device-compiled view of the PRODUCT's field.cuh / ec.cuh / pairing_wave.cuh (hipcc, gfx950): one kernel per field type
// and one per curve, so the arithmetic the kernels really run - the inline assembly of mont_asm.h and the lazy [0, 2p)
// forms that the host build of tests/host_shim/field_shim.cpp never compiles - can be tested operand by operand against
// integers.  Test-only; never part of libhekaton.  Built twice by the Makefile next to it: as shipped, and with
// -DHK_NO_ASM_MUL (the C++ fallback under the same lazy representation).
//
// Operands enter as raw limbs (that is how representatives in [p, 2p) get into registers); every HIP status is returned
// to the caller; the shim allocates and frees its own buffers and never touches an hk_ctx.
#include "../../hekaton_system_amd/csrc/ec.cuh"
#include "../../hekaton_system_amd/csrc/pairing_wave.cuh"
#include "shim_common.cuh"

enum FieldOp { F_ADD = 0, F_SUB, F_MUL, F_SQR, F_NEG, F_DBL, F_HALVE, F_CANON, F_TO_MONT, F_FROM_MONT, F_INV, F_IS_ZERO, F_EQ,
               F_CHAIN, F_NOPS };
enum WaveOp { W_MUL = 0, W_SQR, W_CYC_SQR, W_CONJ, W_FROB1, W_FROB2, W_FROB3, W_INV, W_NOPS };

template <class F> struct IsBase { static constexpr bool value = false; };
template <class P> struct IsBase<Fp<P>> { static constexpr bool value = true; };

// one lane per element; a, b, out: n x F::N limbs
template <class F, int V>
__global__ void __launch_bounds__(64)
k_field_op(int op, const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out, u32 n, int raw, int chain) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F x, y, r;
    ld_raw(x, a + (size_t)i * F::N);
    ld_raw(y, b + (size_t)i * F::N);
    int flag = -1;
    switch (op) {
        case F_ADD: r = F::add(x, y); break;
        case F_SUB: r = F::sub(x, y); break;
        case F_MUL: r = F::mul(x, y); break;
        case F_SQR: r = F::sqr(x); break;
        case F_NEG: r = F::neg(x); break;
        case F_DBL: r = F::dbl(x); break;
        case F_HALVE: r = F::halve(x); break;
        case F_CANON: r = F::canon(x); break;
        case F_INV: r = fp_inv(x); break;
        case F_IS_ZERO: flag = x.is_zero() ? 1 : 0; break;
        case F_EQ: flag = (x == y) ? 1 : 0; break;
        case F_CHAIN:                                   // r <- r y + x - 2 y, nothing canonicalised in between
            r = x;
            HK_NOUNROLL for (int k = 0; k < chain; k++) r = F::sub(F::add(F::mul(r, y), x), F::dbl(y));
            break;
        default:
            if constexpr (IsBase<F>::value) {
                if (op == F_TO_MONT) r = F::to_mont(x);
                else r = F::from_mont(x);
            } else {
                r = F::zero();                          // refused on the host side
            }
    }
    u32* o = out + (size_t)i * F::N;
    if (flag >= 0) {
        for (int k = 0; k < F::N; k++) o[k] = k == 0 ? (u32)flag : 0u;
        return;
    }
    if (!raw) r = F::canon(r);
    st_raw(o, r);
}

// one 64-lane workgroup per element; a, b: n x 12 Fq (raw limbs, NOT canonicalised on the way into LDS);
// out: n x 13 Fq, canonical: the 12 coefficients of dst and its padding slot
template <class P, int V>
__global__ void __launch_bounds__(64)
k_wave_op(int op, const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out, int alias) {
    typedef WaveF12<P> W;
    typedef Fp<P> Fq;
    __shared__ WaveArea<P> area;
    __shared__ Fq slots[4 * WV_SLOT];
    WaveArea<P>* w = &area;
    Fq *A = slots, *B = slots + WV_SLOT, *D = slots + 2 * WV_SLOT, *T = slots + 3 * WV_SLOT;
    u32 lane = threadIdx.x;
    W::init(w);
    if (lane < 12) {
        ld_raw(A[lane], a + ((size_t)blockIdx.x * 12 + lane) * P::N);
        ld_raw(B[lane], b + ((size_t)blockIdx.x * 12 + lane) * P::N);
    }
    if (lane == 12) { A[12] = Fq::zero(); B[12] = Fq::zero(); }
    if (lane < 13) { D[lane] = Fq::one(); T[lane] = Fq::one(); }        // stale content a correct op must overwrite
    W::sync();
    Fq* dst = alias == 0 ? D : (alias == 2 ? B : A);
    const Fq* src = A;
    switch (op) {
        case W_MUL: W::mul(dst, A, alias == 3 ? A : B, w); break;
        case W_SQR: W::sqr(dst, src, w); break;
        case W_CYC_SQR: W::cyc_sqr(dst, src, w); break;
        case W_CONJ: W::conj(dst, src); break;
        case W_FROB1: W::template frob<1>(dst, src); break;
        case W_FROB2: W::template frob<2>(dst, src); break;
        case W_FROB3: W::template frob<3>(dst, src); break;
        default: W::inv(dst, src, T, w); break;                          // dst, a, tmp distinct: alias 0 only
    }
    W::sync();
    if (lane < 13) st_raw(out + ((size_t)blockIdx.x * 13 + lane) * P::N, Fq::canon(dst[lane]));
}

// ---- host side ---------------------------------------------------------------------------------------------------
namespace {

// uploads a and b (in_bytes each), runs launch(da, db, dout), downloads out (out_bytes)
template <class L>
int run(const void* a, const void* b, void* out, size_t in_bytes, size_t out_bytes, L launch) {
    DevBufs d;
    const u32 *da, *db;
    u32* dout;
    SHIM_GET(&da, in_bytes, a);
    SHIM_GET(&db, in_bytes, b ? b : a);
    SHIM_GET(&dout, out_bytes, nullptr);
    launch(da, db, dout);
    return finish(out, dout, out_bytes);
}

template <class F>
int field_op(int op, const void* a, const void* b, void* out, size_t n, int raw, int chain) {
    if (!IsBase<F>::value && (op == F_TO_MONT || op == F_FROM_MONT)) return -(int)hipErrorInvalidValue;
    size_t bytes = n * F::N * sizeof(u32);
    return run(a, b, out, bytes, bytes, [&](const u32* da, const u32* db, u32* dout) {
        hipLaunchKernelGGL((k_field_op<F, VARIANT>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, op, da, db, dout, (u32)n, raw, chain);
    });
}

template <class P>
int wave_op(int op, const void* a, const void* b, void* out, size_t n, int alias) {
    size_t in_bytes = n * 12 * P::N * sizeof(u32), out_bytes = n * 13 * P::N * sizeof(u32);
    return run(a, b, out, in_bytes, out_bytes, [&](const u32* da, const u32* db, u32* dout) {
        hipLaunchKernelGGL((k_wave_op<P, VARIANT>), dim3((unsigned)n), dim3(64), 0, 0, op, da, db, dout, alias);
    });
}

}  // namespace

extern "C" {
// 1 when the arithmetic was compiled with the inline assembly of mont_asm.h, 0 for the -DHK_NO_ASM_MUL build
int dshim_uses_asm(void) { return VARIANT; }
// field: 0 bn254 Fr, 1 bn254 Fq, 2 bls Fr, 3 bls Fq, 4 bn254 Fq2, 5 bls Fq2 (as shim_field_op); op: FieldOp;
// a, b, out: n elements of raw limbs (b may be null for unary ops); raw: store the registers as they stand instead of through
// canon(); chain: iterations of F_CHAIN.  Returns 0 or minus the first failing hipError_t.
int dshim_field_op(int field, int op, const void* a, const void* b, void* out, size_t n, int raw, int chain) {
    if (op < 0 || op >= F_NOPS || n == 0 || n > (1u << 24) || chain < 0) return -(int)hipErrorInvalidValue;
    switch (field) {
        case 0: return field_op<Fp<Bn254FrP>>(op, a, b, out, n, raw, chain);
        case 1: return field_op<Fp<Bn254FqP>>(op, a, b, out, n, raw, chain);
        case 2: return field_op<Fp<Bls381FrP>>(op, a, b, out, n, raw, chain);
        case 3: return field_op<Fp<Bls381FqP>>(op, a, b, out, n, raw, chain);
        case 4: return field_op<Fp2<Bn254FqP>>(op, a, b, out, n, raw, chain);
        case 5: return field_op<Fp2<Bls381FqP>>(op, a, b, out, n, raw, chain);
    }
    return -(int)hipErrorInvalidValue;
}
// curve: 0 bn254, 1 bls12-381; op: WaveOp; a, b: n x 12 Fq raw limbs; out: n x 13 Fq canonical (slot 12 is the padding);
// alias: 0 dst distinct, 1 dst == a, 2 dst == b (mul), 3 a == b == dst (mul)
int dshim_wave_op(int curve, int op, const void* a, const void* b, void* out, size_t n, int alias) {
    if (op < 0 || op >= W_NOPS || n == 0 || n > (1u << 20) || alias < 0 || alias > 3) return -(int)hipErrorInvalidValue;
    if (alias >= 2 && op != W_MUL) return -(int)hipErrorInvalidValue;
    if (alias != 0 && op == W_INV) return -(int)hipErrorInvalidValue;
    if (curve == 0) return wave_op<Bn254FqP>(op, a, b, out, n, alias);
    if (curve == 1) return wave_op<Bls381FqP>(op, a, b, out, n, alias);
    return -(int)hipErrorInvalidValue;
}
}
