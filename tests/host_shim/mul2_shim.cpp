// Host-compiled view of Fp::mul2 / mulsub / neg_operand of the PRODUCT's field.cuh (g++): the C++ fallback that every build
// without a fused block takes (HK_NO_ASM_MUL, host code), on canonical values.  Test-only; never part of libhekaton.
#include "../../hekaton_system_amd/csrc/field.cuh"
#include <string.h>
using namespace hk;

// op 0: mul2(a, b, c, d), 1: mulsub(a, b, c, d), 2: mul2(a, b, c, neg_operand(d))
template <class F>
static void run(int op, const unsigned char* a, const unsigned char* b, const unsigned char* c, const unsigned char* d,
                unsigned char* out, size_t n) {
    for (size_t i = 0; i < n; i++) {
        F x, y, z, w, r;
        memcpy(&x, a + i * sizeof(F), sizeof(F));
        memcpy(&y, b + i * sizeof(F), sizeof(F));
        memcpy(&z, c + i * sizeof(F), sizeof(F));
        memcpy(&w, d + i * sizeof(F), sizeof(F));
        if (op == 0) r = F::mul2(x, y, z, w);
        else if (op == 1) r = F::mulsub(x, y, z, w);
        else r = F::mul2(x, y, z, F::neg_operand(w));
        memcpy(out + i * sizeof(F), &r, sizeof(F));
    }
}

extern "C" {
// field: 0 bn254 Fr, 1 bn254 Fq, 2 bls Fr, 3 bls Fq; a..d, out: n elements of little-endian limbs.  0, or 1 for a bad argument
int shim_mul2(int field, int op, const unsigned char* a, const unsigned char* b, const unsigned char* c, const unsigned char* d,
              unsigned char* out, size_t n) {
    if (op < 0 || op > 2) return 1;
    switch (field) {
        case 0: run<Fp<Bn254FrP>>(op, a, b, c, d, out, n); return 0;
        case 1: run<Fp<Bn254FqP>>(op, a, b, c, d, out, n); return 0;
        case 2: run<Fp<Bls381FrP>>(op, a, b, c, d, out, n); return 0;
        case 3: run<Fp<Bls381FqP>>(op, a, b, c, d, out, n); return 0;
    }
    return 1;
}
}
