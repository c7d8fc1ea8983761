// Host-compiled view of the PRODUCT's class_sums.cuh (g++): the HK_HD chunk body of hk_class_power_sums run chunk by chunk
// over the host's own table, in the kernels' own shape - the same workgroups, the same stride over the grid, the same
// partials - with serial sums where the device sums in LDS.  Test-only; never part of libhekaton.
//
// Built twice by tests/test_agg_verify_cpu.py: as a shared object (the extern "C" entry, compared with the Python mirror) and,
// with -DCLASS_SUMS_MAIN, as a stand-alone program that prints one digest per case (run plain and under
// -fsanitize=address,undefined: same digests, clean exit).
#include "../../hekaton_system_amd/csrc/class_sums.cuh"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace hk;

// 0: sums written; 1: a class id >= n_classes, nothing written
template <class Fr>
static int class_sums(const void* x_mont, const u32* class_of, size_t n, size_t n_classes, void* sums_out) {
    Fr x, tab[AQ_PW_LEN];
    memcpy(&x, x_mont, sizeof(Fr));
    aq_powers_table<Fr>(x, tab);
    const u32 n_chunks = (u32)((n + AQ_CHUNK - 1) / AQ_CHUNK), n_wgs = cs_workgroups(n_chunks);
    const u32 n_groups = (u32)((n_classes + CS_GROUP - 1) / CS_GROUP);
    u32 nbits = 0;
    while (((u64)1 << nbits) < n_chunks) nbits++;
    std::vector<Fr> part((size_t)n_groups * n_wgs * CS_GROUP, Fr::zero());
    bool ok = true;
    // k_cs_chunks: grid (n_wgs, n_groups)
    for (u32 g = 0; g < n_groups; g++)
        for (u32 b = 0; b < n_wgs; b++)
            for (u32 tid = 0; tid < CS_WG; tid++) {
                CsAcc<Fr> acc;
                cs_acc_zero<Fr>(acc);
                for (u32 t = b * CS_WG + tid; t < n_chunks; t += n_wgs * CS_WG)
                    ok = cs_chunk<Fr>(tab, class_of, n, (u32)n_classes, t, nbits, g, acc) && ok;
                Fr* out = part.data() + cs_part_at(g, n_wgs, b);
                for (u32 k = 0; k < CS_GROUP; k++) out[k] = Fr::add(out[k], acc.a[k]);
            }
    if (!ok) return 1;
    // k_cs_reduce: one workgroup per class
    for (u32 c = 0; c < n_classes; c++) {
        Fr acc = Fr::zero();
        for (u32 b = 0; b < n_wgs; b++) acc = Fr::add(acc, part[cs_part_at(c / CS_GROUP, n_wgs, b) + c % CS_GROUP]);
        ((Fr*)sums_out)[c] = acc;
    }
    return 0;
}

extern "C" {
// curve: 0 bn254, 1 bls12-381; the arguments of hk_class_power_sums, host buffers only
int shim_class_power_sums(int curve, const void* x_mont, const u32* class_of, size_t n, size_t n_classes, void* sums_out) {
    return curve == 0 ? class_sums<Fp<Bn254FrP>>(x_mont, class_of, n, n_classes, sums_out)
                      : class_sums<Fp<Bls381FrP>>(x_mont, class_of, n, n_classes, sums_out);
}
}

#ifdef CLASS_SUMS_MAIN
static u64 fnv(const void* p, size_t n, u64 h = 1469598103934665603ull) {
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}
// field elements from a seed: Montgomery products and sums of what came before stay in [0, p)
template <class Fr>
static Fr next_value(Fr& state) {
    state = Fr::add(Fr::mul(state, state), Fr::r2());
    return state;
}
template <class Fr>
static void run_cases(const char* name) {
    Fr st = Fr::r2();
    const size_t shapes[][2] = {{1, 1}, {7, 2}, {8, 5}, {9, 8}, {2047, 9}, {2049, 1024}, {4097, 17}, {65537, 5}};
    u32 lcg = 12345;
    for (auto& sh : shapes) {
        const size_t n = sh[0], nc = sh[1];
        const Fr x = next_value(st);
        std::vector<u32> cls(n);                                            // exactly n: a read past the end is reported
        for (size_t i = 0; i < n; i++) {
            lcg = lcg * 1664525u + 1013904223u;
            cls[i] = (lcg >> 8) % (u32)nc;
        }
        std::vector<Fr> out(nc);                                            // exactly n_classes
        const int rc = class_sums<Fr>(&x, cls.data(), n, nc, out.data());
        printf("%s sums n=%zu classes=%zu rc=%d %016llx\n", name, n, nc, rc, (unsigned long long)fnv(out.data(), nc * sizeof(Fr)));
        // the same with the last id out of range: refused, the output as it was
        cls[n - 1] = (u32)nc;
        std::vector<Fr> keep(out);
        const int rc2 = class_sums<Fr>(&x, cls.data(), n, nc, out.data());
        printf("%s refused n=%zu classes=%zu rc=%d same=%d\n", name, n, nc, rc2, (int)!memcmp(keep.data(), out.data(), nc * sizeof(Fr)));
    }
}
int main() {
    run_cases<Fp<Bn254FrP>>("bn254");
    run_cases<Fp<Bls381FrP>>("bls12_381");
    return 0;
}
#endif
