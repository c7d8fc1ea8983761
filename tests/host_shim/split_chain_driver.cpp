// Runs split_window_chain and jac_to_xyzz of hekaton_system_amd/csrc/endo.cuh on the host for tests/test_sweep_edges_cpu.py,
// which builds it with -fsanitize=address,undefined: the table accessors are the part the sanitizer watches.
//   split_chain_driver   reads lines "<group> <four affine points, hex>" from stdin (group: 0 bn254 G1, 1 bn254 G2,
//                        2 bls G1, 3 bls G2) and prints "<group> <inf 0|1> <lane> <|magnitude| * point, affine, hex>" for
//                        lane t = 0 .. 3, which multiplies point t (inf = 1: the point at infinity) by magnitude t of
//                        0x77..7 (ND nibbles), 0, 1, 8
// Every product runs twice: over a row of its own (SplitTabRow) and, the four lanes side by side as the lanes of a launch
// are, over one heap block of exactly SPLIT_TABLE x lanes entries strided by lane; results and tables must agree.
// The strided policy here is the driver's own (bounds-checked): it shows that the chain asks its table for entries
// 0 .. SPLIT_TABLE - 1 only and survives a layout other than a row.  The kernels' SplitTabStrided is device code; its own
// index arithmetic is covered by the GPU tests of k_points_mul_split, not here.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../hekaton_system_amd/csrc/ec.cuh"
#include "../../hekaton_system_amd/csrc/pairing.cuh"
#include "../../hekaton_system_amd/csrc/msm.cuh"
#include "../../hekaton_system_amd/csrc/endo.cuh"
using namespace hk;

// the layout of k_points_mul_split's table: entry k of lane t at tab[k lanes + t]
template <class F>
struct HostStrided {
    std::vector<Jac<F>>* tab;
    size_t lanes, t;
    Jac<F> ld(int k) const { return tab->at((size_t)k * lanes + t); }
    void st(int k, const Jac<F>& e) const { tab->at((size_t)k * lanes + t) = e; }
};

template <class F>
static int run(int group, const char* hex) {
    constexpr int ND = SplitDigits<F>::ND;
    constexpr size_t LANES = 4;
    if (strlen(hex) != 2 * LANES * sizeof(Affine<F>)) return 2;
    Affine<F> pts[LANES];
    for (size_t i = 0; i < sizeof(pts); i++) {
        unsigned v;
        if (sscanf(hex + 2 * i, "%2x", &v) != 1) return 2;
        ((unsigned char*)pts)[i] = (unsigned char)v;
    }
    u32 mags[LANES][6] = {{0}, {0}, {1}, {8}};
    for (int d = 0; d < ND; d++) mags[0][d >> 3] |= 7u << (4 * (d & 7));
    for (int inf = 0; inf < 2; inf++) {
        std::vector<Jac<F>> shared(SPLIT_TABLE * LANES);
        Affine<F> got[LANES];
        Jac<F> rows[LANES][SPLIT_TABLE];
        for (size_t t = 0; t < LANES; t++) {
            Affine<F> q = pts[t];
            if (inf) memset(&q, 0, sizeof(q));
            if (q.is_inf() != (inf == 1)) return 2;
            u32 m[6];
            for (int l = 0; l < 6; l++) m[l] = mags[t][l];
            split_bias<ND>(m);
            Jac<F> a, b;
            split_window_chain(q, m, SplitTabRow<F>{rows[t]}, a);
            split_window_chain(q, m, HostStrided<F>{&shared, LANES, t}, b);
            got[t] = ec_to_affine(jac_to_xyzz(a));
            Affine<F> other = ec_to_affine(jac_to_xyzz(b));
            if (memcmp(&got[t], &other, sizeof(other)) != 0) { fprintf(stderr, "group %d lane %zu: row and strided tables differ\n", group, t); return 1; }
        }
        // no lane wrote into another's entries: after all four ran, entry k of lane t is still its own (k + 1) P
        for (size_t t = 0; t < LANES && !inf; t++)
            for (int k = 0; k < SPLIT_TABLE; k++)
                if (memcmp(&shared[k * LANES + t], &rows[t][k], sizeof(Jac<F>)) != 0) { fprintf(stderr, "group %d lane %zu entry %d: overwritten\n", group, t, k); return 1; }
        for (size_t t = 0; t < LANES; t++) {
            printf("%d %d %zu ", group, inf, t);
            for (size_t i = 0; i < sizeof(got[t]); i++) printf("%02x", ((const unsigned char*)&got[t])[i]);
            printf("\n");
        }
    }
    return 0;
}

int main() {
    int group;
    static char hex[4096];
    while (scanf("%d %4095s", &group, hex) == 2) {
        int rc = 2;
        switch (group) {
            case 0: rc = run<Fp<Bn254FqP>>(group, hex); break;
            case 1: rc = run<Fp2<Bn254FqP>>(group, hex); break;
            case 2: rc = run<Fp<Bls381FqP>>(group, hex); break;
            case 3: rc = run<Fp2<Bls381FqP>>(group, hex); break;
        }
        if (rc) return rc;
    }
    return 0;
}
