// Prints the sub-list plan rule of hekaton_system_amd/csrc/msm.cuh for tests/test_msm_sublist_cpu.py:
//   "plan <n> <c> <n_sub> <lanes> | <c W WP F B NB K n gshift chunk T0 n_levels kconst-hash> | <the same of the sub-list plan>"
//                                                          for every (n, c, n_sub) of argv: n scalars of 254 bits under window c
//   "rule <nq> <kept> <0|1>"                               msm_compact_rule at the shipped threshold 0.75
//   "rank <n_rank> : <idx ...> : <rank ...>"               msm_rank_table of the index list 0, 3, 6, ... then the last 4
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hekaton_system_amd/csrc/msm.cuh"

using namespace hk;

static void print_plan(const MsmPlan& p) {
    unsigned h = 0;
    for (int i = 0; i < 10; i++) h = h * 31u + p.kconst[i];
    printf(" | %u %u %u %u %u %u %u %u %u %u %u %u %u", p.c, p.W, p.WP, p.F, p.B, p.NB, p.K, p.n, p.gshift, p.chunk, p.T[0],
           p.n_levels, h);
}

int main(int argc, char** argv) {
    const unsigned lanes = 262144u;
    for (int a = 1; a + 2 < argc; a += 3) {
        unsigned n = (unsigned)atoi(argv[a]), c = (unsigned)atoi(argv[a + 1]), n_sub = (unsigned)atoi(argv[a + 2]);
        MsmPlan pz = msm_make_plan(n, 254, c, 1u, lanes);
        MsmPlan ps = msm_sub_plan(pz, n_sub, lanes);
        printf("plan %u %u %u %u", n, c, n_sub, lanes);
        print_plan(pz);
        print_plan(ps);
        printf("\n");
    }
    const size_t rules[][2] = {{4095, 0}, {4096, 0}, {4096, 3071}, {4096, 3072}, {4096, 3073}, {100000, 74999}, {100000, 75000}};
    for (auto& r : rules) printf("rule %zu %zu %d\n", r[0], r[1], msm_compact_rule(r[0], r[1], 0.75) ? 1 : 0);
    const size_t n_rank = 50;
    std::vector<u32> idx, rank(n_rank);
    for (u32 i = 0; i + 4 < n_rank; i += 3) idx.push_back(i);
    for (u32 e = 0; e < 4; e++) idx.push_back((u32)n_rank - 4 + e);
    msm_rank_table(idx.data(), idx.size(), rank.data(), n_rank);
    printf("rank %zu :", n_rank);
    for (u32 v : idx) printf(" %u", v);
    printf(" :");
    for (u32 v : rank) printf(" %u", v);
    printf("\n");
    return 0;
}
