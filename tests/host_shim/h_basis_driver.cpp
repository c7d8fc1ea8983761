// Runs the host helpers of hekaton_system_amd/csrc/h_basis_plan.h for tests/test_h_basis_cpu.py.
//   h_basis_driver transpose        reads "n_rows n_cols", n_rows + 1 row pointers and nnz columns from stdin; prints
//                                   "ok 0|1", then (ok) the n_cols + 1 column pointers, the nnz rows and the nnz CSR positions
//   h_basis_driver rule             prints "default <HB_HEAVY_COL>", then for every stdin line "<env or -> <entries>":
//                                   "<threshold> <heavy 0|1>"
//   h_basis_driver form <env or ->  prints "eval" or "coeff"
#include <cstdio>
#include <cstring>
#include <string>

#include "../../hekaton_system_amd/csrc/h_basis_plan.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (strcmp(argv[1], "transpose") == 0) {
        unsigned long long n_rows, n_cols, v;
        if (scanf("%llu %llu", &n_rows, &n_cols) != 2) return 2;
        std::vector<uint64_t> rp(n_rows + 1);
        for (auto& x : rp) { if (scanf("%llu", &v) != 1) return 2; x = v; }
        std::vector<uint32_t> col;
        while (scanf("%llu", &v) == 1) col.push_back((uint32_t)v);
        if (col.size() < rp[n_rows] && rp[n_rows] < (1ull << 32)) return 2;
        std::vector<uint64_t> col_ptr;
        std::vector<uint32_t> row, src;
        bool ok = hk::hb_transpose(rp.data(), col.data(), n_rows, n_cols, col_ptr, row, src);
        printf("ok %d\n", ok ? 1 : 0);
        if (!ok) return 0;
        for (auto x : col_ptr) printf("%llu ", (unsigned long long)x);
        printf("\n");
        for (auto x : row) printf("%u ", x);
        printf("\n");
        for (auto x : src) printf("%u ", x);
        printf("\n");
        return 0;
    }
    if (strcmp(argv[1], "rule") == 0) {
        printf("default %u\n", hk::HB_HEAVY_COL);
        char env[64];
        unsigned long long entries;
        while (scanf("%63s %llu", env, &entries) == 2) {
            uint32_t thr = hk::hb_heavy_threshold(strcmp(env, "-") == 0 ? nullptr : env);
            printf("%u %d\n", thr, hk::hb_col_is_heavy(entries, thr) ? 1 : 0);
        }
        return 0;
    }
    if (strcmp(argv[1], "form") == 0 && argc >= 3) {
        printf("%s\n", hk::hb_eval_form(strcmp(argv[2], "-") == 0 ? nullptr : argv[2]) ? "eval" : "coeff");
        return 0;
    }
    return 2;
}
