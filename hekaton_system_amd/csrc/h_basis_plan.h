// h_basis_plan.h — the host-side bookkeeping of an evaluation-basis proving key (h_basis.cuh): which form a key takes, the
// transpose of the class's C matrix, and which of its columns are too long for one lane.  Plain C++, no HIP:
// tests/test_h_basis_cpu.py compiles it into a small host program.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace hk {

// A column of C with more entries than this is summed as an MSM over the bases G (msm_bases) instead of one lane's chain of
// scalar multiplications: the "one" variable of a circuit occurs in most rows.  The columns below it run side by side, so
// the light path takes as long as its longest chain (256 full-width products: ~0.4 s); a heavy column costs one m-point MSM.
// HK_H_BASIS_HEAVY_COL overrides (>= 1).
constexpr uint32_t HB_HEAVY_COL = 256;

inline uint32_t hb_heavy_threshold(const char* env) {
    long v = env ? atol(env) : 0;
    return v >= 1 ? (uint32_t)(v > 0x7fffffffL ? 0x7fffffffL : v) : HB_HEAVY_COL;
}
inline bool hb_col_is_heavy(uint64_t entries, uint32_t threshold) { return entries > threshold; }

// HK_H_BASIS as given -> whether a key with a QAP holds its H query in the coset's evaluation basis (the default) or in
// the coefficient basis ("coeff")
inline bool hb_eval_form(const char* env) { return !(env && strcmp(env, "coeff") == 0); }

// CSR -> CSC of an n_rows x n_cols matrix whose structure is sound (row_ptr non-decreasing from 0 to nnz, every column
// < n_cols: r1cs_validate): col_ptr[n_cols + 1]; row[e] and src[e] = the row and the CSR position of entry e, the entries of
// a column in ascending CSR position (so ascending row, duplicates kept).  false: a column or a row pointer out of range.
inline bool hb_transpose(const uint64_t* row_ptr, const uint32_t* col, size_t n_rows, size_t n_cols,
                         std::vector<uint64_t>& col_ptr, std::vector<uint32_t>& row, std::vector<uint32_t>& src) {
    const uint64_t nnz = row_ptr[n_rows];
    if (row_ptr[0] != 0 || nnz >= ((uint64_t)1 << 32)) return false;
    col_ptr.assign(n_cols + 1, 0);
    for (uint64_t e = 0; e < nnz; e++) {
        if (col[e] >= n_cols) return false;
        col_ptr[col[e] + 1]++;
    }
    for (size_t k = 0; k < n_cols; k++) col_ptr[k + 1] += col_ptr[k];
    row.assign(nnz, 0);
    src.assign(nnz, 0);
    std::vector<uint64_t> next(col_ptr.begin(), col_ptr.end() - 1);
    for (size_t r = 0; r < n_rows; r++) {
        if (row_ptr[r] > row_ptr[r + 1] || row_ptr[r + 1] > nnz) return false;
        for (uint64_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) {
            uint64_t at = next[col[e]]++;
            row[at] = (uint32_t)r;
            src[at] = (uint32_t)e;
        }
    }
    return true;
}

}  // namespace hk
