// csr.cuh — the three CSR matrices of an R1CS on the device: their device view (CsrDev), the kernels that read them row-wise
// (k_spmv, csr_dot) or check them (k_csr_check), and the one way a call gets them there: host NULL check (csr_host_ok),
// staging of whatever is still on the host (R1csStage), structural validation with one read-back (r1cs_validate).
#pragma once
#include <algorithm>
#include "hk_internal.h"
#include "ntt.cuh"          // fr_load / fr_store

namespace hk {

struct CsrDev { const u64* row_ptr; const u32* col; const void* val; size_t n_rows, nnz; };

#if defined(__HIPCC__)

// <M_row, z> over the non-zeros [b, e) of the row (ark-groth16 `evaluate_constraint`); a coefficient equal to one skips its
// product.  Empty (b == e): zero.
template <class Fr>
__device__ __forceinline__ Fr csr_dot(const u32* __restrict__ col, const Fr* __restrict__ val, u64 b, u64 e, const Fr* __restrict__ z) {
    const Fr one = Fr::one();
    Fr acc = Fr::zero();
    HK_NOUNROLL for (u64 k = b; k < e; k++) {
        const Fr c = fr_load(&val[k]);
        Fr x = fr_load(&z[col[k]]);
        if (!(c == one)) x = Fr::mul(x, c);
        acc = Fr::add(acc, x);
    }
    return acc;
}

// out[row] = <M_row, z>, one lane per row of the WHOLE domain vector: rows past the matrix are written too - z[row - n_rows]
// for the n_copy instance rows of a ("a[start..end] = full_assignment[..num_inputs]"), zero for the rest - so the 3 m-element
// vectors need no memset before the transforms
template <class Fr>
__global__ void k_spmv(const u64* __restrict__ row_ptr, const u32* __restrict__ col, const Fr* __restrict__ val,
                       const Fr* __restrict__ z, Fr* __restrict__ out, u32 n_rows, u32 n_copy, u32 m) {
    u32 row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m) return;
    if (row >= n_rows) {
        fr_store(&out[row], row - n_rows < n_copy ? fr_load(&z[row - n_rows]) : Fr::zero());
        return;
    }
    fr_store(&out[row], csr_dot<Fr>(col, val, row_ptr[row], row_ptr[row + 1], z));
}

// Structural validation of a CSR matrix before any kernel indexes with it: row_ptr non-decreasing and within nnz,
// every column < n_cols.  *bad becomes non-zero on the first violation (grid-stride over rows and non-zeros).
template <int UNUSED>
__global__ void k_csr_check(const u64* __restrict__ row_ptr, const u32* __restrict__ col, u64 n_rows, u64 nnz,
                            u32 n_cols, u32* __restrict__ bad) {
    u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x, stride = (u64)gridDim.x * blockDim.x;
    u32 f = 0;
    for (u64 i = t; i < n_rows; i += stride) {
        u64 b = row_ptr[i], e = row_ptr[i + 1];
        if (b > e || e > nnz) f = 1;
    }
    for (u64 k = t; k < nnz; k += stride)
        if (col[k] >= n_cols) f = 2;
    if (t == 0 && (row_ptr[0] != 0 || row_ptr[n_rows] != nnz)) f = 3;
    if (f) atomicOr(bad, f);
}

#endif  // __HIPCC__

// the arrays a matrix must bring (on the host or on the device): checked before its first byte is read
static inline bool csr_host_ok(const hk_csr* M) { return M && M->row_ptr && (!M->nnz || (M->col && M->val_mont)); }

// HK_ERR_ARG unless the three (device-resident) matrices are structurally sound for n_cols variables: a malformed matrix
// must come back as an error (the reference returns an ark error), never as an out-of-bounds device read.  k_csr_check indexes
// with nothing it read, so all three run before the one read-back.  `flag`: one u32 of device scratch.  Synchronises `s`.
static hk_status r1cs_validate(hipStream_t s, const CsrDev D[3], size_t n_cols, u32* flag) {
    if (n_cols >= ((size_t)1 << 32)) return HK_ERR_ARG;
    HK_HIP(hipMemsetAsync(flag, 0, sizeof(u32), s));
    for (int k = 0; k < 3; k++) {
        size_t work = D[k].n_rows > D[k].nnz ? D[k].n_rows : D[k].nnz;
        u32 blocks = (u32)std::max<size_t>(std::min<size_t>((work + 255) / 256, 2048), 1);
        HK_LAUNCH((k_csr_check<0>), dim3(blocks), dim3(256), 0, s, D[k].row_ptr, D[k].col, (u64)D[k].n_rows,
                  (u64)D[k].nnz, (u32)n_cols, flag);
    }
    u32 h = 0;
    HK_HIP(hipMemcpyAsync(&h, flag, sizeof(u32), hipMemcpyDeviceToHost, s));
    HK_HIP(hipStreamSynchronize(s));
    return h ? HK_ERR_ARG : HK_OK;
}

// A call's matrices (each csr_host_ok) on their way to the device.  The constructor decides per array whether it is on the
// host - before the carve, which may not ask; carve() takes lane scratch for those arrays only, and the flag word; upload()
// copies them on the lane's stream, fills out[3] and validates it (r1cs_validate: HK_ERR_ARG, one synchronize).
struct R1csStage {
    const hk_csr* Ms[3];
    size_t n_cols = 0, fr_bytes = 0;
    bool host[3][3];
    const void* p[3][3];
    u32* flag = nullptr;

    // array j of matrix k: row_ptr, col, val_mont
    const void* src(int k, int j) const { return j == 0 ? (const void*)Ms[k]->row_ptr : j == 1 ? (const void*)Ms[k]->col : Ms[k]->val_mont; }
    size_t bytes(int k, int j) const { return j == 0 ? 8 * (Ms[k]->n_rows + 1) : (j == 1 ? 4 : fr_bytes) * Ms[k]->nnz; }
    R1csStage() = default;
    R1csStage(const hk_csr* A, const hk_csr* B, const hk_csr* C, size_t n_cols_, size_t fr_bytes_)
        : Ms{A, B, C}, n_cols(n_cols_), fr_bytes(fr_bytes_) {
        for (int k = 0; k < 3; k++)
            for (int j = 0; j < 3; j++) host[k][j] = bytes(k, j) && !is_device_ptr(src(k, j));
    }
    void carve(Carve& c) {
        for (int k = 0; k < 3; k++)
            for (int j = 0; j < 3; j++) p[k][j] = host[k][j] ? c.take(bytes(k, j)) : src(k, j);
        flag = c.n<u32>(1);
    }
    hk_status upload(Lane* L, CsrDev out[3]) const {
        for (int k = 0; k < 3; k++) {
            for (int j = 0; j < 3; j++)
                if (host[k][j]) HK_HIP(hipMemcpyAsync((void*)p[k][j], src(k, j), bytes(k, j), hipMemcpyHostToDevice, L->stream));
            out[k] = {(const u64*)p[k][0], (const u32*)p[k][1], p[k][2], Ms[k]->n_rows, Ms[k]->nnz};
        }
        return r1cs_validate(L->stream, out, n_cols, flag);
    }
};

}  // namespace hk
