// Device-compiled view of the PRODUCT's Fr transform layer, launch by launch (hipcc, gfx950): the table kernels and
// pow_from_tables of ntt.cuh, ONE k_ntt_pass4 launch with every argument the caller's, k_scale_pow, k_bitrev, k_mul_pointwise,
// k_spmv of csr.cuh and scan_u32 of scan.cuh.  NttHost::passes / QapHost::run (ntt_host.cuh) chain them with stages, tiles,
// batch and epilogue they derive themselves; here the caller picks lo, nst, cols_bits, the block size, the stride, the mask
// and the data, so that every seam is compared with integers alone (tests/ntt_ref.py).  Test-only; never part of libhekaton.
//
// Built twice by the Makefile next to it: as shipped, and with -DHK_NO_ASM_MUL.  The kernels are the product's own templates
// under their product names; what keeps this library's launches on its own code objects is the -Bsymbolic link of the
// Makefile and a loader that does not merge the libraries' symbols (ctypes: RTLD_LOCAL), as for ec_dev_shim.hip.
// k_pow_from_tables_op exists here only and carries the variant in its name.
//
// All Fr operands are canonical Montgomery bytes, as the kernels keep them in memory.  Every HIP status is returned to the
// caller; the shim allocates and frees its own buffers and never touches an hk_ctx.  A shape outside a kernel's contract is
// refused on the host with SHIM_REFUSED and never launched.
#include "../../hekaton_system_amd/csrc/csr.cuh"
#include "../../hekaton_system_amd/csrc/ntt.cuh"
#include "../../hekaton_system_amd/csrc/scan.cuh"
#include "shim_common.cuh"

constexpr unsigned MAX_LOGN = 22;            // largest vector an entry point takes (64 MiB of Fr)
constexpr unsigned SCAN_PAD = 64;            // u32 the caller's `out` of dshim_scan_u32 holds past n

// out[i] = g^js[i] from the three-level tables, one lane per j
template <class Fr, int V>
__global__ void k_pow_from_tables_op(const Fr* __restrict__ pw, const u32* __restrict__ js, u32 n, u32 logn, Fr* __restrict__ out) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fr_store(&out[i], pow_from_tables(pw, js[i], logn));
}

// ---- host side ---------------------------------------------------------------------------------------------------
namespace {

// the launches of NttHost::ensure for one direction
template <class Fr>
int ntt_tables(unsigned L, const void* sq, void* out) {
    size_t half = (size_t)1 << (L - 1), full = (size_t)1 << L;
    DevBufs d;
    Fr *d_sq, *tmp, *tf;
    SHIM_GET(&d_sq, sizeof(Fr) * 32, sq, sizeof(Fr) * L);
    SHIM_GET(&tmp, sizeof(Fr) * half, nullptr);
    SHIM_GET(&tf, sizeof(Fr) * full, nullptr);
    u32 blocks = (u32)((half + 255) / 256), blocks_full = (u32)((full + 255) / 256);
    hipLaunchKernelGGL((k_pow_table<Fr>), dim3(blocks), dim3(256), 0, 0, tmp, d_sq, (u32)half, L - 1);
    hipLaunchKernelGGL((k_stage_tables<Fr>), dim3(blocks_full), dim3(256), 0, 0, tf, tmp, L);
    return finish(out, tf, sizeof(Fr) * (full - 1));
}

template <class Fr>
int pow_table(const void* sq, unsigned count, unsigned nbits, void* out) {
    DevBufs d;
    Fr *d_sq, *tw;
    SHIM_GET(&d_sq, sizeof(Fr) * 32, sq, sizeof(Fr) * nbits);
    SHIM_GET(&tw, sizeof(Fr) * count, nullptr);
    hipLaunchKernelGGL((k_pow_table<Fr>), dim3((count + 255) / 256), dim3(256), 0, 0, tw, d_sq, (u32)count, (u32)nbits);
    return finish(out, tw, sizeof(Fr) * count);
}

template <class Fr>
int pow_from(const void* pw, const unsigned* js, unsigned n, unsigned logn, void* out) {
    DevBufs d;
    Fr *d_pw, *d_out;
    u32* d_js;
    SHIM_GET(&d_pw, sizeof(Fr) * 3 * POW_TABLE_SIZE, pw);
    SHIM_GET(&d_js, sizeof(u32) * n, js);
    SHIM_GET(&d_out, sizeof(Fr) * n, nullptr);
    hipLaunchKernelGGL((k_pow_from_tables_op<Fr, VARIANT>), dim3((n + 63) / 64), dim3(64), 0, 0, (const Fr*)d_pw, (const u32*)d_js,
                       (u32)n, (u32)logn, d_out);
    return finish(out, d_out, sizeof(Fr) * n);
}

// one launch of k_ntt_pass4 with the grid and LDS of NttHost::passes
template <class Fr>
int ntt_pass(int dit, void* data, size_t stride, unsigned batch, const void* tws, unsigned logn, unsigned lo, unsigned nst,
             unsigned cols_bits, unsigned threads, int post, unsigned npost, const void* scale, const void* pw, const void* sub,
             const void* kc) {
    size_t n = (size_t)1 << logn, total = (size_t)batch * stride;
    DevBufs d;
    Fr *d_data, *d_tws, *d_pw = nullptr, *d_sub = nullptr;
    SHIM_GET(&d_data, sizeof(Fr) * total, data);
    SHIM_GET(&d_tws, sizeof(Fr) * n, tws, sizeof(Fr) * (n - 1));
    if (pw) SHIM_GET(&d_pw, sizeof(Fr) * 3 * POW_TABLE_SIZE, pw);
    if (sub) SHIM_GET(&d_sub, sizeof(Fr) * n, sub);
    Fr sc = Fr::one(), k = Fr::one();
    if (scale) memcpy(&sc, scale, sizeof(Fr));
    if (kc) memcpy(&k, kc, sizeof(Fr));
    u32 tile_log = nst + cols_bits;
    dim3 grid(1u << (logn - tile_log), batch);
    size_t lds = sizeof(Fr) << tile_log;
    if (dit)
        hipLaunchKernelGGL((k_ntt_pass4<Fr, 1>), grid, dim3(threads), lds, 0, d_data, stride, (const Fr*)d_tws, (u32)logn, (u32)lo,
                           (u32)nst, (u32)cols_bits, post, (u32)npost, sc, (const Fr*)d_pw, (const Fr*)d_sub, k);
    else
        hipLaunchKernelGGL((k_ntt_pass4<Fr, 0>), grid, dim3(threads), lds, 0, d_data, stride, (const Fr*)d_tws, (u32)logn, (u32)lo,
                           (u32)nst, (u32)cols_bits, post, (u32)npost, sc, (const Fr*)d_pw, (const Fr*)d_sub, k);
    return finish(data, d_data, sizeof(Fr) * total);
}

template <class Fr>
int scale_pow(void* data, size_t stride, unsigned batch, const void* pw, const void* scale, unsigned logn, int bitrev_index,
              int use_pow) {
    size_t n = (size_t)1 << logn, total = (size_t)batch * stride;
    DevBufs d;
    Fr *d_data, *d_pw = nullptr;
    SHIM_GET(&d_data, sizeof(Fr) * total, data);
    if (pw) SHIM_GET(&d_pw, sizeof(Fr) * 3 * POW_TABLE_SIZE, pw);
    Fr sc;
    memcpy(&sc, scale, sizeof(Fr));
    hipLaunchKernelGGL((k_scale_pow<Fr>), dim3((u32)((n + 255) / 256), batch), dim3(256), 0, 0, d_data, stride, (const Fr*)d_pw, sc,
                       (u32)logn, bitrev_index, use_pow);                                       // as NttHost::scale
    return finish(data, d_data, sizeof(Fr) * total);
}

template <class Fr>
int bitrev(void* data, unsigned logn) {
    size_t n = (size_t)1 << logn;
    DevBufs d;
    Fr* d_data;
    SHIM_GET(&d_data, sizeof(Fr) * n, data);
    hipLaunchKernelGGL((k_bitrev<Fr>), dim3((u32)((n + 255) / 256)), dim3(256), 0, 0, d_data, (u32)logn);   // as NttHost::bitrev
    return finish(data, d_data, sizeof(Fr) * n);
}

template <class Fr>
int mul_pointwise(void* a, const void* b, size_t m) {
    DevBufs d;
    Fr *da, *db;
    SHIM_GET(&da, sizeof(Fr) * m, a);
    SHIM_GET(&db, sizeof(Fr) * m, b);
    hipLaunchKernelGGL((k_mul_pointwise<Fr>), dim3((u32)((m + 255) / 256)), dim3(256), 0, 0, da, (const Fr*)db, m);   // as QapHost::run
    return finish(a, da, sizeof(Fr) * m);
}

template <class Fr>
int spmv(const unsigned long long* row_ptr, const unsigned* col, const void* val, size_t nnz, const void* z, size_t n_z, void* out,
         unsigned n_rows, unsigned n_copy, unsigned m) {
    DevBufs d;
    u64* d_rp;
    u32* d_col;
    Fr *d_val, *d_z, *d_out;
    SHIM_GET(&d_rp, sizeof(u64) * ((size_t)n_rows + 1), row_ptr);
    SHIM_GET(&d_col, sizeof(u32) * nnz, col);
    SHIM_GET(&d_val, sizeof(Fr) * nnz, val);
    SHIM_GET(&d_z, sizeof(Fr) * n_z, z);
    SHIM_GET(&d_out, sizeof(Fr) * m, out);
    hipLaunchKernelGGL((k_spmv<Fr>), dim3((u32)(((size_t)m + 255) / 256)), dim3(256), 0, 0, (const u64*)d_rp, (const u32*)d_col,
                       (const Fr*)d_val, (const Fr*)d_z, d_out, (u32)n_rows, (u32)n_copy, (u32)m);     // as QapHost::run
    return finish(out, d_out, sizeof(Fr) * m);
}

}  // namespace

#define BY_CURVE(curve, fn, ...)                                        \
    do {                                                                \
        if ((curve) == 0) return fn<Fp<Bn254FrP>>(__VA_ARGS__);         \
        if ((curve) == 1) return fn<Fp<Bls381FrP>>(__VA_ARGS__);        \
        return SHIM_REFUSED;                                       \
    } while (0)

extern "C" {
int dshim_ntt_uses_asm(void) { return VARIANT; }
unsigned dshim_ntt_scan_pad(void) { return SCAN_PAD; }

// Every entry point: curve 0 BN254 Fr, 1 BLS12-381 Fr; returns 0, minus the first failing hipError_t, SHIM_REFUSED for
// arguments outside the kernels' contract (nothing launched), or (dshim_scan_u32) the product's hk_status.
//
// sq: log_table entries sq[k] = w^(2^k) -> out: the 2^log_table - 1 stage-table entries (k_pow_table over 2^(log_table - 1)
// entries, then k_stage_tables)
int dshim_ntt_tables(int curve, unsigned log_table, const void* sq, void* out) {
    if (log_table < 1 || log_table > MAX_LOGN || !sq || !out) return SHIM_REFUSED;
    BY_CURVE(curve, ntt_tables, log_table, sq, out);
}
// sq: nbits entries -> out[i] = prod of sq[k] over the set bits k of i, i < count
int dshim_pow_table(int curve, const void* sq, unsigned count, unsigned nbits, void* out) {
    if (count < 1 || count > (1u << MAX_LOGN) || nbits > 32 || !sq || !out) return SHIM_REFUSED;
    BY_CURVE(curve, pow_table, sq, count, nbits, out);
}
// pw: 3 x POW_TABLE_SIZE entries; js: n exponents below 2^logn -> out[i] = pow_from_tables(pw, js[i], logn)
int dshim_pow_from_tables(int curve, const void* pw, const unsigned* js, unsigned n, unsigned logn, void* out) {
    if (n < 1 || n > (1u << 16) || logn > 32 || !pw || !js || !out) return SHIM_REFUSED;
    for (unsigned i = 0; i < n; i++)
        if (logn < 32 && (js[i] >> logn)) return SHIM_REFUSED;
    BY_CURVE(curve, pow_from, pw, js, n, logn, out);
}
// One k_ntt_pass4<Fr, dit> launch, grid (2^(logn - nst - cols_bits), batch), LDS 32 << (nst + cols_bits), `threads` lanes a
// block.  data: batch * stride elements (vector v at v * stride), transformed in place; tws: the 2^logn - 1 stage-table entries;
// scale, kc: one element each, or null for one; pw: 3 x POW_TABLE_SIZE entries (needed for post & 2); sub: 2^logn elements
// (needed for post & 4).
int dshim_ntt_pass(int curve, int dit, void* data, size_t stride, unsigned batch, const void* tws, unsigned logn, unsigned lo,
                   unsigned nst, unsigned cols_bits, unsigned threads, int post, unsigned npost, const void* scale, const void* pw,
                   const void* sub, const void* kc) {
    if (logn < 1 || logn > MAX_LOGN || nst < 1 || cols_bits > lo || nst + cols_bits > (unsigned)NTT_TILE_LOG || lo + nst > logn)
        return SHIM_REFUSED;
    if (threads < 1 || threads > (unsigned)NTT_THREADS || batch < 1 || batch > 16 || stride < ((size_t)1 << logn) ||
        stride > ((size_t)1 << (MAX_LOGN + 1)) || !data || !tws || post < 0 || post > 7)
        return SHIM_REFUSED;
    if (((post & 2) && !pw) || ((post & 4) && !sub) || dit < 0 || dit > 1) return SHIM_REFUSED;
    BY_CURVE(curve, ntt_pass, dit, data, stride, batch, tws, logn, lo, nst, cols_bits, threads, post, npost, scale, pw, sub, kc);
}
// data: batch * stride elements; x[pos] *= scale * g^idx, idx = pos or bitrev(pos), only `scale` without use_pow
int dshim_scale_pow(int curve, void* data, size_t stride, unsigned batch, const void* pw, const void* scale, unsigned logn,
                    int bitrev_index, int use_pow) {
    if (logn > MAX_LOGN || batch < 1 || batch > 16 || stride < ((size_t)1 << logn) || stride > ((size_t)1 << (MAX_LOGN + 1)) ||
        !data || !scale || (use_pow && !pw))
        return SHIM_REFUSED;
    BY_CURVE(curve, scale_pow, data, stride, batch, pw, scale, logn, bitrev_index, use_pow);
}
int dshim_bitrev(int curve, void* data, unsigned logn) {
    if (logn > MAX_LOGN || !data) return SHIM_REFUSED;
    BY_CURVE(curve, bitrev, data, logn);
}
// a[i] *= b[i], i < m
int dshim_mul_pointwise(int curve, void* a, const void* b, size_t m) {
    if (m < 1 || m > ((size_t)1 << MAX_LOGN) || !a || !b) return SHIM_REFUSED;
    BY_CURVE(curve, mul_pointwise, a, b, m);
}
// k_spmv over the m rows of a domain vector: the n_rows rows of the CSR matrix (row_ptr: n_rows + 1, col / val: nnz; z: n_z
// elements), then z[0 .. n_copy), then zeros.  out: m elements, uploaded as they are and read back.  The matrix is checked
// on the host as r1cs_validate checks it on the device.
int dshim_spmv(int curve, const unsigned long long* row_ptr, const unsigned* col, const void* val, size_t nnz, const void* z,
               size_t n_z, void* out, unsigned n_rows, unsigned n_copy, unsigned m) {
    if (!row_ptr || !z || !out || (nnz && (!col || !val)) || m < 1 || m > (1u << MAX_LOGN) || n_rows > m || n_z < 1 ||
        n_z > (1u << MAX_LOGN) || n_copy > n_z || nnz > ((size_t)1 << MAX_LOGN))
        return SHIM_REFUSED;
    if (row_ptr[0] != 0 || row_ptr[n_rows] != nnz) return SHIM_REFUSED;
    for (unsigned i = 0; i < n_rows; i++)
        if (row_ptr[i] > row_ptr[i + 1] || row_ptr[i + 1] > nnz) return SHIM_REFUSED;
    for (size_t k = 0; k < nnz; k++)
        if (col[k] >= n_z) return SHIM_REFUSED;
    BY_CURVE(curve, spmv, row_ptr, col, val, nnz, z, n_z, out, n_rows, n_copy, m);
}
// the product's scan_u32 with `tops` of scan_u32_tops_len(n).  in: n counts; out: n + dshim_ntt_scan_pad() u32, uploaded as
// they are and read back, so that the caller sees what was written past n
int dshim_scan_u32(const unsigned* in, unsigned* out, unsigned n) {
    if ((n && !in) || !out || n > (1u << 24)) return SHIM_REFUSED;
    DevBufs d;
    u32 *d_in, *d_out, *d_tops;
    size_t cap = (size_t)n + SCAN_PAD;
    SHIM_GET(&d_in, sizeof(u32) * n, in);
    SHIM_GET(&d_out, sizeof(u32) * cap, out);
    SHIM_GET(&d_tops, sizeof(u32) * scan_u32_tops_len(n), nullptr);
    hk_status st = scan_u32(0, (const u32*)d_in, d_out, d_tops, (u32)n);
    if (st != HK_OK) return (int)st;
    return finish(out, d_out, sizeof(u32) * cap);
}
}
