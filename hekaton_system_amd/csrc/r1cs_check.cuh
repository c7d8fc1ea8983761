// r1cs_check.cuh — does a device-resident assignment satisfy its R1CS, and if not, where (hk_r1cs_check / hk_pk_r1cs_check,
// DESIGN.md section 4k): ark's `cs.is_satisfied()` / `which_is_unsatisfied()` (cp-groth16/src/lib.rs:158,291;
// distributed-prover/src/subcircuit_circuit.rs:311-399) on assignments that never exist on the host.
//
//   rows     k_r1cs_rows: one lane per (row, assignment): the three dot products <A_i,z>, <B_i,z>, <C_i,z> in one pass
//            (csr_dot), the test a b == c on canonical values, and the verdicts of 64 consecutive rows leave the wave as
//            one __ballot word that lane 0 stores into the assignment's bitmap of ceil(n_rows / 64) u64.  No m-element
//            vectors, no transforms.
//   compact  k_r1cs_compact: one workgroup per assignment walks its bitmap: popcounts, an exclusive scan in LDS
//            (wg_scan_u32), n_bad, first_bad and the failing rows of rank < cap, then the 0xFFFFFFFF padding.  The rank
//            of a failing row is the number of set bits in front of it: no atomics, nothing depends on an arrival order.
//   vals     k_r1cs_vals (only with bad_vals): one lane per (assignment, slot) recomputes the three sides of its listed row and
//            stores them canonical; empty slots store zeros.
#pragma once
#include "pk.cuh"
#include "csr.cuh"
#include "scan.cuh"

namespace hk {

constexpr u32 R1_WORDS_PER_LANE = 2;                                   // bitmap words per lane of a compact tile
constexpr u32 R1_TILE_WORDS = 256 * R1_WORDS_PER_LANE;                 // = 32 768 rows per tile
constexpr u32 R1_NONE = 0xffffffffu;

#if defined(__HIPCC__)

// bitmap[y words + w] bit l = row 64 w + l of assignment y fails.  Lanes past n_rows run empty rows and vote 0: every lane of
// a wave reaches the ballot.  grid = (ceil(n_rows / 256), batch).
template <class Fr>
__global__ void __launch_bounds__(256)
k_r1cs_rows(const u64* __restrict__ rpa, const u32* __restrict__ ca, const Fr* __restrict__ va,
            const u64* __restrict__ rpb, const u32* __restrict__ cb, const Fr* __restrict__ vb,
            const u64* __restrict__ rpc, const u32* __restrict__ cc, const Fr* __restrict__ vc,
            const Fr* __restrict__ z, size_t n_v, u32 n_rows, u32 words, u64* __restrict__ bitmap) {
    const u32 row = blockIdx.x * 256 + threadIdx.x;
    const bool valid = row < n_rows;
    const u32 rr = valid ? row : 0u;                                   // row_ptr has n_rows + 1 >= 1 entries
    const Fr* zb = z + (size_t)blockIdx.y * n_v;
    const Fr a = csr_dot<Fr>(ca, va, rpa[rr], valid ? rpa[rr + 1] : rpa[rr], zb);
    const Fr b = csr_dot<Fr>(cb, vb, rpb[rr], valid ? rpb[rr + 1] : rpb[rr], zb);
    const Fr c = csr_dot<Fr>(cc, vc, rpc[rr], valid ? rpc[rr + 1] : rpc[rr], zb);
    const bool bad = valid && !(Fr::mul(a, b) == c);                   // operator== compares canonical representatives
    const u64 m = __ballot(bad);
    const u32 w = row >> 6;
    if ((threadIdx.x & 63u) == 0 && w < words) bitmap[(size_t)blockIdx.y * words + w] = m;
}

struct R1Verdict { u32 n_bad, first_bad; };                            // hk_r1cs_verdict

// One workgroup per assignment.  A tile is R1_TILE_WORDS words, lane t owns R1_WORDS_PER_LANE consecutive words of it, so
// (tile, lane, word, bit) is row order.  rows (cap > 0): cap u32 per assignment.
template <int UNUSED>
__global__ void __launch_bounds__(256)
k_r1cs_compact(const u64* __restrict__ bitmap, u32 words, R1Verdict* __restrict__ verdicts, u32* __restrict__ rows, u32 cap) {
    __shared__ u32 s[256];
    const u32 tid = threadIdx.x;
    const u64* bm = bitmap + (size_t)blockIdx.x * words;
    u32* out = rows + (size_t)blockIdx.x * cap;
    u32 carry = 0;                                                     // failing rows in front of the tile: uniform
    HK_NOUNROLL for (u32 t0 = 0; t0 < words; t0 += R1_TILE_WORDS) {
        const u32 w0 = t0 + tid * R1_WORDS_PER_LANE;
        u64 v[R1_WORDS_PER_LANE];
        u32 sum = 0;
        HK_UNROLL for (u32 j = 0; j < R1_WORDS_PER_LANE; j++) {
            v[j] = w0 + j < words ? bm[w0 + j] : 0ull;
            sum += (u32)__popcll(v[j]);
        }
        u32 rank = carry + wg_scan_u32(s, tid, sum) - sum;
        const u32 total = s[255];
        HK_UNROLL for (u32 j = 0; j < R1_WORDS_PER_LANE; j++) {
            u64 m = v[j];
            const u32 lowest = (w0 + j) * 64 + (u32)__ffsll((unsigned long long)m) - 1;
            if (m && rank == 0) verdicts[blockIdx.x].first_bad = lowest;           // one lane of the whole walk
            const u32 pc = (u32)__popcll(m);
            HK_NOUNROLL for (u32 r = rank; m && r < cap; r++) {
                out[r] = (w0 + j) * 64 + (u32)__ffsll((unsigned long long)m) - 1;
                m &= m - 1;
            }
            rank += pc;
        }
        carry += total;
        __syncthreads();                                               // s is rewritten by the next tile
    }
    if (tid == 0) {
        verdicts[blockIdx.x].n_bad = carry;
        if (carry == 0) verdicts[blockIdx.x].first_bad = R1_NONE;
    }
    HK_NOUNROLL for (u64 r = (u64)carry + tid; r < cap; r += 256) out[r] = R1_NONE;
}

// vals[g] = (a, b, c) of row rows[g], g = assignment x cap + slot; zeros for an empty slot
template <class Fr>
__global__ void __launch_bounds__(256)
k_r1cs_vals(const u64* __restrict__ rpa, const u32* __restrict__ ca, const Fr* __restrict__ va,
            const u64* __restrict__ rpb, const u32* __restrict__ cb, const Fr* __restrict__ vb,
            const u64* __restrict__ rpc, const u32* __restrict__ cc, const Fr* __restrict__ vc,
            const Fr* __restrict__ z, size_t n_v, const u32* __restrict__ rows, u32 cap, u32 total, Fr* __restrict__ vals) {
    const u32 g = blockIdx.x * 256 + threadIdx.x;
    const bool live = g < total;
    const u32 gg = live ? g : 0u;
    const u32 row = rows[gg];
    const bool listed = live && row != R1_NONE;
    const u32 rr = listed ? row : 0u;
    const Fr* zb = z + (size_t)(gg / cap) * n_v;
    const Fr a = csr_dot<Fr>(ca, va, rpa[rr], listed ? rpa[rr + 1] : rpa[rr], zb);
    const Fr b = csr_dot<Fr>(cb, vb, rpb[rr], listed ? rpb[rr + 1] : rpb[rr], zb);
    const Fr c = csr_dot<Fr>(cc, vc, rpc[rr], listed ? rpc[rr + 1] : rpc[rr], zb);
    if (live) {                                                        // only the stores are guarded
        fr_store(&vals[(size_t)g * 3 + 0], a);
        fr_store(&vals[(size_t)g * 3 + 1], b);
        fr_store(&vals[(size_t)g * 3 + 2], c);
    }
}

#endif  // __HIPCC__

// The launches of one call over matrices that are on the device and sound for n_v columns.
template <class C>
struct R1csRun {
    typedef typename C::Fr Fr;
    // what the caller decides before the carve: sizes and which outputs live on the host
    size_t n_v, batch, cap;            // cap == 0: verdicts only
    u32 n_rows, words;
    bool want_vals, rows_host, vals_host;
    u64* bitmap;
    R1Verdict* vd;
    u32* rows_s;
    Fr* vals_s;

    R1csRun(size_t n_rows_, size_t n_v_, size_t batch_, uint32_t* bad_rows, void* bad_vals, size_t cap_)
        : n_v(n_v_), batch(batch_), cap(bad_rows ? cap_ : 0), n_rows((u32)n_rows_), words((u32)((n_rows_ + 63) / 64)) {
        want_vals = cap && bad_vals;
        rows_host = cap && !is_device_ptr(bad_rows);
        vals_host = want_vals && !is_device_ptr(bad_vals);
    }
    void carve(Carve& c) {
        bitmap = c.n<u64>(batch * words);
        vd = c.n<R1Verdict>(batch);
        rows_s = c.n<u32>(rows_host ? batch * cap : 0);
        vals_s = c.n<Fr>(vals_host ? batch * cap * 3 : 0);
    }
    hk_status run(hipStream_t s, const CsrDev* M, const Fr* z, hk_r1cs_verdict* verdicts, uint32_t* bad_rows, void* bad_vals) const {
        u32* rows_d = cap ? (rows_host ? rows_s : bad_rows) : nullptr;
        Fr* vals_d = want_vals ? (vals_host ? vals_s : (Fr*)bad_vals) : nullptr;
        for (size_t b0 = 0; b0 < batch && n_rows; b0 += 32768) {       // grid.y < 65 536
            const u32 nb = (u32)(batch - b0 < 32768 ? batch - b0 : 32768);
            HK_LAUNCH((k_r1cs_rows<Fr>), dim3((n_rows + 255) / 256, nb), dim3(256), 0, s, M[0].row_ptr, M[0].col,
                      (const Fr*)M[0].val, M[1].row_ptr, M[1].col, (const Fr*)M[1].val, M[2].row_ptr, M[2].col,
                      (const Fr*)M[2].val, z + b0 * n_v, n_v, n_rows, words, bitmap + b0 * words);
        }
        HK_LAUNCH((k_r1cs_compact<0>), dim3((u32)batch), dim3(256), 0, s, (const u64*)bitmap, words, vd, rows_d, (u32)cap);
        if (want_vals) {
            const u32 total = (u32)(batch * cap);
            HK_LAUNCH((k_r1cs_vals<Fr>), dim3((total + 255) / 256), dim3(256), 0, s, M[0].row_ptr, M[0].col, (const Fr*)M[0].val,
                      M[1].row_ptr, M[1].col, (const Fr*)M[1].val, M[2].row_ptr, M[2].col, (const Fr*)M[2].val, z, n_v,
                      (const u32*)rows_d, (u32)cap, total, vals_d);
        }
        static_assert(sizeof(R1Verdict) == sizeof(hk_r1cs_verdict), "hk_r1cs_verdict is two u32");
        HK_HIP(hipMemcpyAsync(verdicts, vd, batch * sizeof(R1Verdict), hipMemcpyDeviceToHost, s));
        if (rows_host) HK_HIP(hipMemcpyAsync(bad_rows, rows_s, batch * cap * 4, hipMemcpyDeviceToHost, s));
        if (vals_host) HK_HIP(hipMemcpyAsync(bad_vals, vals_s, batch * cap * 3 * sizeof(Fr), hipMemcpyDeviceToHost, s));
        return HK_OK;
    }
};

// what both entries refuse before anything else is looked at; *done: nothing to do
static inline hk_status r1cs_check_args(size_t n_rows, size_t n_v, size_t batch, const void* z, const hk_r1cs_verdict* verdicts,
                                        const uint32_t* bad_rows, const void* bad_vals, size_t cap, bool* done) {
    *done = false;
    if (n_rows >= ((size_t)1 << 32) || n_v >= ((size_t)1 << 32)) return HK_ERR_ARG;
    if (bad_vals && !bad_rows) return HK_ERR_ARG;
    if (batch == 0) { *done = true; return HK_OK; }
    if (!z || !verdicts) return HK_ERR_ARG;
    // lanes of k_r1cs_vals and workgroups of k_r1cs_compact are u32; a row of z has column 0
    const size_t lim = (size_t)1 << 31;
    if (n_v == 0 || batch >= lim || (bad_rows && (cap >= lim || batch * cap >= lim))) return HK_ERR_ARG;
    return HK_OK;
}

template <class C>
hk_status Ops<C>::r1cs_check(hk_ctx* ctx, const hk_csr* A, const hk_csr* B, const hk_csr* Cm, const void* z, size_t n_v, size_t batch,
                             hk_r1cs_verdict* verdicts, uint32_t* bad_rows, void* bad_vals, size_t cap) {
    if (A->n_rows != B->n_rows || A->n_rows != Cm->n_rows) return HK_ERR_ARG;
    if (!csr_host_ok(A) || !csr_host_ok(B) || !csr_host_ok(Cm)) return HK_ERR_ARG;
    bool done;
    HK_TRY(r1cs_check_args(A->n_rows, n_v, batch, z, verdicts, bad_rows, bad_vals, cap, &done));
    if (done) return HK_OK;
    R1csRun<C> run(A->n_rows, n_v, batch, bad_rows, bad_vals, cap);
    R1csStage stage(A, B, Cm, n_v, sizeof(Fr));
    Staged zin = staged(z, batch * n_v * sizeof(Fr));
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    HK_TRY(L->carve([&](Carve& c) { stage.carve(c); stage_carve(c, &zin, 1); run.carve(c); }));
    CsrDev D[3];
    HK_TRY(stage.upload(L, D));
    HK_TRY(stage_upload(L, &zin, 1));
    HK_TRY(run.run(L->stream, D, (const Fr*)zin.p, verdicts, bad_rows, bad_vals));
    return L->settle();
}

template <class C>
hk_status Ops<C>::pk_r1cs_check(hk_ctx* ctx, const hk_pk* h, const void* z, size_t n_v, size_t batch, hk_r1cs_verdict* verdicts,
                                uint32_t* bad_rows, void* bad_vals, size_t cap) {
    const PkImpl<C>* pk = (const PkImpl<C>*)h->impl;
    if (h->ctx != ctx || !pk->has_qap) return HK_ERR_ARG;
    if (n_v != pk->n_v) return HK_ERR_LEN;                             // as hk_prove
    bool done;
    HK_TRY(r1cs_check_args(pk->csr[0].n_rows, n_v, batch, z, verdicts, bad_rows, bad_vals, cap, &done));
    if (done) return HK_OK;
    R1csRun<C> run(pk->csr[0].n_rows, n_v, batch, bad_rows, bad_vals, cap);
    Staged zin = staged(z, batch * n_v * sizeof(Fr));
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    HK_TRY(L->carve([&](Carve& c) { stage_carve(c, &zin, 1); run.carve(c); }));
    HK_TRY(stage_upload(L, &zin, 1));
    HK_TRY(run.run(L->stream, pk->csr, (const Fr*)zin.p, verdicts, bad_rows, bad_vals));
    return L->settle();
}

}  // namespace hk
