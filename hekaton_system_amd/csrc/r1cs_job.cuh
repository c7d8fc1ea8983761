// r1cs_job.cuh — the partitioned R1CS job on the device (hk_r1cs_job_trace / hk_r1cs_job_witness): the
// time-ordered ROM trace of distributed-prover/src/partitioned_r1cs_circuit.rs:182-220 `get_portal_subtraces` and the imported
// wires of a subcircuit's assignment (:129-149), both gathered from the job's witness block where it lies.  The job is
// hekaton_system_amd/r1cs_circuit.py `PartitionedR1csJob`; the tables of hk_r1cs_job_desc are its `tables()`.
//
// A transaction's witness block is the P partitions' witnesses back to back; transaction g reads block g * tx_stride (block 0
// when tx_stride == 0).  S = slot_offsets[P] portal slots per transaction, partition-major and in time order inside a
// partition (its owned `set`s, its borrowed `get`s, the dummy `set` of a one-partition job), so entry e of the flattened trace
// is slot e % S of transaction e / S:
//     addr = 1 + (e / S) * sets_per_tx + slot_rank[e % S]        val = block[slot_src[e % S]], or 0 for HK_R1CS_SRC_ZERO
//
//   k_rj_trace   one lane per Fr of the trace, Fr fastest: even lanes make an address (an integer below 2^32 into Montgomery
//                form with one field multiplication), odd lanes copy a value.  A wave stores 64 consecutive Fr.
//   k_rj_body    one lane per (row, column) over column 0 and the body columns, a row per blockIdx.y: a wave reads 64 consecutive
//                Fr of one witness and stores 64 consecutive Fr of one row (the first lane of a row stores the constant 1).
#pragma once
#include "curve_ops_impl.cuh"
#include "job_args.h"
#include "poseidon.cuh"         // fr_select

namespace hk {

constexpr u32 RJ_GRID_ROWS = 65535;     // rows of one k_rj_body launch: the y extent of a grid

#if defined(__HIPCC__)

// every index is 32 bits wide (the call refuses 2^31 entries): no 64-bit division, whose expansion joins a 32-bit and a 64-bit
// path
template <class Fr>
__global__ void __launch_bounds__(256)
k_rj_trace(const Fr* __restrict__ wit, const u32* __restrict__ rank, const u32* __restrict__ src, u32 S, u32 sets_per_tx,
           u32 tx_stride, u32 n_fr, Fr* __restrict__ out) {
    const u32 t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_fr) return;
    const u32 e = t >> 1, g = e / S, s = e - g * S;
    const bool is_val = t & 1u;
    const u32 k = src[s];
    // both lanes of an entry load: the address lane reads wire 0 of its block and drops it
    const Fr v = fr_load(&wit[(u64)g * tx_stride + (is_val && k != HK_R1CS_SRC_ZERO ? k : 0u)]);
    Fr a = Fr::zero();
    a.v[0] = 1u + g * sets_per_tx + rank[s];                       // below 2^32: the call checked 1 + T O
    a = Fr::to_mont(a);
    fr_store(&out[t], fr_select(is_val, fr_select(k != HK_R1CS_SRC_ZERO, v, Fr::zero()), a));
}

// row blockIdx.y starts at wire 0 of its subcircuit's witness, wit + base[row]; lane c of the row: c == 0 -> column 0 <- 1,
// else column body_col0 + c - 1 <- wire c.  The grid's y is the row: no division.
template <class Fr>
__global__ void __launch_bounds__(256)
k_rj_body(const Fr* __restrict__ wit, const u64* __restrict__ base, u32 per, size_t n_v, size_t body_col0, Fr* __restrict__ z) {
    const u32 c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= per) return;
    Fr* row = z + (size_t)b * n_v;
    const Fr x = fr_select(c != 0, fr_load(&wit[base[b] + c]), Fr::one());
    fr_store(c ? &row[body_col0 + c - 1] : &row[0], x);
}

#endif  // __HIPCC__

// what both calls check of the descriptor; *n_wit: Fr of the whole witness buffer
static inline hk_status rj_check(const hk_r1cs_job_desc* d, size_t* n_wit) {
    if (!d->slot_offsets || !d->slot_rank || !d->slot_src || !d->witness_mont) return HK_ERR_ARG;
    const size_t P = d->n_parts, T = d->n_txs;
    if (P == 0 || T == 0 || P * T > ((size_t)1 << 24)) return HK_ERR_ARG;                      // as hk_exec_tree's n_sub
    if (d->tx_len == 0) return HK_ERR_ARG;                                                     // a block holds wire 0 at least
    HK_TRY(offsets_check(d->slot_offsets, P));
    const size_t S = d->slot_offsets[P];
    for (size_t s = 0; s < S; s++) {
        if (d->slot_rank[s] >= d->sets_per_tx) return HK_ERR_ARG;
        if (d->slot_src[s] != HK_R1CS_SRC_ZERO && d->slot_src[s] >= d->tx_len) return HK_ERR_ARG;
    }
    if (1 + (u64)T * d->sets_per_tx >= ((u64)1 << 32)) return HK_ERR_ARG;                      // an address is a u32 on the device
    if ((u64)T * S >= ((u64)1 << 31)) return HK_ERR_ARG;                                       // as hk_trace_sort's n_entries
    if (d->tx_stride != 0 && d->tx_stride < d->tx_len) return HK_ERR_ARG;                      // blocks would overlap
    *n_wit = (T - 1) * (size_t)d->tx_stride + d->tx_len;
    return HK_OK;
}

template <class C>
hk_status Ops<C>::r1cs_job_trace(hk_ctx* ctx, const hk_r1cs_job_desc* d, void* time_entries_out) {
    size_t n_wit;
    HK_TRY(rj_check(d, &n_wit));
    const size_t S = d->slot_offsets[d->n_parts], n_fr = 2 * S * d->n_txs, fr = sizeof(Fr);
    if (n_fr == 0) return HK_OK;
    if (!time_entries_out || bufs_overlap(time_entries_out, n_fr * fr, d->witness_mont, n_wit * fr)) return HK_ERR_ARG;
    Staged in = staged(d->witness_mont, n_wit * fr), out = staged(time_entries_out, n_fr * fr);
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    u32 *rank_d, *src_d;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, &in, 1);
        rank_d = c.n<u32>(S);
        src_d = c.n<u32>(S);
        stage_carve(c, &out, 1);
    }));
    hipStream_t s = L->stream;
    const void* wit = in.p;
    Fr* out_d = (Fr*)out.p;
    HK_TRY(stage_upload(L, &in, 1));
    HK_HIP(hipMemcpyAsync(rank_d, d->slot_rank, 4 * S, hipMemcpyHostToDevice, s));
    HK_HIP(hipMemcpyAsync(src_d, d->slot_src, 4 * S, hipMemcpyHostToDevice, s));
    HK_LAUNCH((k_rj_trace<Fr>), dim3((u32)((n_fr + 255) / 256)), dim3(256), 0, s, (const Fr*)wit, (const u32*)rank_d,
              (const u32*)src_d, (u32)S, d->sets_per_tx, d->tx_stride, (u32)n_fr, out_d);
    HK_TRY(stage_download(L, &out, 1));
    return L->settle();
}

template <class C>
hk_status Ops<C>::r1cs_job_witness(hk_ctx* ctx, const hk_r1cs_job_desc* d, const uint32_t* sub_index, size_t batch, size_t n_v,
                                   size_t body_col0, void* z_out) {
    size_t n_wit;
    HK_TRY(rj_check(d, &n_wit));
    if (!d->wit_offsets || !d->body_len || (batch && (!sub_index || !z_out))) return HK_ERR_ARG;
    const size_t P = d->n_parts, T = d->n_txs, fr = sizeof(Fr);
    // partition p's witness is [wit_offsets[p], wit_offsets[p + 1]) of a block and holds wire 0 and its body_len[p] body wires
    if (d->wit_offsets[0] != 0 || d->wit_offsets[P] != d->tx_len) return HK_ERR_ARG;
    for (size_t p = 0; p < P; p++)
        if (d->wit_offsets[p + 1] <= d->wit_offsets[p] || d->body_len[p] >= d->wit_offsets[p + 1] - d->wit_offsets[p])
            return HK_ERR_ARG;
    if (batch >= (1u << 20) || n_v >= ((size_t)1 << 31) || batch * n_v >= ((size_t)1 << 38)) return HK_ERR_ARG;
    std::vector<u64> base(batch);                          // outlives the lane's copy
    for (size_t b = 0; b < batch; b++) {
        const size_t i = sub_index[b];
        if (i >= P * T || i % P != sub_index[0] % P) return HK_ERR_ARG;
        base[b] = (u64)(i / P) * d->tx_stride + d->wit_offsets[i % P];
    }
    if (batch == 0) return HK_OK;
    const size_t len = d->body_len[sub_index[0] % P];
    if (body_col0 < 1 || body_col0 > n_v || len > n_v - body_col0) return HK_ERR_ARG;
    if (!is_device_ptr(z_out) || bufs_overlap(z_out, batch * n_v * fr, d->witness_mont, n_wit * fr)) return HK_ERR_ARG;
    Staged in = staged(d->witness_mont, n_wit * fr);
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    u64* base_d;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, &in, 1);
        base_d = c.n<u64>(batch);
    }));
    hipStream_t s = L->stream;
    const void* wit = in.p;
    HK_TRY(stage_upload(L, &in, 1));
    HK_HIP(hipMemcpyAsync(base_d, base.data(), 8 * batch, hipMemcpyHostToDevice, s));
    const u32 per = (u32)(1 + len);                                // <= n_v < 2^31
    for (size_t b0 = 0; b0 < batch; b0 += RJ_GRID_ROWS) {           // a grid's y holds at most 65 535 rows
        const u32 nb = (u32)std::min(batch - b0, (size_t)RJ_GRID_ROWS);
        HK_LAUNCH((k_rj_body<Fr>), dim3((per + 255) / 256, nb), dim3(256), 0, s, (const Fr*)wit, (const u64*)base_d + b0, per,
                  n_v, body_col0, (Fr*)z_out + b0 * n_v);
    }
    return L->settle();
}

}  // namespace hk
