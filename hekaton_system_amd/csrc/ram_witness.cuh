// ram_witness.cuh — the witness of a RAM portal subcircuit on the device (hk_ram_stage0_witness / hk_ram_stage1_witness,
// DESIGN.md section 4m): what distributed-prover/src/portal_manager/ram_portal_manager.rs:150-230 and
// subcircuit_circuit.rs:166-273 witness for a `MEM_TYPE = Ram` circuit, from hk_trace_sort's and hk_exec_tree's RAM outputs
// where they lie.  The column order is hekaton_system_amd/vm_circuit.py `RamSubcircuit._program`'s and is stated once, here.
//
// An ENTRY takes RW_ENTRY = 35 columns: val, addr, timestamp bit 0 .. 31 (least significant first), read.  With K = n_portals:
//
//   stage 0 (70 K columns from stage0_col0)   the K time-ordered entries, then the K address-ordered ones
//   portal block (43 K + 37 columns from col0)
//     [0, 35)                                 the previous leaf's last address-ordered entry (all zero in front of entry 0)
//     chain of order y at 35 + y (1 + 4 K)    evals[i - 1][y] (1 for i = 0), then per entry p1 = c1 addr, p2 = c2 ts,
//                                             e = val + p1 + p2 + c3 read, cur <- cur (tr_chal - e)
//     pair j at 37 + 8 K + 35 j               of [previous] + the address-ordered entries, d = addr' - addr: inv = 1 / d or 0,
//                                             same = [d == 0], sr = same read', delta bit 0 .. 31 of ts' - ts - 1 when same, else 0
//   membership block (from pos_col0)          hk_poseidon_path's order over the six leaf fields
//
//   k_rw_canon     one lane per (row, slot): the timestamp of each of the row's 2 K + 1 entries out of Montgomery form ONCE, as a
//                  u32 in scratch, the `same` flag of each pair, and the call's error word: a timestamp >= 2^32 or a read flag
//                  other than 0 / 1 in a selected subcircuit.  Nothing is written to the output before the host has read that word.
//   k_rw_template  row <- template, column fastest.
//   k_rw_fill      every copied or bit-valued column, COLUMN FASTEST: a wave stores 64 consecutive Fr of one row.  Bits are
//                  Fr::one() / Fr::zero() picked by an integer test of the canonical timestamps in scratch: no field operation.
//   k_rw_products  one lane per (row, order, entry): p1, p2, e; one lane per (row, pair): inv (fp_inv, 0 -> 0), same, sr.
//   k_rw_chunk_prod / k_rw_chunk_scan / k_rw_chain_walk   the two chains of a row in chunks of RW_CHUNK entries: the product of
//                  each chunk's factors tr_chal - e, one lane per chain over the chunk products, then every chunk walked from
//                  the evaluation in front of it: RW_CHUNK + K / RW_CHUNK + RW_CHUNK products in sequence instead of K.
//   k_poseidon_membership<Fr, 6>   poseidon.cuh's quad kernel with a six-field leaf.
#pragma once
#include "poseidon.cuh"
#include "stage1.cuh"        // s1_prologue, EtChal

namespace hk {

constexpr u32 RW_ENTRY = 35;           // columns of one entry: val, addr, 32 timestamp bits, read
constexpr u32 RW_CHUNK = 32;           // entries of one chunk of a running-evaluation chain

#if defined(__HIPCC__)

// what the kernels share: row b is subcircuit rows[2 b] whose entries start at rows[2 b + 1] in both orders
template <class Fr>
struct RwArgs {
    const Fr* time_e;
    const Fr* addr_e;
    const u32* rows;
    u32* ts32;             // batch x (2 K + 1): canonical timestamps of the time entries, the address entries, the previous entry
    u32* same;             // batch x K: pair j joins entries of one address
    u32 batch, K;
    size_t n_v, inst_col0, stage0_col0, col0;
    Fr* z;
};

// entry s of row b: s < K time-ordered, s < 2 K address-ordered, s == 2 K the previous leaf's last entry (nullptr in front
// of entry 0)
template <class Fr>
__device__ __forceinline__ const Fr* rw_entry(const RwArgs<Fr>& a, u64 off, u32 s) {
    if (s < a.K) return a.time_e + (off + s) * 4;
    if (s < 2 * a.K) return a.addr_e + (off + (s - a.K)) * 4;
    return off ? a.addr_e + (off - 1) * 4 : nullptr;
}

template <class Fr>
__global__ void __launch_bounds__(256) k_rw_canon(RwArgs<Fr> a, u32* __restrict__ flag) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 per = 2 * a.K + 1;
    if (g >= (u64)a.batch * per) return;
    const u32 b = (u32)(g / per), s = (u32)(g % per);
    const u64 off = a.rows[2 * b + 1];
    const Fr* e = rw_entry(a, off, s);
    u32 ts = 0;
    bool ok = true;
    if (e) {
        const Fr t = Fr::from_mont(fr_load(&e[2]));
        u32 hi = 0;
        HK_UNROLL for (int i = 1; i < Fr::N; i++) hi |= t.v[i];
        ts = t.v[0];
        const Fr rd = Fr::canon(fr_load(&e[3]));
        // the previous entry belongs to a subcircuit that is not selected: it is never a reason to refuse
        if (s < 2 * a.K) ok = hi == 0 && (rd.is_zero() || rd == Fr::one());
    }
    a.ts32[g] = ts;
    if (s >= a.K && s < 2 * a.K) {
        const Fr* p = rw_entry(a, off, s == a.K ? 2 * a.K : s - 1);
        Fr d = fr_load(&e[0]);
        if (p) d = Fr::sub(d, fr_load(&p[0]));
        a.same[(size_t)b * a.K + (s - a.K)] = Fr::canon(d).is_zero() ? 1u : 0u;
    }
    if (!ok) atomicOr(flag, 1u);
}

// column f of entry s of row b: a copy of val / addr / read, or timestamp bit f - 2 as Fr::one() / Fr::zero()
template <class Fr>
__device__ __forceinline__ Fr rw_entry_col(const RwArgs<Fr>& a, u64 off, const u32* ts, u32 s, u32 f) {
    const Fr* e = rw_entry(a, off, s);
    Fr x = Fr::zero();
    if (f >= 2 && f < 34) {
        if ((ts[s] >> (f - 2)) & 1u) x = Fr::one();
    } else if (e) {
        x = fr_load(&e[f == 0 ? 1 : f == 1 ? 0 : 3]);              // val, addr, read out of (addr, val, ts, read)
    }
    return x;
}

// hk_ram_stage0_witness: lane (b, c) over the 70 K stage-0 columns alone, column fastest (a.n_v = 70 K, a.stage0_col0 = 0)
template <class Fr>
__global__ void __launch_bounds__(256) k_rw_stage0(RwArgs<Fr> a) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 per = 2 * RW_ENTRY * a.K;
    if (g >= (u64)a.batch * per) return;
    const u32 b = (u32)(g / per), c = (u32)(g % per);
    fr_store(&a.z[g], rw_entry_col(a, a.rows[2 * b + 1], a.ts32 + (size_t)b * (2 * a.K + 1), c / RW_ENTRY, c % RW_ENTRY));
}

template <class Fr>
__global__ void __launch_bounds__(256)
k_rw_template(const Fr* __restrict__ tmpl, u64 total, size_t n_v, Fr* __restrict__ z) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    fr_store(&z[g], fr_load(&tmpl[g % n_v]));
}

// Lane (b, c), c the fast index over the 5 + 105 K + 35 columns this kernel owns:
//   [0, 5)                       c1, c2, c3, tr_chal, root                       -> inst_col0 + c
//   [5, 5 + 70 K)                field f of stage-0 entry s                      -> stage0_col0 + 35 s + f
//   [5 + 70 K, 40 + 70 K)        field f of the previous entry                   -> col0 + f
//   [40 + 70 K, 40 + 105 K)      column f of pair j; f < 3 belongs to k_rw_products  -> col0 + 37 + 8 K + 35 j + f
template <class Fr>
__global__ void __launch_bounds__(256) k_rw_fill(RwArgs<Fr> a, EtChal<Fr> ch, const Fr* __restrict__ root) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 K = a.K, per = 40 + 105 * K;
    if (g >= (u64)a.batch * per) return;
    const u32 b = (u32)(g / per), c = (u32)(g % per);
    const u64 off = a.rows[2 * b + 1];
    const u32* ts = a.ts32 + (size_t)b * (2 * K + 1);
    Fr* z = a.z + (size_t)b * a.n_v;
    if (c < 5) {
        fr_store(&z[a.inst_col0 + c], c == 4 ? fr_load(root) : ch.c[c]);
        return;
    }
    if (c < 40 + 70 * K) {                                         // an entry's column: a copy or a timestamp bit
        const u32 s = (c - 5) / RW_ENTRY, f = (c - 5) % RW_ENTRY;
        Fr* dst = s < 2 * K ? &z[a.stage0_col0 + (c - 5)] : &z[a.col0 + f];
        fr_store(dst, rw_entry_col(a, off, ts, s, f));
        return;
    }
    const u32 j = (c - (40 + 70 * K)) / RW_ENTRY, f = (c - (40 + 70 * K)) % RW_ENTRY;
    if (f < 3) return;
    const u32 t1 = ts[K + j], t0 = ts[j ? K + j - 1 : 2 * K];
    const u32 delta = a.same[(size_t)b * K + j] ? t1 - t0 - 1u : 0u;
    fr_store(&z[a.col0 + 37 + 8 * K + RW_ENTRY * j + f], (delta >> (f - 3)) & 1u ? Fr::one() : Fr::zero());
}

// Role-major on purpose, unlike k_rw_fill: a lane's three stores are 4 or 35 columns from its neighbour's whichever index is
// fast, so nothing coalesces either way, and with b fast the lanes of a wave share a role - the fp_inv lanes do not sit among
// product lanes and make a whole wave wait for the inversion.  62 us of a 3.2 ms call at k = 3 104.
// Lane (role, b): roles [0, 2 K) = (order y, entry j): p1, p2, e at col0 + 35 + y (1 + 4 K) + 1 + 4 j; roles
// [2 K, 3 K) = pair j: inv, same, sr.
template <class Fr>
__global__ void __launch_bounds__(256) k_rw_products(RwArgs<Fr> a, EtChal<Fr> ch) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 K = a.K;
    if (g >= (u64)3 * K * a.batch) return;
    const u32 role = (u32)(g / a.batch), b = (u32)(g % a.batch);
    const u64 off = a.rows[2 * b + 1];
    Fr* z = a.z + (size_t)b * a.n_v;
    if (role < 2 * K) {
        const u32 y = role / K, j = role % K;
        const Fr* e = (y ? a.addr_e : a.time_e) + (off + j) * 4;
        Fr* w = z + a.col0 + RW_ENTRY + y * (1 + 4 * K) + 1 + 4 * j;
        const Fr p1 = Fr::mul(ch.c[0], fr_load(&e[0])), p2 = Fr::mul(ch.c[1], fr_load(&e[2]));
        Fr r = Fr::add(Fr::add(fr_load(&e[1]), p1), Fr::add(p2, Fr::mul(ch.c[2], fr_load(&e[3]))));
        fr_store(&w[0], p1);
        fr_store(&w[1], p2);
        fr_store(&w[2], r);
    } else {
        const u32 j = role - 2 * K;
        const Fr* e = a.addr_e + (off + j) * 4;
        const Fr* p = rw_entry(a, off, j ? K + j - 1 : 2 * K);
        Fr d = fr_load(&e[0]);
        if (p) d = Fr::sub(d, fr_load(&p[0]));
        d = Fr::canon(d);
        const bool same = d.is_zero();
        Fr* w = z + a.col0 + 37 + 8 * K + RW_ENTRY * j;
        fr_store(&w[0], fp_inv(d));                                // maps 0 to 0
        fr_store(&w[1], same ? Fr::one() : Fr::zero());
        fr_store(&w[2], same ? fr_load(&e[3]) : Fr::zero());
    }
}

// The chains, split as hk_exec_tree splits its product scan: a chain is cut into chunks of RW_CHUNK entries.  Chain g = 2 b + y
// starts at column col0 + 35 + y (1 + 4 K) of row b; its entry j has e at + 1 + 4 j + 2 (stored by k_rw_products) and cur at
// + 1 + 4 j + 3.
template <class Fr>
__device__ __forceinline__ Fr* rw_chain(const RwArgs<Fr>& a, u32 g) {
    return a.z + (size_t)(g >> 1) * a.n_v + a.col0 + RW_ENTRY + (g & 1u) * (1 + 4 * a.K);
}
// (1) prods[g][c] = product of (tr_chal - e) over chunk c of chain g: one lane per (chain, chunk)
template <class Fr>
__global__ void __launch_bounds__(256) k_rw_chunk_prod(RwArgs<Fr> a, EtChal<Fr> ch, u32 n_chunks, Fr* __restrict__ prods) {
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    if (t >= (u64)2 * a.batch * n_chunks) return;
    const u32 g = (u32)(t / n_chunks), c = (u32)(t % n_chunks);
    const Fr* w = rw_chain(a, g);
    const u32 end = min(a.K, (c + 1) * RW_CHUNK);
    Fr acc = Fr::one();
    HK_NOUNROLL for (u32 j = c * RW_CHUNK; j < end; j++) acc = Fr::mul(acc, Fr::sub(ch.c[3], fr_load(&w[1 + 4 * j + 2])));
    fr_store(&prods[t], acc);
}
// (2) one lane per chain: the start evaluation - evals[i - 1][y], 1 for i = 0 - into the chain's first column, and prods[g][c]
// <- the evaluation in front of chunk c
template <class Fr>
__global__ void __launch_bounds__(64)
k_rw_chunk_scan(RwArgs<Fr> a, const Fr* __restrict__ evals, u32 n_chunks, Fr* __restrict__ prods) {
    const u32 g = blockIdx.x * 64 + threadIdx.x;
    if (g >= 2 * a.batch) return;
    const u32 i = a.rows[2 * (g >> 1)];
    Fr run = Fr::one();
    if (i) run = fr_load(&evals[(size_t)(i - 1) * 2 + (g & 1u)]);
    fr_store(rw_chain(a, g), run);
    Fr* p = prods + (size_t)g * n_chunks;
    HK_NOUNROLL for (u32 c = 0; c < n_chunks; c++) {
        const Fr t = fr_load(&p[c]);
        fr_store(&p[c], run);
        run = Fr::mul(run, t);
    }
}
// (3) one lane per (chain, chunk): cur <- cur (tr_chal - e) over the chunk, from the evaluation in front of it
template <class Fr>
__global__ void __launch_bounds__(256) k_rw_chain_walk(RwArgs<Fr> a, EtChal<Fr> ch, u32 n_chunks, const Fr* __restrict__ prods) {
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    if (t >= (u64)2 * a.batch * n_chunks) return;
    const u32 g = (u32)(t / n_chunks), c = (u32)(t % n_chunks);
    Fr* w = rw_chain(a, g);
    const u32 end = min(a.K, (c + 1) * RW_CHUNK);
    Fr cur = fr_load(&prods[t]);
    HK_NOUNROLL for (u32 j = c * RW_CHUNK; j < end; j++) {
        cur = Fr::mul(cur, Fr::sub(ch.c[3], fr_load(&w[1 + 4 * j + 2])));
        fr_store(&w[1 + 4 * j + 3], cur);
    }
}

#endif  // __HIPCC__

// the lane counts of both calls: every grid is ceil(lanes / 256) blocks, lanes a u64 below 2^38
static inline bool rw_lanes_ok(size_t K, size_t batch, size_t n_v) {
    return K != 0 && K <= (1u << 16) && batch < (1u << 20) && batch * (40 + 105 * K) < ((size_t)1 << 38) &&
           batch * n_v < ((size_t)1 << 38);
}

template <class C>
hk_status Ops<C>::ram_stage0_witness(hk_ctx* ctx, const uint32_t* offsets, uint32_t n_sub, uint32_t n_portals,
                                     const void* time_entries, const void* addr_entries, const uint32_t* sub_index, size_t batch,
                                     void* w_out) {
    if (!offsets || !time_entries || !addr_entries || (batch && (!sub_index || !w_out))) return HK_ERR_ARG;
    const size_t K = n_portals;
    if (n_sub == 0 || !rw_lanes_ok(K, batch, 70 * K)) return HK_ERR_ARG;
    std::vector<u32> rows;                                 // outlives the lane's copy
    HK_TRY(portal_rows(offsets, n_sub, K, sub_index, batch, rows));
    if (batch == 0) return HK_OK;
    if (!is_device_ptr(w_out)) return HK_ERR_ARG;
    const size_t bytes = (size_t)offsets[n_sub] * 4 * sizeof(Fr);
    Staged in[2] = {staged(time_entries, bytes), staged(addr_entries, bytes)};
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    u32 *rows_d, *ts32, *same, *flag;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, in, 2);
        rows_d = c.n<u32>(2 * batch);
        ts32 = c.n<u32>(batch * (2 * K + 1));
        same = c.n<u32>(batch * K);
        flag = c.n<u32>(1);
    }));
    hipStream_t s = L->stream;
    HK_TRY(stage_upload(L, in, 2));
    HK_HIP(hipMemcpyAsync(rows_d, rows.data(), 4 * rows.size(), hipMemcpyHostToDevice, s));
    HK_HIP(hipMemsetAsync(flag, 0, 4, s));
    // a row of w_out is the 70 K stage-0 columns alone: stage0_col0 = 0, n_v = 70 K; the other ranges are never written
    RwArgs<Fr> a{(const Fr*)in[0].p, (const Fr*)in[1].p, rows_d, ts32, same, (u32)batch, (u32)K, 70 * K, 0, 0, 0, (Fr*)w_out};
    const u64 n_canon = (u64)batch * (2 * K + 1), n_fill = (u64)batch * 70 * K;
    // the timestamps and the error word first: nothing touches w_out before the host has read it (as hk_ram_stage1_witness)
    HK_LAUNCH((k_rw_canon<Fr>), dim3((u32)((n_canon + 255) / 256)), dim3(256), 0, s, a, flag);
    u32 fl = 0;
    HK_HIP(hipMemcpyAsync(&fl, flag, 4, hipMemcpyDeviceToHost, s));
    HK_HIP(hipStreamSynchronize(s));
    if (fl) { HK_TRY(L->settle()); return HK_ERR_ARG; }
    HK_LAUNCH((k_rw_stage0<Fr>), dim3((u32)((n_fill + 255) / 256)), dim3(256), 0, s, a);
    return L->settle();
}

template <class C>
hk_status Ops<C>::ram_stage1_witness(hk_ctx* ctx, const hk_ram_stage1_desc* d, const uint32_t* sub_index, size_t batch, size_t n_v,
                                     void* z_out) {
    const size_t n_sub = d->n_sub, K = d->n_portals, depth = d->depth;
    if (!rw_lanes_ok(K, batch, n_v)) return HK_ERR_ARG;
    std::vector<u32> rows;                                 // outlives the lane's copies
    EtChal<Fr> ch;
    HK_TRY(s1_prologue(d, sub_index, batch, z_out, 4, rows, ch));
    // the four column ranges: inside [1, n_v), no two overlapping.  Six leaf fields take two permutations, as four do.
    const size_t lo[4] = {d->inst_col0, d->stage0_col0, d->col0, d->pos_col0};
    const size_t len[4] = {5, 70 * K, 43 * K + 37, poseidon_path_len(d->leaf_hash, d->node_hash, depth)};
    HK_TRY(col_ranges_check(lo, len, 4, n_v));
    if (batch == 0) return HK_OK;
    if (!is_device_ptr(z_out)) return HK_ERR_ARG;

    const size_t n = d->offsets[n_sub], fr = sizeof(Fr);
    constexpr int N_IN = 8;                                // the last one, the template, may be absent
    Staged in[N_IN] = {staged(d->time_entries_mont, n * 4 * fr), staged(d->addr_entries_mont, n * 4 * fr),
                       staged(d->consts_mont, d->n_consts * fr), staged(d->evals_mont, n_sub * 2 * fr),
                       staged(d->leaves_mont, n_sub * 6 * fr),   staged(d->siblings_mont, n_sub * depth * fr),
                       staged(d->root_mont, fr),                 staged(d->template_mont, n_v * fr)};
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    u32 *rows_d, *ts32, *same, *flag;
    Fr* prods;
    const u32 n_chunks = (u32)((K + RW_CHUNK - 1) / RW_CHUNK);
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, in, N_IN);
        rows_d = c.n<u32>(2 * batch);
        ts32 = c.n<u32>(batch * (2 * K + 1));
        same = c.n<u32>(batch * K);
        flag = c.n<u32>(1);
        prods = c.n<Fr>(2 * batch * n_chunks);
    }));
    hipStream_t s = L->stream;
    HK_TRY(stage_upload(L, in, N_IN));
    HK_HIP(hipMemcpyAsync(rows_d, rows.data(), 4 * rows.size(), hipMemcpyHostToDevice, s));
    HK_HIP(hipMemsetAsync(flag, 0, 4, s));
    RwArgs<Fr> a{(const Fr*)in[0].p, (const Fr*)in[1].p, rows_d, ts32, same, (u32)batch, (u32)K, n_v,
                 (size_t)d->inst_col0, (size_t)d->stage0_col0, (size_t)d->col0, (Fr*)z_out};
    const u32 nb = (u32)batch;
    auto blocks = [](u64 lanes) { return dim3((u32)((lanes + 255) / 256)); };
    // the timestamps and the error word first: nothing touches z_out before the host has read it
    HK_LAUNCH((k_rw_canon<Fr>), blocks((u64)batch * (2 * K + 1)), dim3(256), 0, s, a, flag);
    u32 fl = 0;
    HK_HIP(hipMemcpyAsync(&fl, flag, 4, hipMemcpyDeviceToHost, s));
    HK_HIP(hipStreamSynchronize(s));
    if (fl) { HK_TRY(L->settle()); return HK_ERR_ARG; }
    if (d->template_mont)
        HK_LAUNCH((k_rw_template<Fr>), blocks((u64)batch * n_v), dim3(256), 0, s, (const Fr*)in[7].p, (u64)batch * n_v, n_v,
                  (Fr*)z_out);
    HK_LAUNCH((k_rw_fill<Fr>), blocks((u64)batch * (40 + 105 * K)), dim3(256), 0, s, a, ch, (const Fr*)in[6].p);
    HK_LAUNCH((k_rw_products<Fr>), blocks((u64)batch * 3 * K), dim3(256), 0, s, a, ch);
    HK_LAUNCH((k_rw_chunk_prod<Fr>), blocks((u64)2 * batch * n_chunks), dim3(256), 0, s, a, ch, n_chunks, prods);
    HK_LAUNCH((k_rw_chunk_scan<Fr>), dim3((2 * nb + 63) / 64), dim3(64), 0, s, a, (const Fr*)in[3].p, n_chunks, prods);
    HK_LAUNCH((k_rw_chain_walk<Fr>), blocks((u64)2 * batch * n_chunks), dim3(256), 0, s, a, ch, n_chunks, (const Fr*)prods);
    HK_TRY((poseidon_membership<Fr, 6>(s, in[2].p, d->leaf_hash, d->node_hash, in[4].p, in[5].p, rows_d, rows_d, 2, depth, batch, n_v,
                                       (size_t)d->pos_col0, z_out)));
    return L->settle();
}

}  // namespace hk
