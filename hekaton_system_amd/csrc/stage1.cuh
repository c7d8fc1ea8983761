// stage1.cuh — the challenge-dependent columns of a subcircuit's stage-1 assignment on the device (hk_stage1_witness,
// DESIGN.md section 4i): what distributed-prover/src/subcircuit_circuit.rs:206-252 witnesses from the Stage1Request of
// coordinator.rs:569-604, taken from hk_exec_tree's outputs where they lie.
//
//   k_s1_values      the three instance values and the portal block (10 k + 4 columns for k entries per order): copies, the two
//                    running-evaluation chains, the address-step (inv, same) pairs.  One lane per (role, row), role-major, so
//                    the lanes of a wave share a role: 4 k + 5 copies, 2 chains of k products, k inversions.
//   k_poseidon_membership<Fr, 4>   the Poseidon membership block on a quad of lanes per row (poseidon.cuh).
#pragma once
#include "exec_tree.cuh"     // EtChal, et_repr
#include "poseidon.cuh"

namespace hk {

#if defined(__HIPCC__)

// Row b of z is subcircuit i = rows[2 b], whose entries start at off = rows[2 b + 1] in both orders.  Lane g: role g / batch,
// row g % batch.  Roles, with K = n_portals:
//   [0, 3)               instance: entry_chal, tr_chal, root                          -> inst_col0 + role
//   [3, 3 + 4 K)         (addr, val) of the K time-ordered then the K address-ordered entries -> col0 + (role - 3)
//   [3 + 4 K, 5 + 4 K)   the previous leaf's last address-ordered entry, zero in front of entry 0    -> col0 + 8 K + 2 + f
//   [5 + 4 K, 7 + 4 K)   chain of order y: evals[i - 1][y] (1 for i = 0), then per entry e = val + entry_chal addr and
//                        cur <- cur (tr_chal - e)                                     -> col0 + 4 K + y (1 + 2 K) ...
//   [7 + 4 K, 7 + 5 K)   step j: d = addr[off + j] - addr[off + j - 1] (minus 0 at entry 0), inv = 1 / d or 0, same = [d == 0]
//                                                                                    -> col0 + 8 K + 4 + 2 j, + 1
template <class Fr>
__global__ void __launch_bounds__(256)
k_s1_values(const Fr* __restrict__ time_e, const Fr* __restrict__ addr_e, const u32* __restrict__ rows, u32 batch, u32 K,
            EtChal<Fr> ch, const Fr* __restrict__ evals, const Fr* __restrict__ root, size_t n_v, size_t inst_col0, size_t col0,
            Fr* __restrict__ z_out) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 role = g / batch, b = g % batch;
    if (role >= 7 + 5 * K) return;
    const u32 i = rows[2 * b];
    const u64 off = rows[2 * b + 1];
    Fr* z = z_out + (size_t)b * n_v;
    if (role < 3) {
        fr_store(&z[inst_col0 + role], role == 2 ? fr_load(root) : ch.c[role]);
    } else if (role < 3 + 4 * K) {
        const u32 c = role - 3;                                    // 2 K Fr of the time order, then 2 K of the address order
        const Fr* src = c < 2 * K ? time_e + off * 2 + c : addr_e + off * 2 + (c - 2 * K);
        fr_store(&z[col0 + c], fr_load(src));
    } else if (role < 5 + 4 * K) {
        const u32 f = role - (3 + 4 * K);
        Fr x = Fr::zero();
        if (off) x = fr_load(&addr_e[(off - 1) * 2 + f]);
        fr_store(&z[col0 + 8 * K + 2 + f], x);
    } else if (role < 7 + 4 * K) {
        const u32 y = role - (5 + 4 * K);
        const Fr* e = (y ? addr_e : time_e) + off * 2;
        Fr* w = z + col0 + 4 * K + y * (1 + 2 * K);
        Fr cur = Fr::one();
        if (i) cur = fr_load(&evals[(size_t)(i - 1) * 2 + y]);
        fr_store(w++, cur);
        HK_NOUNROLL for (u32 j = 0; j < K; j++) {
            Fr r = et_repr<Fr, 2>(e + 2 * (size_t)j, ch);
            cur = Fr::mul(cur, Fr::sub(ch.c[1], r));
            fr_store(w++, r);
            fr_store(w++, cur);
        }
    } else {
        const u32 j = role - (7 + 4 * K);
        const u64 at = off + j;
        Fr d = fr_load(&addr_e[at * 2]);
        if (at) d = Fr::sub(d, fr_load(&addr_e[(at - 1) * 2]));
        d = Fr::canon(d);
        Fr* w = z + col0 + 8 * K + 4 + 2 * j;
        fr_store(&w[0], fp_inv(d));                                // maps 0 to 0
        fr_store(&w[1], d.is_zero() ? Fr::one() : Fr::zero());
    }
}

#endif  // __HIPCC__

// What hk_stage1_witness and hk_ram_stage1_witness check alike of a descriptor D (hk_stage1_desc / hk_ram_stage1_desc: the same
// leading fields) and hand their kernels: the NULL pointers, the tree's shape, the rows (job_args.h portal_rows), the Poseidon
// pair, and the n_chal challenges (the rest zero).  Reads sub_index[0 .. batch): the caller bounds its lane counts before.
template <class Fr, class D>
hk_status s1_prologue(const D* d, const uint32_t* sub_index, size_t batch, const void* z_out, size_t n_chal, std::vector<u32>& rows,
                      EtChal<Fr>& ch) {
    if (!d->offsets || !d->time_entries_mont || !d->addr_entries_mont || !d->challenges_mont || !d->evals_mont ||
        !d->leaves_mont || !d->siblings_mont || !d->root_mont || !d->consts_mont || !d->leaf_hash || !d->node_hash ||
        (batch && (!sub_index || !z_out)))
        return HK_ERR_ARG;
    HK_TRY(tree_shape_check(d->n_sub, d->depth));
    HK_TRY(portal_rows(d->offsets, d->n_sub, d->n_portals, sub_index, batch, rows));
    HK_TRY(poseidon_pair_check(d->leaf_hash, d->node_hash, d->n_consts));
    for (size_t k = 0; k < 4; k++) {
        ch.c[k] = Fr::zero();
        if (k < n_chal) memcpy(&ch.c[k], (const char*)d->challenges_mont + k * sizeof(Fr), sizeof(Fr));
    }
    return HK_OK;
}

template <class C>
hk_status Ops<C>::stage1_witness(hk_ctx* ctx, const hk_stage1_desc* d, const uint32_t* sub_index, size_t batch, size_t n_v,
                                 void* z_out) {
    const size_t n_sub = d->n_sub, K = d->n_portals, depth = d->depth;
    if (K == 0 || K > (1u << 16) || batch >= (1u << 20) || (7 + 5 * K) * batch >= ((size_t)1 << 31)) return HK_ERR_ARG;   // lanes of k_s1_values
    std::vector<u32> rows;                                 // (subcircuit, its first entry) per row; outlives the lane's copies
    EtChal<Fr> ch;
    HK_TRY(s1_prologue(d, sub_index, batch, z_out, 2, rows, ch));
    // the three column ranges: inside [1, n_v), no two overlapping
    const size_t lo[3] = {d->inst_col0, d->col0, d->pos_col0};
    const size_t len[3] = {3, 10 * K + 4, poseidon_path_len(d->leaf_hash, d->node_hash, depth)};      // as hk_poseidon_path
    HK_TRY(col_ranges_check(lo, len, 3, n_v));
    if (batch == 0) return HK_OK;
    if (!is_device_ptr(z_out)) return HK_ERR_ARG;

    const size_t n = d->offsets[n_sub], fr = sizeof(Fr);
    Staged in[] = {staged(d->time_entries_mont, n * 2 * fr), staged(d->addr_entries_mont, n * 2 * fr),
                   staged(d->consts_mont, d->n_consts * fr), staged(d->evals_mont, n_sub * 2 * fr),
                   staged(d->leaves_mont, n_sub * 4 * fr),   staged(d->siblings_mont, n_sub * depth * fr),
                   staged(d->root_mont, fr)};
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    u32* rows_d;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, in, 7);
        rows_d = c.n<u32>(2 * batch);
    }));
    hipStream_t s = L->stream;
    HK_TRY(stage_upload(L, in, 7));
    HK_HIP(hipMemcpyAsync(rows_d, rows.data(), 4 * rows.size(), hipMemcpyHostToDevice, s));
    const Fr *tp = (const Fr*)in[0].p, *ap = (const Fr*)in[1].p;
    const u32 nb = (u32)batch, lanes = (u32)((7 + 5 * K) * batch);
    HK_LAUNCH((k_s1_values<Fr>), dim3((lanes + 255) / 256), dim3(256), 0, s, tp, ap, (const u32*)rows_d, nb, (u32)K, ch,
              (const Fr*)in[3].p, (const Fr*)in[6].p, n_v, (size_t)d->inst_col0, (size_t)d->col0, (Fr*)z_out);
    HK_TRY((poseidon_membership<Fr, 4>(s, in[2].p, d->leaf_hash, d->node_hash, in[4].p, in[5].p, rows_d, rows_d, 2, depth, batch, n_v,
                                       (size_t)d->pos_col0, z_out)));
    return L->settle();
}

}  // namespace hk
