// job_args.h — the argument rules the job entries share (hk_exec_tree, hk_stage0 / stage1_witness and their RAM twins,
// hk_r1cs_job_*, hk_vkd_*, hk_sha_tree*, hk_trace_sort, hk_poseidon_path), each stated once.  Host only:
// nothing but include/hekaton.h and the standard library, so a stand-alone host program can include it
// (tests/host_shim/job_args_driver.cpp).  A rule refuses with HK_ERR_ARG and touches nothing.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/hekaton.h"

namespace hk {

// ---- Poseidon descriptors (execution tree, subcircuit_circuit.rs:233-252) --------------------------------------------
// The host-side description of one Poseidon instance of the tree (poseidon_util.rs:53-62): width t = rate + 1 (3 or 4),
// S-box exponent 5 or 17, rf full and rp partial rounds; consts = ark[(rf + rp)][t] then mds[t][t], Montgomery.
struct PoseidonDesc { uint32_t t, alpha, rf, rp, off; };
inline PoseidonDesc poseidon_desc(const hk_poseidon_desc* d) {
    return {d->t, d->alpha, d->full_rounds, d->partial_rounds, d->consts_offset};
}
// witnesses of one traced permutation: per S-box 3 chain values at alpha 5 and 5 at 17, t of them in a full round and one in
// a partial round, and the t state elements after every round
inline size_t poseidon_trace_len(const hk_poseidon_desc* d) {
    size_t chain = d->alpha == 5 ? 3 : 5;
    return (size_t)d->full_rounds * (d->t * chain + d->t) + (size_t)d->partial_rounds * (chain + d->t);
}
// columns of a membership block: two leaf permutations, then per level (bit, sibling, left input) and a node permutation
inline size_t poseidon_path_len(const hk_poseidon_desc* lh, const hk_poseidon_desc* nh, size_t depth) {
    return 2 * poseidon_trace_len(lh) + depth * (3 + poseidon_trace_len(nh));
}
// the (leaf, node) pair of a job: rounds even and non-zero, constants inside n_consts, and the pair the kernels are compiled
// for - the reference's two instances (poseidon_util.rs:53-62): t 4 / alpha 5 over a leaf, t 3 / alpha 17 two-to-one
inline hk_status poseidon_pair_check(const hk_poseidon_desc* lh, const hk_poseidon_desc* nh, size_t n_consts) {
    for (const hk_poseidon_desc* p : {lh, nh}) {
        if ((p->full_rounds & 1) || p->full_rounds + p->partial_rounds == 0 ||
            (size_t)p->consts_offset + (size_t)(p->full_rounds + p->partial_rounds) * p->t + (size_t)p->t * p->t > n_consts)
            return HK_ERR_ARG;
    }
    if (lh->t != 4 || nh->t != 3 || lh->alpha != 5 || nh->alpha != 17) return HK_ERR_ARG;
    return HK_OK;
}

// ---- subtraces ------------------------------------------------------------------------------------------------------------
// offsets: n_sub + 1 words, offsets[0] = 0, non-decreasing
inline hk_status offsets_check(const uint32_t* offsets, size_t n_sub) {
    if (offsets[0] != 0) return HK_ERR_ARG;
    for (size_t i = 0; i < n_sub; i++)
        if (offsets[i + 1] < offsets[i]) return HK_ERR_ARG;
    return HK_OK;
}
// what a portal witness call checks of (offsets, sub_index) and hands its kernels: rows[2 b] = subcircuit sub_index[b],
// rows[2 b + 1] = its first entry.  Every selected subcircuit owns exactly K entries.  Reads sub_index[0 .. batch): a caller
// bounds batch (its lane counts) BEFORE this.
inline hk_status portal_rows(const uint32_t* offsets, size_t n_sub, size_t K, const uint32_t* sub_index, size_t batch,
                             std::vector<uint32_t>& rows) {
    if (offsets_check(offsets, n_sub) != HK_OK) return HK_ERR_ARG;
    rows.resize(2 * batch);
    for (size_t b = 0; b < batch; b++) {
        const uint32_t i = sub_index[b];
        if (i >= n_sub || offsets[i + 1] - offsets[i] != K) return HK_ERR_ARG;
        rows[2 * b] = i;
        rows[2 * b + 1] = offsets[i];
    }
    return HK_OK;
}
// an execution tree: 2^depth = n_sub leaves, 2 <= n_sub <= 2^24 (ark MerkleTree::new wants 2^k >= 2 leaves)
inline hk_status tree_shape_check(size_t n_sub, size_t depth) {
    if (n_sub < 2 || (n_sub & (n_sub - 1)) || n_sub > ((size_t)1 << 24) || depth > 24 || ((size_t)1 << depth) != n_sub)
        return HK_ERR_ARG;
    return HK_OK;
}

// ---- columns and buffers --------------------------------------------------------------------------------------------------
// n column ranges [lo[a], lo[a] + len[a]): each inside [1, n_v) - column 0 is the constant's - and no two overlapping
inline hk_status col_ranges_check(const size_t* lo, const size_t* len, int n, size_t n_v) {
    for (int a = 0; a < n; a++) {
        if (lo[a] < 1 || lo[a] > n_v || len[a] > n_v - lo[a]) return HK_ERR_ARG;
        for (int b = 0; b < a; b++)
            if (lo[a] < lo[b] + len[b] && lo[b] < lo[a] + len[a]) return HK_ERR_ARG;
    }
    return HK_OK;
}
// two buffers share a byte; a NULL buffer is absent and overlaps nothing
inline bool bufs_overlap(const void* a, size_t a_len, const void* b, size_t b_len) {
    return a && b && (const char*)a < (const char*)b + b_len && (const char*)b < (const char*)a + a_len;
}

}  // namespace hk
