// job_args_driver.cpp — hekaton_system_amd/csrc/job_args.h over a table of the refusals the GPU tests name for the rules the
// job entries share, each beside its nearest valid case.  Prints one `name status` line per case (tests/test_job_args_cpu.py
// holds the expected statuses); exits non-zero when portal_rows hands back other rows than it should.  Host only: built with
// the host compiler, once plain and once with -fsanitize=address,undefined.
#include <cstdio>
#include <vector>

#include "../../hekaton_system_amd/csrc/job_args.h"

using namespace hk;

static void say(const char* name, hk_status st) {
    printf("%s %s\n", name, st == HK_OK ? "HK_OK" : st == HK_ERR_ARG ? "HK_ERR_ARG" : "OTHER");
}

int main() {
    // ---- the Poseidon pair: the reference's shapes, (8 + 56) x 4 + 16 = 272 leaf constants, then (8 + 33) x 3 + 9 = 132
    const hk_poseidon_desc leaf{4, 5, 8, 56, 0}, node{3, 17, 8, 33, 272};
    const size_t n_consts = 404;
    auto pair = [&](const char* name, hk_poseidon_desc l, hk_poseidon_desc n, size_t nc) { say(name, poseidon_pair_check(&l, &n, nc)); };
    hk_poseidon_desc x;
    pair("poseidon_valid", leaf, node, n_consts);
    x = leaf; x.t = 5;            pair("poseidon_leaf_t5", x, node, n_consts + 1000);
    x = leaf; x.alpha = 17;       pair("poseidon_leaf_alpha17", x, node, n_consts);
    x = node; x.t = 4;            pair("poseidon_node_t4", leaf, x, n_consts + 1000);
    x = node; x.alpha = 5;        pair("poseidon_node_alpha5", leaf, x, n_consts);
    x = leaf; x.full_rounds = 7;  pair("poseidon_odd_rounds", x, node, n_consts);
    x = node; x.full_rounds = 9;  pair("poseidon_node_odd_rounds", leaf, x, n_consts + 1000);
    pair("poseidon_consts_four_short", leaf, node, n_consts - 4);
    pair("poseidon_consts_one_short", leaf, node, n_consts - 1);
    x = leaf; x.full_rounds = x.partial_rounds = 0;  pair("poseidon_zero_rounds", x, node, n_consts);
    if (poseidon_trace_len(&leaf) != 8 * (4 * 3 + 4) + 56 * (3 + 4) || poseidon_trace_len(&node) != 8 * (3 * 5 + 3) + 33 * (5 + 3) ||
        poseidon_path_len(&leaf, &node, 3) != 2 * poseidon_trace_len(&leaf) + 3 * (3 + poseidon_trace_len(&node)))
        return 2;
    const PoseidonDesc pd = poseidon_desc(&node);
    if (pd.t != 3 || pd.alpha != 17 || pd.rf != 8 || pd.rp != 33 || pd.off != 272) return 2;

    // ---- offsets
    { const uint32_t o[] = {0, 2, 2, 5};  say("offsets_valid", offsets_check(o, 3)); }
    { const uint32_t o[] = {1, 2, 2, 5};  say("offsets_first_one", offsets_check(o, 3)); }
    { const uint32_t o[] = {0, 3, 2, 5};  say("offsets_decreasing", offsets_check(o, 3)); }
    { const uint32_t o[] = {0, 2, 4, 3};  say("offsets_decreasing_last", offsets_check(o, 3)); }

    // ---- rows: every selected subcircuit owns exactly K = 2 entries
    std::vector<uint32_t> rows;
    {
        const uint32_t o[] = {0, 2, 4, 6, 8}, sub[] = {3, 0, 3};
        say("rows_valid", portal_rows(o, 4, 2, sub, 3, rows));
        const uint32_t want[] = {3, 6, 0, 0, 3, 6};
        if (rows.size() != 6) return 3;
        for (int k = 0; k < 6; k++) if (rows[k] != want[k]) return 3;
        say("rows_empty_batch", portal_rows(o, 4, 2, nullptr, 0, rows));
        if (!rows.empty()) return 3;
        const uint32_t past[] = {0, 4};
        say("rows_sub_index_n_sub", portal_rows(o, 4, 2, past, 2, rows));
        const uint32_t first_one[] = {1, 2, 4, 6, 8};
        say("rows_offsets_first_one", portal_rows(first_one, 4, 2, sub, 3, rows));
    }
    {
        const uint32_t o[] = {0, 1, 4, 6}, s0[] = {2, 0}, s1[] = {2, 1}, s2[] = {2};
        say("rows_k_minus_1_entries", portal_rows(o, 3, 2, s0, 2, rows));
        say("rows_k_plus_1_entries", portal_rows(o, 3, 2, s1, 2, rows));
        say("rows_k_entries", portal_rows(o, 3, 2, s2, 1, rows));
    }

    // ---- tree shape
    say("tree_2_1", tree_shape_check(2, 1));
    say("tree_8_3", tree_shape_check(8, 3));
    say("tree_2p24", tree_shape_check((size_t)1 << 24, 24));
    say("tree_2p25", tree_shape_check((size_t)1 << 25, 25));
    say("tree_n_sub_0", tree_shape_check(0, 0));
    say("tree_n_sub_1", tree_shape_check(1, 0));
    say("tree_n_sub_3", tree_shape_check(3, 2));
    say("tree_n_sub_6", tree_shape_check(6, 3));
    say("tree_depth_minus_1", tree_shape_check(8, 2));
    say("tree_depth_plus_1", tree_shape_check(8, 4));

    // ---- column ranges of an assignment of n_v = 100 columns
    auto cols = [&](const char* name, size_t l0, size_t n0, size_t l1, size_t n1, size_t l2, size_t n2) {
        const size_t lo[3] = {l0, l1, l2}, len[3] = {n0, n1, n2};
        say(name, col_ranges_check(lo, len, 3, 100));
    };
    cols("cols_abutting_to_the_end", 1, 5, 6, 10, 16, 84);
    cols("cols_any_order", 16, 84, 1, 5, 6, 10);
    cols("cols_column_0", 0, 5, 6, 10, 16, 84);
    cols("cols_past_n_v_by_one", 1, 5, 6, 10, 16, 85);
    cols("cols_first_past_n_v", 101, 0, 6, 10, 16, 84);
    cols("cols_overlap_0_1", 1, 6, 6, 10, 16, 84);
    cols("cols_overlap_1_2", 1, 5, 6, 11, 16, 84);
    cols("cols_overlap_0_2", 15, 2, 1, 10, 16, 84);
    cols("cols_overlap_reordered", 16, 84, 6, 11, 1, 5);

    // ---- buffers
    static char buf[64];
    auto ov = [&](const char* name, const void* a, size_t al, const void* b, size_t bl) {
        say(name, bufs_overlap(a, al, b, bl) ? HK_ERR_ARG : HK_OK);
    };
    ov("bufs_one_byte", buf, 16, buf + 15, 16);
    ov("bufs_one_byte_swapped", buf + 15, 16, buf, 16);
    ov("bufs_abutting", buf, 16, buf + 16, 16);
    ov("bufs_abutting_swapped", buf + 16, 16, buf, 16);
    ov("bufs_same", buf, 16, buf, 16);
    ov("bufs_inside", buf, 64, buf + 20, 1);
    ov("bufs_null_a", nullptr, 16, buf, 16);
    ov("bufs_null_b", buf, 16, nullptr, 16);
    return 0;
}
