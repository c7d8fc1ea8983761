// vkd_tree.cuh — a VKD batch applied to the directory on the device (hk_vkd_tree): the sibling paths
// hk_vkd_desc.siblings_mont wants and the roots before and after the batch, from the directory's leaves and the batch's own.
// The host mirror is hekaton_system_amd/vkd_circuit.py `directory_paths`: a `SparseTree` (sparse_tree.rs:70-177) that takes
// one insert after the other.
//
// EVENTS in time order: the M initial leaves, then the U updates' new leaves; E = M + U; event e is (idx_e, leaf_e), idx the
// low `depth` bits of the username digest.  N(e, l): the node of height l above idx_e right after event e.
//     N(e, 0)     = leaf hash of leaf_e, cut to 216 bits
//     N(e, l + 1) = cut(H2(left, right)), {left, right} = {N(e, l), S(e, l)} by bit l of idx_e (1: the current node is the right child)
//     S(e, l)     = N(e', l) of the latest e' < e with (idx_e' >> l) == (idx_e >> l) ^ 1, else EMPTY[l]
// siblings[u][l] = S(M + u, l); roots = N(M - 1, depth) (EMPTY[depth] for M = 0), N(E - 1, depth).
//
// THE ORDER.  At level l the events are kept sorted by (idx >> l, event number): `ord` (position -> event) and, per position,
// the bounds [rs, re) of its run of equal prefix.  The sibling prefix's run, when there is one, is the next run (bit l = 0) or
// the one before (bit l = 1); both runs are sorted by event number, so a binary search of e in the sibling run gives c, the
// sibling events older than e: the predecessor is that run's element c - 1, and e's position at level l + 1 is (start of the
// merged pair) + (its rank in its own run) + c.  Level 0 is a stable LSD radix sort of the event numbers by idx (the passes of
// trace_sort.cuh over the 8 index planes); at level `depth` the order is the identity.
//
//   k_vt_empty   one quad: EMPTY[0 .. depth].
//   k_vt_events  one quad per event: the username digest's index words (planes, by event number, twice: the sort moves one copy)
//                and N(e, 0).
//   k_vt_runs    one lane per position of the level-0 order: its run's bounds (two binary searches over the sorted planes) and,
//                for an update event, its status - the element before it in its run holds the 66 bytes the index held.
//   k_vt_level   one quad per position: the search, the hash, the new position, the sibling store of an update event.  One
//                launch per level; N, ord, rs and re ping-pong between levels.
//   k_vt_small   E <= VT_WG_EVENTS: events, sort, runs and every level in ONE workgroup, a barrier between the steps.
// A quad past the end recomputes the last one and stores nothing.  No limb or key array is indexed by a
// run-time value: no private memory.
#pragma once
#include "trace_sort.cuh"
#include "vkd.cuh"

namespace hk {

constexpr u32 VT_WG_EVENTS = 64;                     // events of one 256-lane workgroup (a quad each)
constexpr u32 VT_KEY_WORDS = 8;                      // index planes: a digest's limbs, zero from bit `depth` up
constexpr size_t VT_MAX_UPDATES = (size_t)1 << 20, VT_MAX_EVENTS = (size_t)1 << 22;

#if defined(__HIPCC__)

// the 66 bytes of event e: initial leaf e, or leaf_new of update e - M
__device__ __forceinline__ const unsigned char* vt_leaf(const unsigned char* leaves0, const unsigned char* leaves, u32 M, u32 e) {
    return e < M ? leaves0 + (size_t)e * VKD_LEAF_BYTES : leaves + ((size_t)(e - M) * 2 + 1) * VKD_LEAF_BYTES;
}

// event e on a quad: idx[k E + e] = key[k E + e] = word k of its index, ord[e] = e, node[e] = N(e, 0)
template <class Fr>
__device__ __forceinline__ void vt_event(const Fr* consts, const PoseidonDesc& leaf_d, const unsigned char* p, u32 e, u32 E,
                                         u32 depth, bool store, u32* idx, u32* key, u32* ord, Fr* node) {
    const u32 q = threadIdx.x & 3u;
    const Fr d = Fr::from_mont(vkd_hash_quad<Fr>(consts, leaf_d, p, VKD_NAME_BYTES));
    HK_UNROLL for (u32 h = 0; h < 2; h++) {
        const u32 k = q + 4 * h;
        const u32 have = depth > 32u * k ? depth - 32u * k : 0u;                 // bits of this word below `depth`
        const u32 w = vkd_limb(d, k) & (have >= 32u ? ~0u : (1u << have) - 1u);
        if (store) idx[(size_t)k * E + e] = w;
        if (store) key[(size_t)k * E + e] = w;
    }
    if (store && q == 0) ord[e] = e;
    const Fr h = Fr::from_mont(vkd_hash_quad<Fr>(consts, leaf_d, p, VKD_LEAF_BYTES));
    if (store && q == 0) fr_store(&node[e], Fr::to_mont(vkd_mask_node(h)));
}

// position p of the level-0 order (key: the sorted planes): rs[p], re[p] = the bounds of its run of equal index; status of an
// update event.  In front of p every key is at most p's and behind it at least, so both searches test equality only.
__device__ __forceinline__ void vt_runs(const u32* key, const u32* ord, u32 p, u32 E, u32 M, const unsigned char* leaves0,
                                        const unsigned char* leaves, const u32* kinds, u32* rs, u32* re, unsigned char* status) {
    u32 mine[VT_KEY_WORDS];
    HK_UNROLL for (u32 k = 0; k < VT_KEY_WORDS; k++) mine[k] = key[(size_t)k * E + p];
    u32 lo = 0, hi = p;                                                          // the first position of my key, in [0, p]
    HK_NOUNROLL while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        u32 diff = 0;
        HK_UNROLL for (u32 k = 0; k < VT_KEY_WORDS; k++) diff |= key[(size_t)k * E + mid] ^ mine[k];
        lo = diff ? mid + 1 : lo;
        hi = diff ? hi : mid;
    }
    const u32 first = lo;
    lo = p + 1, hi = E;                                                          // the first position of a larger key, in (p, E]
    HK_NOUNROLL while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        u32 diff = 0;
        HK_UNROLL for (u32 k = 0; k < VT_KEY_WORDS; k++) diff |= key[(size_t)k * E + mid] ^ mine[k];
        hi = diff ? mid : hi;
        lo = diff ? lo : mid + 1;
    }
    rs[p] = first;
    re[p] = lo;
    const u32 e = ord[p];
    if (status && e >= M) {
        const u32 u = e - M;
        const bool has = first < p;                                              // the run is in event order: p - 1 is the latest
        const unsigned char* cur = vt_leaf(leaves0, leaves, M, ord[has ? p - 1 : p]);
        const unsigned char* old = leaves + (size_t)u * 2 * VKD_LEAF_BYTES;
        u32 diff = 0;
        HK_NOUNROLL for (u32 j = 0; j < VKD_LEAF_BYTES; j++) diff |= (u32)cur[j] ^ (u32)old[j];
        const u32 st_append = has ? HK_VKD_ST_OCCUPIED : HK_VKD_ST_OK;
        const u32 st_update = !has ? HK_VKD_ST_ABSENT : (diff ? HK_VKD_ST_STALE : HK_VKD_ST_OK);
        status[u] = (unsigned char)(kinds[u] == HK_VKD_APPEND ? st_append : st_update);
    }
}

// position t of the level-l order on a quad: S(e, l) and N(e, l + 1) of its event e, e's position at level l + 1 with the bounds
// of its merged run there, and S into the siblings of an update event.  nin / nout: N(., l) / N(., l + 1) by event number.
template <class Fr>
__device__ __forceinline__ void vt_level(const Fr* consts, const PoseidonDesc& node_d, const u32* idx, u32 E, u32 M, u32 depth, u32 l,
                                         u32 t, bool store, const u32* ord, const u32* rs, const u32* re, const Fr* nin,
                                         const Fr* empty, u32* ord_o, u32* rs_o, u32* re_o, Fr* nout, Fr* sib_out) {
    const u32 q = threadIdx.x & 3u;
    const u32 e = ord[t], s = rs[t], end = re[t];
    const bool bit = (idx[(size_t)(l >> 5) * E + e] >> (l & 31u)) & 1u;
    // the run that may be the sibling prefix's: the next one for a left child, the one before for a right child
    const bool has_nb = bit ? s > 0 : end < E;
    const u32 nb = has_nb ? (bit ? s - 1 : end) : t;
    const u32 e2 = ord[nb], nb_s = rs[nb], nb_e = re[nb];
    // it is when both have one parent: bits [l + 1, depth) agree - whole words, the lowest one shifted
    const u32 w0 = (l + 1) >> 5, sh = (l + 1) & 31u;
    u32 diff = 0;
    HK_UNROLL for (u32 k = 0; k < VT_KEY_WORDS; k++) {
        if (k >= w0 && 32u * k < depth) {                                        // the same in the whole grid
            const u32 x = idx[(size_t)k * E + e] ^ idx[(size_t)k * E + e2];
            diff |= k == w0 ? x >> sh : x;
        }
    }
    const bool sib = has_nb && diff == 0;
    const u32 ss = bit ? nb_s : end, se = bit ? s : nb_e;                        // the sibling run, when sib
    u32 lo = ss, hi = sib ? (se < E ? se : E) : ss;                              // its events older than e: [ss, lo)
    HK_NOUNROLL while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        const bool older = ord[mid] < e;
        lo = older ? mid + 1 : lo;
        hi = older ? hi : mid;
    }
    const u32 c = lo - ss;
    const u32 pred = ord[c ? lo - 1 : t];
    const Fr sv = fr_load(c ? &nin[pred] : &empty[l]);
    const Fr cur = fr_load(&nin[e]);
    const Fr left = fr_select(bit, sv, cur), right = fr_select(bit, cur, sv);
    const Fr st = poseidon_permute_quad<Fr, 3, 17>(consts, node_d, poseidon_pair_input(left, right));
    const Fr nxt = Fr::to_mont(vkd_mask_node(Fr::from_mont(quad_bcast<Fr, 0x55>(st))));
    const u32 ps = sib && bit ? ss : s, pe = sib && !bit ? se : end;             // the merged run
    const u32 np = ps + (t - s) + c;
    if (store && q == 0 && np < E) {                                             // np < E: a permutation of the positions
        ord_o[np] = e;
        rs_o[np] = ps;
        re_o[np] = pe;
        fr_store(&nout[e], nxt);
        if (e >= M) fr_store(&sib_out[(size_t)(e - M) * depth + l], sv);
    }
}

// EMPTY[0] = the leaf hash of 32 zero bytes, EMPTY[l + 1] = cut(H2(EMPTY[l], EMPTY[l])): every quad of the wave walks the one
// chain, lane 0 stores
template <class Fr>
__global__ void __launch_bounds__(64)
k_vt_empty(const Fr* __restrict__ consts, PoseidonDesc leaf_d, PoseidonDesc node_d, const unsigned char* __restrict__ zeros,
           u32 depth, Fr* __restrict__ empty) {
    const bool writer = threadIdx.x == 0;
    Fr cur = Fr::to_mont(vkd_mask_node(Fr::from_mont(vkd_hash_quad<Fr>(consts, leaf_d, zeros, VKD_NAME_BYTES))));
    if (writer) fr_store(&empty[0], cur);
    HK_NOUNROLL for (u32 l = 0; l < depth; l++) {
        const Fr s = poseidon_permute_quad<Fr, 3, 17>(consts, node_d, poseidon_pair_input(cur, cur));
        cur = Fr::to_mont(vkd_mask_node(Fr::from_mont(quad_bcast<Fr, 0x55>(s))));
        if (writer) fr_store(&empty[l + 1], cur);
    }
}

template <class Fr>
__global__ void __launch_bounds__(256)
k_vt_events(const Fr* consts, PoseidonDesc leaf_d, const unsigned char* leaves0, const unsigned char* leaves, u32 M, u32 E, u32 depth,
            u32* idx, u32* key, u32* ord, Fr* node) {
    const u32 t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const bool store = t < E;
    const u32 e = store ? t : E - 1;
    vt_event<Fr>(consts, leaf_d, vt_leaf(leaves0, leaves, M, e), e, E, depth, store, idx, key, ord, node);
}

template <int UNUSED>
__global__ void __launch_bounds__(256)
k_vt_runs(const u32* key, const u32* ord, u32 E, u32 M, const unsigned char* leaves0, const unsigned char* leaves, const u32* kinds,
          u32* rs, u32* re, unsigned char* status) {
    const u32 p = blockIdx.x * 256 + threadIdx.x;
    if (p < E) vt_runs(key, ord, p, E, M, leaves0, leaves, kinds, rs, re, status);
}

template <class Fr>
__global__ void __launch_bounds__(256)
k_vt_level(const Fr* consts, PoseidonDesc node_d, const u32* idx, u32 E, u32 M, u32 depth, u32 l, const u32* ord, const u32* rs,
           const u32* re, const Fr* nin, const Fr* empty, u32* ord_o, u32* rs_o, u32* re_o, Fr* nout, Fr* sib_out) {
    const u32 t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const bool store = t < E;
    vt_level<Fr>(consts, node_d, idx, E, M, depth, l, store ? t : E - 1, store, ord, rs, re, nin, empty, ord_o, rs_o, re_o, nout,
                 sib_out);
}

// The whole call for E <= VT_WG_EVENTS in ONE workgroup, a barrier between the steps (as k_ts_small and k_et_tree_tail do).
// k? / o? / rs? / re? / n?: the ping-pong buffers; after depth / 8 passes and depth levels the results lie where the host's own
// count of swaps says.
template <class Fr>
__global__ void __launch_bounds__(256)
k_vt_small(const Fr* consts, PoseidonDesc leaf_d, PoseidonDesc node_d, const unsigned char* leaves0, const unsigned char* leaves,
           const u32* kinds, u32 M, u32 E, u32 depth, const Fr* empty, u32* idx, u32* ka, u32* kb, u32* oa, u32* ob, u32* rsa,
           u32* rsb, u32* rea, u32* reb, Fr* na, Fr* nb, Fr* sib_out, unsigned char* status) {
    __shared__ u32 cnt[4 * 256], woff[4 * 256], sc[256];
    const u32 tid = threadIdx.x;
    const bool store = (tid >> 2) < E;
    const u32 t = store ? tid >> 2 : E - 1;
    vt_event<Fr>(consts, leaf_d, vt_leaf(leaves0, leaves, M, t), t, E, depth, store, idx, ka, oa, na);
    __syncthreads();
    HK_NOUNROLL for (u32 p = 0; p < depth / 8; p++) {
        ts_tile_pass<(int)VT_KEY_WORDS>(ka, oa, kb, ob, E, 0, E, p >> 2, (p & 3u) * 8, nullptr, 1, 0, cnt, woff, sc);
        u32* x = ka; ka = kb; kb = x;
        x = oa; oa = ob; ob = x;
    }
    if (tid < E) vt_runs(ka, oa, tid, E, M, leaves0, leaves, kinds, rsa, rea, status);
    __syncthreads();
    HK_NOUNROLL for (u32 l = 0; l < depth; l++) {
        vt_level<Fr>(consts, node_d, idx, E, M, depth, l, t, store, oa, rsa, rea, na, empty, ob, rsb, reb, nb, sib_out);
        __syncthreads();
        u32* x = oa; oa = ob; ob = x;
        x = rsa; rsa = rsb; rsb = x;
        x = rea; rea = reb; reb = x;
        Fr* y = na; na = nb; nb = y;
    }
}

#endif  // __HIPCC__

template <class C>
hk_status Ops<C>::vkd_tree(hk_ctx* ctx, const hk_vkd_tree_desc* d, void* siblings_out, void* roots_out, uint8_t* status_out) {
    if (!d || !d->kinds || !d->leaves || !d->consts_mont || !d->leaf_hash || !d->node_hash || !siblings_out || !roots_out)
        return HK_ERR_ARG;
    const size_t M = d->n_leaves0, U = d->n_updates, E = M + U, depth = d->depth, fr = sizeof(Fr);
    if (M && !d->leaves0) return HK_ERR_ARG;
    if (depth < 16 || depth > 256 || depth % 8) return HK_ERR_ARG;
    if (U == 0 || U > VT_MAX_UPDATES) return HK_ERR_ARG;
    if (E > VT_MAX_EVENTS) return HK_ERR_LEN;                                  // 4 E lanes, E x depth siblings: below 2^31
    for (size_t u = 0; u < U; u++)
        if (d->kinds[u] != HK_VKD_APPEND && d->kinds[u] != HK_VKD_UPDATE) return HK_ERR_ARG;
    HK_TRY(poseidon_pair_check(d->leaf_hash, d->node_hash, d->n_consts));
    Staged in[3] = {staged(M ? d->leaves0 : nullptr, M * VKD_LEAF_BYTES), staged(d->leaves, U * 2 * VKD_LEAF_BYTES),
                    staged(d->consts_mont, d->n_consts * fr)};
    Staged out[3] = {staged(siblings_out, U * depth * fr), staged(roots_out, 2 * fr), staged(status_out, U)};
    for (int a = 0; a < 3; a++) {
        for (const Staged& x : in)
            if (bufs_overlap(out[a].buf, out[a].bytes, x.buf, x.bytes)) return HK_ERR_ARG;
        if (bufs_overlap(out[a].buf, out[a].bytes, d->kinds, 4 * U)) return HK_ERR_ARG;
        for (int b = 0; b < a; b++)
            if (bufs_overlap(out[a].buf, out[a].bytes, out[b].buf, out[b].bytes)) return HK_ERR_ARG;
    }
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    const u32 ne = (u32)E, nm = (u32)M, nd = (u32)depth;
    const bool small = E <= VT_WG_EVENTS;
    const u32 n_tiles = (ne + TS_TILE - 1) / TS_TILE, n_hist = 256 * n_tiles;
    u32 *kinds_d, *idx, *key[2], *ord[2], *rs[2], *re[2], *hist, *gbase, *tops;
    Fr *node[2], *empty;
    unsigned char* zeros_d;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, in, 3);
        kinds_d = c.n<u32>(U);
        idx = c.n<u32>(VT_KEY_WORDS * E);
        for (int k = 0; k < 2; k++) key[k] = c.n<u32>(VT_KEY_WORDS * E);
        for (int k = 0; k < 2; k++) ord[k] = c.n<u32>(E);
        for (int k = 0; k < 2; k++) rs[k] = c.n<u32>(E);
        for (int k = 0; k < 2; k++) re[k] = c.n<u32>(E);
        hist = c.n<u32>(n_hist);
        gbase = c.n<u32>(n_hist);
        tops = c.n<u32>(scan_u32_tops_len(n_hist));
        for (int k = 0; k < 2; k++) node[k] = c.n<Fr>(E);
        empty = c.n<Fr>(depth + 1);
        zeros_d = (unsigned char*)c.n<u32>(VKD_NAME_BYTES / 4);
        stage_carve(c, out, 3);
    }));
    hipStream_t s = L->stream;
    HK_TRY(stage_upload(L, in, 3));
    HK_HIP(hipMemcpyAsync(kinds_d, d->kinds, 4 * U, hipMemcpyHostToDevice, s));
    HK_HIP(hipMemsetAsync(zeros_d, 0, VKD_NAME_BYTES, s));
    const unsigned char *leaves0 = (const unsigned char*)in[0].p, *leaves = (const unsigned char*)in[1].p;
    const Fr* consts = (const Fr*)in[2].p;
    Fr* sib_d = (Fr*)out[0].p;
    unsigned char* status_d = (unsigned char*)out[2].p;
    const PoseidonDesc a = poseidon_desc(d->leaf_hash), b = poseidon_desc(d->node_hash);
    const u32 passes = nd / 8;
    HK_LAUNCH((k_vt_empty<Fr>), dim3(1), dim3(64), 0, s, consts, a, b, (const unsigned char*)zeros_d, nd, empty);
    int ko = 0, lv = 0;                                     // which of key / ord, and of ord / rs / re / node, is current
    if (small) {
        HK_LAUNCH((k_vt_small<Fr>), dim3(1), dim3(256), 0, s, consts, a, b, leaves0, leaves, (const u32*)kinds_d, nm, ne, nd,
                  (const Fr*)empty, idx, key[0], key[1], ord[0], ord[1], rs[0], rs[1], re[0], re[1], node[0], node[1], sib_d,
                  status_d);
        lv = (int)(nd & 1u);                               // node: one swap per level (ord is not read again)
    } else {
        HK_LAUNCH((k_vt_events<Fr>), dim3((ne + 63) / 64), dim3(256), 0, s, consts, a, leaves0, leaves, nm, ne, nd, idx,
                  key[0], ord[0], node[0]);
        for (u32 p = 0; p < passes; p++) {
            const u32 word = p >> 2, shift = (p & 3u) * 8;
            const u32* gb = nullptr;
            if (n_tiles > 1) {
                HK_LAUNCH((k_ts_hist<0>), dim3(n_tiles), dim3(256), 0, s, (const u32*)key[ko] + (size_t)word * E, ne, shift,
                          n_tiles, hist);
                HK_TRY(scan_u32(s, hist, gbase, tops, n_hist));
                gb = gbase;
            }
            HK_LAUNCH((k_ts_scatter<(int)VT_KEY_WORDS>), dim3(n_tiles), dim3(256), 0, s, (const u32*)key[ko],
                      (const u32*)ord[ko], key[ko ^ 1], ord[ko ^ 1], ne, word, shift, gb, n_tiles);
            ko ^= 1;
        }
        // the levels' ord starts where the sort left it; rs / re / node start at 0
        HK_LAUNCH((k_vt_runs<0>), dim3((ne + 255) / 256), dim3(256), 0, s, (const u32*)key[ko], (const u32*)ord[ko], ne, nm,
                  leaves0, leaves, (const u32*)kinds_d, rs[0], re[0], status_d);
        for (u32 l = 0; l < nd; l++) {
            HK_LAUNCH((k_vt_level<Fr>), dim3((ne + 63) / 64), dim3(256), 0, s, consts, b, (const u32*)idx, ne, nm, nd, l,
                      (const u32*)ord[ko], (const u32*)rs[lv], (const u32*)re[lv], (const Fr*)node[lv], (const Fr*)empty,
                      ord[ko ^ 1], rs[lv ^ 1], re[lv ^ 1], node[lv ^ 1], sib_d);
            ko ^= 1;
            lv ^= 1;
        }
    }
    Fr* roots_d = (Fr*)out[1].p;
    HK_HIP(hipMemcpyAsync(roots_d, M ? node[lv] + (M - 1) : empty + depth, fr, hipMemcpyDeviceToDevice, s));
    HK_HIP(hipMemcpyAsync(roots_d + 1, node[lv] + (E - 1), fr, hipMemcpyDeviceToDevice, s));
    HK_TRY(stage_download(L, out, 3));
    return L->settle();
}

}  // namespace hk
