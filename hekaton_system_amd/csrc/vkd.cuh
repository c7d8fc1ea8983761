// vkd.cuh — the verifiable key directory job on the device (hk_vkd_trace / hk_vkd_witness): the
// time-ordered ROM trace of distributed-prover/src/vkd/vkd_constraints.rs:70-193 `get_portal_subtraces` and the body columns
// of a subcircuit's assignment (:237-342), both from the updates where they lie.  The job is
// hekaton_system_amd/vkd_circuit.py `VkdJob`; the tables of hk_vkd_desc are its `tables()`.
//
// The VALUE TABLE holds every traced value once, V = 3 + U (2 + 3 split) Fr:
//     0 initial root   1 final root   2 null leaf
//     base(u) = 3 + u (2 + 3 split):   + 0 hash of leaf_old (0 for an append)   + 1 hash of leaf_new
//                                      + 2 + s index word s                     + 2 + split + p split + s node after segment s of path p
// and entry e of the flattened trace is (slot_addr[e], values[slot_src[e]]), 0 for HK_VKD_SRC_ZERO.
//
//   k_vkd_hash     one quad per leaf / username hash (3 per update and the null leaf's): the bytes' 27-byte chunks on lanes
//                  1 .. 3, one rate-3 permutation (poseidon_permute_quad), the digest out of Montgomery form, cut to 216
//                  bits (a node) or into the `split` index words.
//   k_vkd_chain    one quad per (update, path): `depth` dependent two-to-one hashes, each followed by from_mont -> mask to
//                  216 bits -> to_mont; the node after every segment is stored.
//   k_vkd_trace    one lane per Fr of the trace, Fr fastest, as k_rj_trace.
//   k_vkd_one      column 0 of every row <- the constant 1.
//   k_vkd_leaf_bits  one lane per (row, bit column of the leaf), column fastest.
//   k_vkd_body     one quad per (row, primitive chain), the chain a grid row: a leaf hash, a username hash or the L hashes of
//                  a segment, with every S-box chain value and round state stored in poseidon_path_trace order
//                  (poseidon_permute_quad with TRACE) and the `bits` / `canon` columns from integer tests of the canonical limbs.
// A quad past the end recomputes the last one and stores nothing: every lane of a quad is in every DPP exchange, only stores
// are guarded.  No limb array is indexed by a run-time value: no private memory.
#pragma once
#include "curve_ops_impl.cuh"
#include "poseidon.cuh"

namespace hk {

constexpr u32 VKD_LEAF_BYTES = 66, VKD_NAME_BYTES = 32, VKD_CHUNK_BYTES = 27;     // a node: the low 8 x 27 = 216 bits of a digest
constexpr u32 VKD_GRID_ROWS = 65535;    // rows of one k_vkd_leaf_bits launch: the y extent of a grid
enum : u32 { VKD_K_PADDING = 0, VKD_K_WRITE_PP, VKD_K_HGC, VKD_K_C, VKD_K_CE, VKD_K_EHC, VKD_K_EQUALITY, VKD_K_COUNT };

// bits of the modulus, and the columns of the `canon` block: one per 1 bit of r - 1 below the top bit
template <class Fr> constexpr u32 vkd_mod_limb(int k) { return k == 0 ? Fr::Params::MOD[0] - 1u : Fr::Params::MOD[k]; }
template <class Fr> constexpr u32 vkd_nbits() {
    u32 n = 0;
    for (int k = 0; k < Fr::N; k++)
        for (u32 b = 0; b < 32; b++)
            if ((Fr::Params::MOD[k] >> b) & 1u) n = 32 * k + b + 1;
    return n;
}
template <class Fr> constexpr u32 vkd_ncanon() {
    u32 n = 0;
    for (int k = 0; k < Fr::N; k++)
        for (u32 b = 0; b < 32; b++)
            if (32 * k + b + 1 < vkd_nbits<Fr>() && ((vkd_mod_limb<Fr>(k) >> b) & 1u)) n++;
    return n;
}

// what one row of k_vkd_body reads: its segment's first sibling, the value-table indices of the node it starts from and of
// its index word, and the byte offset of its leaf
struct VkdRow { u32 sib_off, init_src, word_src, leaf_off; };

#if defined(__HIPCC__)

// limb i of x for a run-time i (0 past the end): a select chain, not an indexed load
template <class Fr>
__device__ __forceinline__ u32 vkd_limb(const Fr& x, u32 i) {
    u32 r = 0;
    HK_UNROLL for (int k = 0; k < Fr::N; k++) r = i == (u32)k ? x.v[k] : r;
    return r;
}

// the low 216 bits of a canonical integer
template <class Fr>
__device__ __forceinline__ Fr vkd_mask_node(Fr d) {
    d.v[6] &= 0x00FFFFFFu;
    d.v[7] = 0;
    return d;
}

// bits [lo, lo + len) of a canonical integer, lo and len multiples of 8, len <= 128
template <class Fr>
__device__ __forceinline__ Fr vkd_word(const Fr& d, u32 lo, u32 len) {
    Fr r = Fr::zero();
    const u32 i0 = lo >> 5, sh = lo & 31u;
    HK_UNROLL for (int k = 0; k < 4; k++) {
        const u32 a = vkd_limb(d, i0 + k), b = vkd_limb(d, i0 + k + 1);
        const u32 x = (a >> sh) | ((b << 1) << (31u - sh));          // sh = 0: nothing of b
        const u32 have = len > 32u * k ? len - 32u * k : 0u;         // bits of this limb that belong to the word
        r.v[k] = have >= 32u ? x : x & ((1u << have) - 1u);
    }
    return r;
}

// chunk c of `n` bytes at p as a canonical integer: bytes [27 c, min(27 c + 27, n)), little-endian; 0 when none are left.
// Every load is of a byte inside [p, p + n).
template <class Fr>
__device__ __forceinline__ Fr vkd_chunk(const unsigned char* __restrict__ p, u32 n, u32 c) {
    Fr r = Fr::zero();
    const u32 off = c * VKD_CHUNK_BYTES;
    HK_UNROLL for (int j = 0; j < (int)VKD_CHUNK_BYTES; j++) {
        const bool in = off + j < n;
        const u32 byte = p[in ? off + j : 0u];
        r.v[j >> 2] |= (in ? byte : 0u) << (8 * (j & 3));
    }
    return r;
}

// the rate-3 hash of `n` bytes (n <= 81: one permutation) on a quad; the digest in Montgomery form on every lane
template <class Fr>
__device__ __forceinline__ Fr vkd_hash_quad(const Fr* __restrict__ consts, const PoseidonDesc& d, const unsigned char* __restrict__ p,
                                            u32 n) {
    const u32 q = threadIdx.x & 3u;
    const Fr c = Fr::to_mont(vkd_chunk<Fr>(p, n, q ? q - 1 : 0u));
    Fr s = poseidon_permute_quad<Fr, 4, 5>(consts, d, fr_select(q != 0, c, Fr::zero()));
    return quad_bcast<Fr, 0x55>(s);
}

// jobs of k_vkd_hash: 0 the null leaf (32 zero bytes: `zeros`); 1 + 3 u + j: j = 0 leaf_old, 1 leaf_new, 2 the username
template <class Fr>
__global__ void __launch_bounds__(256)
k_vkd_hash(const Fr* __restrict__ consts, PoseidonDesc leaf_d, const unsigned char* __restrict__ leaves,
           const unsigned char* __restrict__ zeros, const u32* __restrict__ kinds, u32 n_updates, u32 split, u32 L,
           Fr* __restrict__ values, u32* __restrict__ index_raw) {
    const u32 t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2, q = threadIdx.x & 3u;
    const u32 n_jobs = 1 + 3 * n_updates;
    const bool store = t < n_jobs;
    const u32 job = store ? t : n_jobs - 1;
    const u32 u = job ? (job - 1) / 3 : 0u, j = job ? (job - 1) - 3 * u : 0u;
    const unsigned char* p = job ? leaves + ((size_t)u * 2 + (j ? 1 : 0)) * VKD_LEAF_BYTES : zeros;
    const u32 n = job && j < 2 ? VKD_LEAF_BYTES : VKD_NAME_BYTES;
    const Fr d = Fr::from_mont(vkd_hash_quad<Fr>(consts, leaf_d, p, n));
    const u32 base = 3 + u * (2 + 3 * split);
    if (job == 0 || j < 2) {
        // an append has no old leaf: its entry is 0
        const bool none = job && j == 0 && kinds[u] == HK_VKD_APPEND;
        const Fr node = fr_select(none, Fr::zero(), Fr::to_mont(vkd_mask_node(d)));
        if (store && q == 0) fr_store(&values[job ? base + j : 2u], node);
    } else {
        HK_NOUNROLL for (u32 s0 = 0; s0 < split; s0 += 4) {
            const u32 s = s0 + q;
            const Fr w = Fr::to_mont(vkd_word(d, (s < split ? s : 0u) * L, L));
            if (store && s < split) fr_store(&values[base + 2 + s], w);
        }
        if (store) index_raw[(size_t)u * 8 + q] = vkd_limb(d, q);          // the digest's canonical limbs: k_vkd_chain's bits
        if (store) index_raw[(size_t)u * 8 + 4 + q] = vkd_limb(d, 4 + q);
    }
}

// quad t: path p = t & 1 of update u = t >> 1
template <class Fr>
__global__ void __launch_bounds__(256)
k_vkd_chain(const Fr* __restrict__ consts, PoseidonDesc node_d, const Fr* __restrict__ siblings, const u32* __restrict__ kinds,
            const u32* __restrict__ index_raw, u32 n_updates, u32 depth, u32 split, u32 L, Fr* __restrict__ values) {
    const u32 t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2, q = threadIdx.x & 3u;
    const bool store = t < 2 * n_updates;
    const u32 c = store ? t : 2 * n_updates - 1;
    const u32 u = c >> 1, p = c & 1u;
    const u32 base = 3 + u * (2 + 3 * split);
    const u32 from = p ? base + 1 : (kinds[u] == HK_VKD_UPDATE ? base : 2u);
    Fr cur = fr_load(&values[from]);
    Fr* out = values + base + 2 + split + p * split;
    u32 in_seg = 0;
    HK_NOUNROLL for (u32 l = 0; l < depth; l++) {
        const Fr sib = fr_load(&siblings[(size_t)u * depth + l]);
        const bool bit = (index_raw[(size_t)u * 8 + (l >> 5)] >> (l & 31u)) & 1u;
        const Fr left = fr_select(bit, sib, cur), right = fr_select(bit, cur, sib);
        Fr s = poseidon_permute_quad<Fr, 3, 17>(consts, node_d, poseidon_pair_input(left, right));
        cur = Fr::to_mont(vkd_mask_node(Fr::from_mont(quad_bcast<Fr, 0x55>(s))));
        if (++in_seg == L) {                                             // uniform over the grid
            if (store && q == 0) fr_store(out, cur);
            out++;
            in_seg = 0;
        }
    }
}

template <class Fr>
__global__ void __launch_bounds__(256)
k_vkd_trace(const Fr* __restrict__ values, const u32* __restrict__ slot_addr, const u32* __restrict__ slot_src, u32 n_fr,
            Fr* __restrict__ out) {
    const u32 t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_fr) return;
    const u32 e = t >> 1;
    const bool is_val = t & 1u;
    const u32 k = slot_src[e];
    const Fr v = fr_load(&values[k != HK_VKD_SRC_ZERO ? k : 0u]);          // both lanes of an entry load
    Fr a = Fr::zero();
    a.v[0] = slot_addr[e];
    a = Fr::to_mont(a);
    fr_store(&out[t], fr_select(is_val, fr_select(k != HK_VKD_SRC_ZERO, v, Fr::zero()), a));
}

// ---- the body columns --------------------------------------------------------------------------------------------------
// the digest's `bits` and `canon` columns at w (vkd_nbits + vkd_ncanon of them) from its canonical limbs: lane q of the quad
// stores every fourth column.  canon: from the top bit down, e = "every bit at a 1 of r - 1 so far is 1"; one column per 1
// of r - 1 below the top.
template <class Fr>
__device__ __forceinline__ void vkd_digest_cols(const Fr& d, Fr* __restrict__ w, bool store) {
    constexpr u32 NB = vkd_nbits<Fr>();
    const u32 q = threadIdx.x & 3u;
    HK_UNROLL for (int k = 0; k < Fr::N; k++) {
        HK_NOUNROLL for (u32 b = 0; b < 32; b++) {
            const u32 i = 32 * k + b;
            if (store && i < NB && (i & 3u) == q) fr_store(&w[i], ((d.v[k] >> b) & 1u) ? Fr::one() : Fr::zero());
        }
    }
    Fr* c = w + NB;
    u32 e = 1, n = 0;
    HK_UNROLL for (int k = Fr::N - 1; k >= 0; k--) {
        const u32 m = vkd_mod_limb<Fr>(k);
        HK_NOUNROLL for (u32 bb = 0; bb < 32; bb++) {
            const u32 b = 31u - bb, i = 32 * k + b;
            if (i < NB && ((m >> b) & 1u)) {                            // the same on every lane
                e &= (d.v[k] >> b) & 1u;
                if (i != NB - 1) {
                    if (store && (n & 3u) == q) fr_store(&c[n], e ? Fr::one() : Fr::zero());
                    n++;
                }
            }
        }
    }
}

// column 0 of every row <- 1
template <class Fr>
__global__ void __launch_bounds__(256) k_vkd_one(u32 batch, size_t n_v, Fr* __restrict__ z) {
    const u32 b = blockIdx.x * 256 + threadIdx.x;
    if (b < batch) fr_store(&z[(size_t)b * n_v], Fr::one());
}

// row blockIdx.y, bit column blockIdx.x * 256 + threadIdx.x of its leaf: bytes in order, bits little-endian per byte
template <class Fr>
__global__ void __launch_bounds__(256)
k_vkd_leaf_bits(const unsigned char* __restrict__ leaves, const VkdRow* __restrict__ rows, size_t n_v, size_t col0,
                Fr* __restrict__ z) {
    const u32 c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= 8 * VKD_LEAF_BYTES) return;
    const u32 byte = leaves[(size_t)rows[b].leaf_off + (c >> 3)];
    fr_store(&z[(size_t)b * n_v + col0 + c], ((byte >> (c & 7u)) & 1u) ? Fr::one() : Fr::zero());
}

// chain blockIdx.y of the class: CH_HASH the leaf hash at hash_col0 + 528, CH_INDEX the username hash at index_col0, CH_PATH
// the segment at path_col0.  which[y] names chain y.
enum : u32 { VKD_CH_HASH = 0, VKD_CH_INDEX = 1, VKD_CH_PATH = 2 };
struct VkdChains { u32 which[3]; u32 col0[3]; };

template <class Fr>
__global__ void __launch_bounds__(256)
k_vkd_body(const Fr* __restrict__ consts, PoseidonDesc leaf_d, PoseidonDesc node_d, const unsigned char* __restrict__ leaves,
           const Fr* __restrict__ siblings, const Fr* __restrict__ values, const VkdRow* __restrict__ rows, VkdChains ch, u32 L,
           u32 batch, size_t n_v, Fr* __restrict__ z_out) {
    constexpr u32 NB = vkd_nbits<Fr>(), NC = vkd_ncanon<Fr>();
    const u32 t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2, q = threadIdx.x & 3u;
    const bool store = t < batch;
    const u32 b = store ? t : batch - 1;
    const VkdRow row = rows[b];
    const u32 which = ch.which[blockIdx.y];                               // the same in the whole workgroup
    Fr* w = z_out + (size_t)b * n_v + ch.col0[blockIdx.y];
    if (which != VKD_CH_PATH) {
        const u32 n = which == VKD_CH_HASH ? VKD_LEAF_BYTES : VKD_NAME_BYTES;
        const Fr c = Fr::to_mont(vkd_chunk<Fr>(leaves + row.leaf_off, n, q ? q - 1 : 0u));
        Fr s = poseidon_permute_quad<Fr, 4, 5, true>(consts, leaf_d, fr_select(q != 0, c, Fr::zero()), store, w);
        vkd_digest_cols<Fr>(Fr::from_mont(quad_bcast<Fr, 0x55>(s)), w, store);
        return;
    }
    Fr cur = fr_load(&values[row.init_src]);
    const Fr word = Fr::from_mont(fr_load(&values[row.word_src]));
    HK_NOUNROLL for (u32 l0 = 0; l0 < L; l0 += 4) {
        const u32 l = l0 + q;
        const bool bit = (vkd_limb(word, l >> 5) >> (l & 31u)) & 1u;
        if (store && l < L) fr_store(&w[l], bit ? Fr::one() : Fr::zero());
    }
    w += L;
    HK_NOUNROLL for (u32 l = 0; l < L; l++) {
        const Fr sib = fr_load(&siblings[(size_t)row.sib_off + l]);
        const bool bit = (vkd_limb(word, l >> 5) >> (l & 31u)) & 1u;
        const Fr left = fr_select(bit, sib, cur), right = fr_select(bit, cur, sib);
        if (store && q < 2) fr_store(&w[q], fr_select(q == 0, sib, left));
        w += 2;
        Fr s = poseidon_permute_quad<Fr, 3, 17, true>(consts, node_d, poseidon_pair_input(left, right), store, w);
        const Fr d = Fr::from_mont(quad_bcast<Fr, 0x55>(s));
        vkd_digest_cols<Fr>(d, w, store);
        w += NB + NC;
        cur = Fr::to_mont(vkd_mask_node(d));
        if (l + 1 < L) {                                                  // the last node is the `val` column of the `set`
            if (store && q == 0) fr_store(w, cur);
            w++;
        }
    }
}

#endif  // __HIPCC__

// the layout `vkd_update_to_subcircuit` builds (vkd.rs:362-617), generalised over split: class, update and path segment of
// subcircuit i, the entries of its subtrace, and the slot of its path's `get initial node` inside its subtrace
struct VkdSub { u32 kind, update, seg, n_slots, path_slot; };
static inline VkdSub vkd_sub(const hk_vkd_desc* d, size_t n_sub, size_t i) {
    const u32 S = d->split;
    if (i < 6) return {VKD_K_PADDING, 0, 0, 1, 0};
    if (i == 6) return {VKD_K_WRITE_PP, 0, 0, 3, 0};
    if (i == n_sub - 1) return {VKD_K_EQUALITY, 0, 0, 2, 0};
    const u32 u = (u32)((i - 7) / (2 * S)), k = (u32)((i - 7) % (2 * S));
    const u32 seg = k >= S ? k - S : k;                    // both paths of an update climb past the same siblings
    if (d->kinds[u] == HK_VKD_APPEND) {
        if (k == 0) return {VKD_K_HGC, u, 0, 1 + S + 3, 1 + S};
        if (k == S - 1) return {VKD_K_CE, u, seg, 5, 0};
    } else if (k == S) {
        return {VKD_K_EHC, u, 0, 6, 3};
    }
    return {VKD_K_C, u, seg, 3, 0};
}

// what both calls check of the descriptor; *n_sub: subcircuits, *n_vals: Fr of the value table
static inline hk_status vkd_check(const hk_vkd_desc* d, size_t* n_sub, size_t* n_vals) {
    if (!d || !d->kinds || !d->leaves || !d->siblings_mont || !d->consts_mont || !d->leaf_hash || !d->node_hash || !d->roots_mont ||
        !d->slot_addr || !d->slot_src)
        return HK_ERR_ARG;
    const size_t S = d->split, U = d->n_updates;
    if (S < 2 || d->depth == 0 || d->depth > 256 || d->depth % (8 * S) || d->depth / S < 8) return HK_ERR_ARG;
    if (U == 0 || U > ((size_t)1 << 20)) return HK_ERR_ARG;
    for (size_t u = 0; u < U; u++)
        if (d->kinds[u] != HK_VKD_APPEND && d->kinds[u] != HK_VKD_UPDATE) return HK_ERR_ARG;
    *n_sub = 8 + 2 * S * U;
    *n_vals = 3 + U * (2 + 3 * S);
    if (*n_sub > ((size_t)1 << 24)) return HK_ERR_ARG;                                         // as hk_exec_tree's n_sub
    if (d->n_slots == 0 || (u64)d->n_slots >= ((u64)1 << 30)) return HK_ERR_LEN;               // 2 n_slots lanes, below 2^31
    for (size_t s = 0; s < d->n_slots; s++)
        if (d->slot_src[s] != HK_VKD_SRC_ZERO && d->slot_src[s] >= *n_vals) return HK_ERR_ARG;
    return poseidon_pair_check(d->leaf_hash, d->node_hash, d->n_consts);
}

template <class C>
hk_status Ops<C>::vkd_trace(hk_ctx* ctx, const hk_vkd_desc* d, void* values_out, void* time_entries_out) {
    size_t n_sub, V;
    HK_TRY(vkd_check(d, &n_sub, &V));
    if (!values_out || !time_entries_out) return HK_ERR_ARG;
    const size_t U = d->n_updates, S = d->split, depth = d->depth, fr = sizeof(Fr), n_fr = 2 * (size_t)d->n_slots;
    Staged in[3] = {staged(d->leaves, U * 2 * VKD_LEAF_BYTES), staged(d->siblings_mont, U * depth * fr),
                    staged(d->consts_mont, d->n_consts * fr)};
    Staged out[2] = {staged(values_out, V * fr), staged(time_entries_out, n_fr * fr)};
    for (const Staged& x : in)
        if (bufs_overlap(values_out, V * fr, x.buf, x.bytes) || bufs_overlap(time_entries_out, n_fr * fr, x.buf, x.bytes))
            return HK_ERR_ARG;
    if (bufs_overlap(values_out, V * fr, time_entries_out, n_fr * fr)) return HK_ERR_ARG;
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    u32 *kinds_d, *addr_d, *src_d, *raw_d;
    unsigned char* zeros_d;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, in, 3);
        kinds_d = c.n<u32>(U);
        addr_d = c.n<u32>(d->n_slots);
        src_d = c.n<u32>(d->n_slots);
        raw_d = c.n<u32>(8 * U);
        zeros_d = (unsigned char*)c.n<u32>(VKD_NAME_BYTES / 4);
        stage_carve(c, out, 2);
    }));
    hipStream_t s = L->stream;
    const void *leaves = in[0].p, *sibs = in[1].p, *consts = in[2].p;
    Fr *vals_d = (Fr*)out[0].p, *out_d = (Fr*)out[1].p;
    HK_TRY(stage_upload(L, in, 3));
    HK_HIP(hipMemcpyAsync(kinds_d, d->kinds, 4 * U, hipMemcpyHostToDevice, s));
    HK_HIP(hipMemcpyAsync(addr_d, d->slot_addr, 4 * (size_t)d->n_slots, hipMemcpyHostToDevice, s));
    HK_HIP(hipMemcpyAsync(src_d, d->slot_src, 4 * (size_t)d->n_slots, hipMemcpyHostToDevice, s));
    HK_HIP(hipMemsetAsync(zeros_d, 0, VKD_NAME_BYTES, s));
    HK_HIP(hipMemcpyAsync(vals_d, d->roots_mont, 2 * fr, hipMemcpyHostToDevice, s));
    const PoseidonDesc a = poseidon_desc(d->leaf_hash), b = poseidon_desc(d->node_hash);
    const u32 nu = (u32)U, seg = (u32)(depth / S);
    HK_LAUNCH((k_vkd_hash<Fr>), dim3((1 + 3 * nu + 63) / 64), dim3(256), 0, s, (const Fr*)consts, a,
              (const unsigned char*)leaves, (const unsigned char*)zeros_d, (const u32*)kinds_d, nu, (u32)S, seg, vals_d, raw_d);
    HK_LAUNCH((k_vkd_chain<Fr>), dim3((2 * nu + 63) / 64), dim3(256), 0, s, (const Fr*)consts, b, (const Fr*)sibs,
              (const u32*)kinds_d, (const u32*)raw_d, nu, (u32)depth, (u32)S, seg, vals_d);
    HK_LAUNCH((k_vkd_trace<Fr>), dim3((u32)((n_fr + 255) / 256)), dim3(256), 0, s, (const Fr*)vals_d, (const u32*)addr_d,
              (const u32*)src_d, (u32)n_fr, out_d);
    HK_TRY(stage_download(L, out, 2));
    return L->settle();
}

template <class C>
hk_status Ops<C>::vkd_witness(hk_ctx* ctx, const hk_vkd_desc* d, const uint32_t* sub_index, size_t batch, size_t n_v,
                              const hk_vkd_cols* cols, void* z_out) {
    size_t n_sub, V;
    HK_TRY(vkd_check(d, &n_sub, &V));
    if (!cols || !d->values_mont || (batch && (!sub_index || !z_out))) return HK_ERR_ARG;
    if (cols->kind >= VKD_K_COUNT) return HK_ERR_ARG;
    if (n_v == 0) return HK_ERR_LEN;
    if (batch >= (1u << 20) || n_v >= ((size_t)1 << 31) || batch * n_v >= ((size_t)1 << 38)) return HK_ERR_LEN;
    const size_t U = d->n_updates, S = d->split, depth = d->depth, Lv = depth / S, fr = sizeof(Fr);
    constexpr size_t NB = vkd_nbits<Fr>(), NC = vkd_ncanon<Fr>();
    // the chains of the class and their column ranges: inside [1, n_v), in the order hash < index < path
    const bool has_hash = cols->kind == VKD_K_HGC || cols->kind == VKD_K_EHC, has_index = cols->kind == VKD_K_HGC;
    const bool has_path = cols->kind >= VKD_K_HGC && cols->kind <= VKD_K_EHC;
    const size_t lt = poseidon_trace_len(d->leaf_hash), nt = poseidon_trace_len(d->node_hash);
    VkdChains ch{};
    u32 n_ch = 0;
    size_t end = 1;
    auto range = [&](u32 which, size_t lo, size_t skip, size_t len) {
        if (lo < end || lo > n_v || skip + len > n_v - lo) return false;                // column 0 is the constant's
        end = lo + skip + len;
        ch.which[n_ch] = which;
        ch.col0[n_ch++] = (u32)(lo + skip);
        return true;
    };
    if (has_hash && !range(VKD_CH_HASH, cols->hash_col0, 8 * VKD_LEAF_BYTES, lt + NB + NC)) return HK_ERR_LEN;
    if (has_index && !range(VKD_CH_INDEX, cols->index_col0, 0, lt + NB + NC)) return HK_ERR_LEN;
    if (has_path && !range(VKD_CH_PATH, cols->path_col0, 0, Lv + Lv * (2 + nt + NB + NC + 1) - 1)) return HK_ERR_LEN;
    // per-row tables; the slots of subcircuit i start at the sum of the subtraces before it
    std::vector<u32> first(n_sub + 1, 0);
    for (size_t i = 0; i < n_sub; i++) first[i + 1] = first[i] + vkd_sub(d, n_sub, i).n_slots;
    if (first[n_sub] != d->n_slots) return HK_ERR_ARG;
    std::vector<VkdRow> rows(batch);                       // outlives the lane's copy
    for (size_t b = 0; b < batch; b++) {
        const size_t i = sub_index[b];
        if (i >= n_sub) return HK_ERR_ARG;
        const VkdSub sc = vkd_sub(d, n_sub, i);
        if (sc.kind != cols->kind) return HK_ERR_ARG;
        VkdRow r{0, 0, 0, 0};
        if (has_path) {
            r.sib_off = (u32)(sc.update * depth + sc.seg * Lv);
            r.init_src = d->slot_src[first[i] + sc.path_slot];
            r.word_src = d->slot_src[first[i] + sc.path_slot + 1];
            if (r.init_src >= V || r.word_src >= V) return HK_ERR_ARG;              // a path never starts from the ZERO constant
            r.leaf_off = (u32)((sc.update * 2 + 1) * VKD_LEAF_BYTES);               // the hashed leaf is leaf_new
        }
        rows[b] = r;
    }
    if (batch == 0) return HK_OK;
    if (!is_device_ptr(z_out)) return HK_ERR_ARG;
    Staged in[4] = {staged(d->leaves, U * 2 * VKD_LEAF_BYTES), staged(d->siblings_mont, U * depth * fr),
                    staged(d->consts_mont, d->n_consts * fr), staged(d->values_mont, V * fr)};
    for (const Staged& x : in)
        if (bufs_overlap(z_out, batch * n_v * fr, x.buf, x.bytes)) return HK_ERR_ARG;
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    VkdRow* rows_d;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, in, 4);
        rows_d = (VkdRow*)c.n<u32>(4 * batch);
    }));
    hipStream_t s = L->stream;
    const void* const p[4] = {in[0].p, in[1].p, in[2].p, in[3].p};
    HK_TRY(stage_upload(L, in, 4));
    HK_HIP(hipMemcpyAsync(rows_d, rows.data(), sizeof(VkdRow) * batch, hipMemcpyHostToDevice, s));
    const PoseidonDesc a = poseidon_desc(d->leaf_hash), bd = poseidon_desc(d->node_hash);
    const u32 nb = (u32)batch;
    HK_LAUNCH((k_vkd_one<Fr>), dim3((nb + 255) / 256), dim3(256), 0, s, nb, n_v, (Fr*)z_out);
    if (has_hash)
        for (size_t b0 = 0; b0 < batch; b0 += VKD_GRID_ROWS) {
            const u32 n = (u32)std::min(batch - b0, (size_t)VKD_GRID_ROWS);
            HK_LAUNCH((k_vkd_leaf_bits<Fr>), dim3((8 * VKD_LEAF_BYTES + 255) / 256, n), dim3(256), 0, s,
                      (const unsigned char*)p[0], (const VkdRow*)rows_d + b0, n_v, (size_t)cols->hash_col0,
                      (Fr*)z_out + b0 * n_v);
        }
    if (n_ch)                                              // padding, write pp, equality: no body columns
        HK_LAUNCH((k_vkd_body<Fr>), dim3((nb + 63) / 64, n_ch), dim3(256), 0, s, (const Fr*)p[2], a, bd,
                  (const unsigned char*)p[0], (const Fr*)p[1], (const Fr*)p[3], (const VkdRow*)rows_d, ch, (u32)Lv, nb,
                  n_v, (Fr*)z_out);
    return L->settle();
}

}  // namespace hk
