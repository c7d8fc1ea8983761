// exec_tree.cuh — the coordinator's work between the two rounds of a job on the device (hk_exec_tree):
// the running evaluations after every subcircuit, the execution leaves, their Poseidon Merkle tree and one authentication
// path per subcircuit (distributed-prover/src/coordinator.rs:125-174 `generate_exec_tree`, 425-466 the `generate_proof` loop
// of CoordinatorStage1State::new; eval_tree.rs:53-101).
//
//   (a) evaluations   a product scan: one lane per chunk of ET_CHUNK consecutive entries of the flattened trace (factors and
//                     their product, subtrace boundaries ignored), a tiled exclusive scan of the chunk products (the shape of
//                     scan.cuh's k_scan_u32_*, with Fr::mul), one lane per subcircuit boundary: prefix of its chunk times
//                     the < ET_CHUNK factors left of the boundary.  Time and address order share every launch (grid.y).
//   (b) tree          Poseidon with the state spread over the four lanes of a quad (poseidon_permute_quad): one launch hashes
//                     the leaves, one launch per level wider than a workgroup, one launch with workgroup barriers for all
//                     levels of <= ET_WG_STATES states (and the leaf level too when it fits).
//   (c) paths         siblings[i][l] = level_l[(i >> l) ^ 1], one lane per (i, l).
#pragma once
#include "curve_ops_impl.cuh"
#include "poseidon.cuh"

namespace hk {

constexpr u32 ET_CHUNK = 8;            // entries per lane of the factor pass
constexpr u32 ET_SCAN_TILE = 256;      // chunk products per scan tile (one per lane of a workgroup)
constexpr u32 ET_TOPS_LANES = 64;      // lanes of the scan over the tile totals: each takes ceil(tiles / 64) consecutive tiles
constexpr u32 ET_WG_STATES = 64;       // Poseidon states of one 256-lane workgroup (a quad each)

#if defined(__HIPCC__)

// the challenges in the reference's challenges() order: c[0 .. K - 2] the entry challenges, c[K - 1] = tr_chal
template <class Fr> struct EtChal { Fr c[4]; };

// f[1] + c0 f[0] [+ c1 f[2] + c2 f[3]]: the representation of one entry, and its factor tr_chal - repr
// (rom_transcript.rs:84-86, ram_transcript.rs:109-112)
template <class Fr, int K>
__device__ __forceinline__ Fr et_repr(const Fr* __restrict__ e, const EtChal<Fr>& ch) {
    Fr r = Fr::add(fr_load(&e[1]), Fr::mul(ch.c[0], fr_load(&e[0])));
    if constexpr (K == 4) {
        r = Fr::add(r, Fr::mul(ch.c[1], fr_load(&e[2])));
        r = Fr::add(r, Fr::mul(ch.c[2], fr_load(&e[3])));
    }
    return r;
}
template <class Fr, int K>
__device__ __forceinline__ Fr et_factor(const Fr* __restrict__ e, const EtChal<Fr>& ch) {
    return Fr::sub(ch.c[K - 1], et_repr<Fr, K>(e, ch));
}

// (a1) prods[y][c] = product of the factors of entries [c ET_CHUNK, (c + 1) ET_CHUNK) of order y (0 time, 1 address); an
// entry past n counts as 1.  n_chunks = n / ET_CHUNK + 1: every boundary b <= n has its chunk b / ET_CHUNK.
template <class Fr, int K>
__global__ void __launch_bounds__(64)
k_et_chunk_prod(const Fr* __restrict__ time_e, const Fr* __restrict__ addr_e, u64 n, u32 n_chunks, EtChal<Fr> ch,
                Fr* __restrict__ prods) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const Fr* e = blockIdx.y ? addr_e : time_e;
    Fr acc = Fr::one();
    HK_NOUNROLL for (u32 j = 0; j < ET_CHUNK; j++) {
        u64 k = (u64)c * ET_CHUNK + j;
        if (k < n) acc = Fr::mul(acc, et_factor<Fr, K>(e + k * K, ch));
    }
    fr_store(&prods[(size_t)blockIdx.y * n_chunks + c], acc);
}

// inclusive product scan of one value per lane over a workgroup of W lanes (W a power of two <= 256); s: W Fr of LDS.
// Every lane multiplies in every step (by one below the offset), so no lane leaves the barriers.
template <class Fr, u32 W>
__device__ __forceinline__ Fr et_wg_scan(Fr* s, u32 tid, Fr v) {
    s[tid] = v;
    __syncthreads();
    HK_NOUNROLL for (u32 off = 1; off < W; off <<= 1) {
        Fr x = s[tid >= off ? tid - off : tid];
        x = fr_select(tid >= off, x, Fr::one());
        __syncthreads();
        v = Fr::mul(v, x);
        s[tid] = v;
        __syncthreads();
    }
    return v;
}

// (a2) per tile of ET_SCAN_TILE chunk products: the exclusive prefix within the tile (in place), the tile's total into tops
template <class Fr>
__global__ void __launch_bounds__(ET_SCAN_TILE)
k_et_scan_tile(Fr* __restrict__ prods, Fr* __restrict__ tops, u32 n_chunks, u32 n_tiles) {
    __shared__ Fr s[ET_SCAN_TILE];
    const u32 tid = threadIdx.x;
    const u32 c = blockIdx.x * ET_SCAN_TILE + tid;
    Fr* p = prods + (size_t)blockIdx.y * n_chunks;
    Fr v = Fr::one();
    if (c < n_chunks) v = fr_load(&p[c]);
    Fr inc = et_wg_scan<Fr, ET_SCAN_TILE>(s, tid, v);
    Fr exc = fr_select(tid != 0, s[tid ? tid - 1 : 0], Fr::one());
    if (c < n_chunks) fr_store(&p[c], exc);
    if (tid == ET_SCAN_TILE - 1) fr_store(&tops[(size_t)blockIdx.y * n_tiles + blockIdx.x], inc);
}

// (a3) exclusive scan of the tile totals (in place), one workgroup per order: lane t takes the `per` consecutive tiles
// [t per, (t + 1) per) - their product, a scan over the lanes, then the running prefix back over its tiles.
template <class Fr>
__global__ void __launch_bounds__(ET_TOPS_LANES) k_et_scan_tops(Fr* __restrict__ tops, u32 n_tiles) {
    __shared__ Fr s[ET_TOPS_LANES];
    const u32 tid = threadIdx.x;
    const u32 per = (n_tiles + ET_TOPS_LANES - 1) / ET_TOPS_LANES;
    Fr* p = tops + (size_t)blockIdx.y * n_tiles;
    Fr acc = Fr::one();
    HK_NOUNROLL for (u32 j = 0; j < per; j++) {
        u32 i = tid * per + j;
        if (i < n_tiles) acc = Fr::mul(acc, fr_load(&p[i]));
    }
    et_wg_scan<Fr, ET_TOPS_LANES>(s, tid, acc);
    Fr run = fr_select(tid != 0, s[tid ? tid - 1 : 0], Fr::one());
    HK_NOUNROLL for (u32 j = 0; j < per; j++) {
        u32 i = tid * per + j;
        if (i < n_tiles) {
            Fr t = fr_load(&p[i]);
            fr_store(&p[i], run);
            run = Fr::mul(run, t);
        }
    }
}

// (a4) one lane per (subcircuit i, order y): evaluation after subcircuit i = product of the factors of entries
// [0, offsets[i + 1]) = tile prefix x chunk prefix x the factors between the chunk's start and the boundary.  Writes
// evals[i][y] and leaf field y; the address-order lane also writes the leaf's last entry: entry offsets[i + 1] - 1 of the
// address order, zero when there is none yet (`last_subtrace_entry`; an empty subtrace carries the previous one over).
template <class Fr, int K>
__global__ void __launch_bounds__(64)
k_et_leaves(const Fr* __restrict__ time_e, const Fr* __restrict__ addr_e, const u32* __restrict__ offsets, u32 n_sub,
            u32 n_chunks, u32 n_tiles, EtChal<Fr> ch, const Fr* __restrict__ prods, const Fr* __restrict__ tops,
            Fr* __restrict__ evals, Fr* __restrict__ leaves) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 y = blockIdx.y;
    if (i >= n_sub) return;
    const Fr* e = y ? addr_e : time_e;
    const u32 b = offsets[i + 1];
    const u32 c = b / ET_CHUNK, rem = b % ET_CHUNK;
    Fr v = Fr::mul(fr_load(&tops[(size_t)y * n_tiles + c / ET_SCAN_TILE]), fr_load(&prods[(size_t)y * n_chunks + c]));
    HK_NOUNROLL for (u32 j = 0; j < ET_CHUNK - 1; j++)
        if (j < rem) v = Fr::mul(v, et_factor<Fr, K>(e + ((u64)c * ET_CHUNK + j) * K, ch));
    fr_store(&evals[(size_t)i * 2 + y], v);
    Fr* leaf = leaves + (size_t)i * (2 + K);
    fr_store(&leaf[y], v);
    if (y) {
        HK_UNROLL for (int f = 0; f < K; f++) {
            Fr x = Fr::zero();
            if (b) x = fr_load(&addr_e[(u64)(b - 1) * K + f]);
            fr_store(&leaf[2 + f], x);
        }
    }
}

// ---- the tree: Poseidon on a quad of lanes (poseidon.cuh) ------------------------------------------------------------------
// two-to-one hash of in[0], in[1] on a quad, valid on lane 1: lane 2 loads the right input, every other lane the left one
template <class Fr>
__device__ __forceinline__ Fr et_node_digest(const Fr* __restrict__ consts, const PoseidonDesc& d, const Fr* __restrict__ in) {
    const Fr v = fr_load(&in[(threadIdx.x & 3u) == 2 ? 1 : 0]);
    return poseidon_permute_quad<Fr, 3, 17>(consts, d, poseidon_pair_input(v, v));
}

// (b1) nodes[i] = digest of leaf i (lane 1 of its sponge), one quad per leaf.  A quad past the end hashes the last leaf and
// stores nothing.
template <class Fr>
__global__ void __launch_bounds__(256)
k_et_leaf_hash(const Fr* __restrict__ consts, PoseidonDesc leaf_d, const Fr* __restrict__ leaves, u32 nf, u32 n_sub,
               Fr* __restrict__ nodes) {
    const u32 t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const u32 i = t < n_sub ? t : n_sub - 1;
    Fr h = poseidon_leaf_sponge<Fr>(consts, leaf_d, leaves + (size_t)i * nf, nf);
    if (t < n_sub && (threadIdx.x & 3u) == 1) fr_store(&nodes[t], h);
}

// (b2) one level: out[j] = H(in[2 j], in[2 j + 1]) for j < w_out, one quad per output node
template <class Fr>
__global__ void __launch_bounds__(256)
k_et_level(const Fr* __restrict__ consts, PoseidonDesc node_d, const Fr* __restrict__ in, u32 w_out, Fr* __restrict__ out) {
    const u32 t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const u32 j = t < w_out ? t : w_out - 1;
    Fr h = et_node_digest<Fr>(consts, node_d, in + 2 * (size_t)j);
    if (t < w_out && (threadIdx.x & 3u) == 1) fr_store(&out[t], h);
}

// (b3) every remaining level in ONE workgroup, a barrier between levels (as k_msm_accum_tail does): with_leaves hashes the
// n_sub <= ET_WG_STATES leaves first; then from the level of width w at nodes[off] (w / 2 <= ET_WG_STATES outputs) up to
// the root.  The loop bounds are uniform over the workgroup; only the stores are guarded.
template <class Fr>
__global__ void __launch_bounds__(256)
k_et_tree_tail(const Fr* __restrict__ consts, PoseidonDesc leaf_d, PoseidonDesc node_d, const Fr* __restrict__ leaves, u32 nf,
               u32 with_leaves, u32 w, u32 off, Fr* nodes) {
    const u32 t = threadIdx.x >> 2;
    const bool writer = (threadIdx.x & 3u) == 1;
    if (with_leaves) {
        const u32 i = t < w ? t : w - 1;
        Fr h = poseidon_leaf_sponge<Fr>(consts, leaf_d, leaves + (size_t)i * nf, nf);
        if (t < w && writer) fr_store(&nodes[off + t], h);
        __syncthreads();
    }
    HK_NOUNROLL while (w > 1) {
        const u32 w_out = w >> 1;
        const u32 j = t < w_out ? t : w_out - 1;
        Fr h = et_node_digest<Fr>(consts, node_d, nodes + off + 2 * (size_t)j);
        if (t < w_out && writer) fr_store(&nodes[off + w + t], h);
        __syncthreads();
        off += w;
        w = w_out;
    }
}

// (c) siblings[i][l] = level_l[(i >> l) ^ 1]; level l (n_sub >> l nodes) starts at nodes[2 n_sub - (2 n_sub >> l)]
template <class Fr>
__global__ void __launch_bounds__(256)
k_et_paths(const Fr* __restrict__ nodes, u32 n_sub, u32 depth, Fr* __restrict__ siblings) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (u64)n_sub * depth) return;
    const u32 i = (u32)(k / depth), l = (u32)(k % depth);
    const u64 base = 2 * (u64)n_sub - ((2 * (u64)n_sub) >> l);
    fr_store(&siblings[k], fr_load(&nodes[base + ((i >> l) ^ 1u)]));
}

#endif  // __HIPCC__

template <class C>
hk_status Ops<C>::exec_tree(hk_ctx* ctx, const hk_exec_tree_desc* d, const hk_exec_tree_out* o) {
    const size_t n_sub = d->n_sub, K = d->entry_fields;
    u32 depth = 0;
    while (((size_t)1 << depth) < n_sub) depth++;
    HK_TRY(tree_shape_check(n_sub, depth));                 // n_sub itself: depth is derived from it
    if (K != 2 && K != 4) return HK_ERR_ARG;
    if (!d->offsets || !d->challenges_mont || !d->consts_mont || !d->leaf_hash || !d->node_hash || !o->leaves_mont ||
        !o->siblings_mont || !o->root_mont)
        return HK_ERR_ARG;
    HK_TRY(offsets_check(d->offsets, n_sub));
    const size_t n = d->offsets[n_sub], nf = 2 + K;
    if (n && (!d->time_entries_mont || !d->addr_entries_mont)) return HK_ERR_ARG;
    HK_TRY(poseidon_pair_check(d->leaf_hash, d->node_hash, d->n_consts));

    const u32 n_chunks = (u32)(n / ET_CHUNK + 1), n_tiles = (n_chunks + ET_SCAN_TILE - 1) / ET_SCAN_TILE;
    EtChal<Fr> ch;
    for (size_t k = 0; k < 4; k++) {
        ch.c[k] = Fr::zero();
        if (k < K) memcpy(&ch.c[k], (const char*)d->challenges_mont + k * sizeof(Fr), sizeof(Fr));
    }
    Staged in[3] = {staged(d->time_entries_mont, n * K * sizeof(Fr)), staged(d->addr_entries_mont, n * K * sizeof(Fr)),
                    staged(d->consts_mont, d->n_consts * sizeof(Fr))};
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    u32* off_d;
    Fr *prods, *tops, *evals, *leaves, *nodes, *sibs;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, in, 3);
        off_d = c.n<u32>(n_sub + 1);
        prods = c.n<Fr>(2 * (size_t)n_chunks);
        tops = c.n<Fr>(2 * (size_t)n_tiles);
        evals = c.n<Fr>(2 * n_sub);
        leaves = c.n<Fr>(nf * n_sub);
        nodes = c.n<Fr>(2 * n_sub - 1);
        sibs = c.n<Fr>(n_sub * depth);
    }));
    hipStream_t s = L->stream;
    HK_TRY(stage_upload(L, in, 3));
    HK_HIP(hipMemcpyAsync(off_d, d->offsets, 4 * (n_sub + 1), hipMemcpyHostToDevice, s));
    const Fr *tp = (const Fr*)in[0].p, *ap = (const Fr*)in[1].p, *cp = (const Fr*)in[2].p;
    const u32 ns = (u32)n_sub;

    // (a) running evaluations and leaves
    if (K == 2)
        HK_LAUNCH((k_et_chunk_prod<Fr, 2>), dim3((n_chunks + 63) / 64, 2), dim3(64), 0, s, tp, ap, (u64)n, n_chunks, ch, prods);
    else
        HK_LAUNCH((k_et_chunk_prod<Fr, 4>), dim3((n_chunks + 63) / 64, 2), dim3(64), 0, s, tp, ap, (u64)n, n_chunks, ch, prods);
    HK_LAUNCH((k_et_scan_tile<Fr>), dim3(n_tiles, 2), dim3(ET_SCAN_TILE), 0, s, prods, tops, n_chunks, n_tiles);
    HK_LAUNCH((k_et_scan_tops<Fr>), dim3(1, 2), dim3(ET_TOPS_LANES), 0, s, tops, n_tiles);
    if (K == 2)
        HK_LAUNCH((k_et_leaves<Fr, 2>), dim3((ns + 63) / 64, 2), dim3(64), 0, s, tp, ap, (const u32*)off_d, ns, n_chunks,
                  n_tiles, ch, (const Fr*)prods, (const Fr*)tops, evals, leaves);
    else
        HK_LAUNCH((k_et_leaves<Fr, 4>), dim3((ns + 63) / 64, 2), dim3(64), 0, s, tp, ap, (const u32*)off_d, ns, n_chunks,
                  n_tiles, ch, (const Fr*)prods, (const Fr*)tops, evals, leaves);

    // (b) the tree: nodes = leaf digests, then each level, root last
    const PoseidonDesc a = poseidon_desc(d->leaf_hash), b = poseidon_desc(d->node_hash);
    const bool fused_leaves = ns <= ET_WG_STATES;
    if (!fused_leaves)
        HK_LAUNCH((k_et_leaf_hash<Fr>), dim3((ns + ET_WG_STATES - 1) / ET_WG_STATES), dim3(256), 0, s, cp, a,
                  (const Fr*)leaves, (u32)nf, ns, nodes);
    u32 w = ns, off = 0;
    while ((w >> 1) > ET_WG_STATES) {
        const u32 w_out = w >> 1;
        HK_LAUNCH((k_et_level<Fr>), dim3((w_out + ET_WG_STATES - 1) / ET_WG_STATES), dim3(256), 0, s, cp, b,
                  (const Fr*)(nodes + off), w_out, nodes + off + w);
        off += w;
        w = w_out;
    }
    HK_LAUNCH((k_et_tree_tail<Fr>), dim3(1), dim3(256), 0, s, cp, a, b, (const Fr*)leaves, (u32)nf, fused_leaves ? 1u : 0u,
              w, off, nodes);
    // (c) the paths
    HK_LAUNCH((k_et_paths<Fr>), dim3((u32)((n_sub * depth + 255) / 256)), dim3(256), 0, s, (const Fr*)nodes, ns, depth, sibs);

    struct { void* dst; const Fr* src; size_t count; } outs[] = {
        {o->evals_mont, evals, 2 * n_sub},       {o->leaves_mont, leaves, nf * n_sub}, {o->nodes_mont, nodes, 2 * n_sub - 1},
        {o->siblings_mont, sibs, n_sub * depth}, {o->root_mont, nodes + 2 * n_sub - 2, 1}};
    for (auto& x : outs)
        if (x.dst)
            HK_HIP(hipMemcpyAsync(x.dst, x.src, x.count * sizeof(Fr),
                                  is_device_ptr(x.dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    return L->settle();
}

}  // namespace hk
