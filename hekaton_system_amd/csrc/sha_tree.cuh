// sha_tree.cuh — the head of a big-merkle job on the device (hk_sha_tree / hk_sha_tree_inputs): the
// tree of iterated SHA-256 hashes over the job's leaves, the time-ordered ROM trace of every `set` / `get` and the word-
// program inputs of every class - what distributed-prover/src/tree_hash_circuit.rs:313-470
// `MerkleTreeCircuit::get_portal_subtraces` and hekaton_system_amd/sha_circuit.py `ShaMerkleJob.__init__` / `program_inputs`
// do on the host.
//
//   levels   one lane per node of a level (sha256.cuh: ns applications, a dependent chain of ns (+ 1) compressions per lane;
//            the nodes of a level are independent).  The leaf level has n / 2 + 1 lanes: the padding subcircuit hashes 64
//            zero bytes next to the leaves.  Digests pass through global memory, 32 B per subcircuit in hashlib's byte
//            order.  One launch per level wider than a workgroup, one launch with workgroup barriers for all levels of
//            <= ST_WG_NODES nodes (and the leaf level too when it fits), as exec_tree.cuh's k_et_tree_tail.
//   trace    one lane per (subcircuit, slot): (addr, val) in Montgomery form, hk_exec_tree's ROM layout.
//   inputs   one lane per (member, input word) of the class's word program.
// Subcircuit order: leaves 0 .. n / 2 - 1; the level of width w starts at n - 2 w (parents, the root at n - 2); padding n - 1.
#pragma once
#include "curve_ops_impl.cuh"
#include "ntt.cuh"           // fr_store
#include "sha256.cuh"
#include "job_args.h"

namespace hk {

constexpr u32 ST_WG_NODES = 256;       // nodes of a level the one-workgroup tail takes: a lane each
constexpr u32 ST_LEVEL_LANES = 64;     // lanes per workgroup of a level launch: a wave, so that the chains spread over the CUs

#if defined(__HIPCC__)

// children of node j of a level above the leaves (n / 2 <= j <= n - 2): with d = n - j the level's width is the power of
// two w with w < d <= 2 w, it starts at n - 2 w and the level below at n - 4 w
__device__ __forceinline__ u32 st_left_child(u32 n, u32 j) {
    const u32 d = n - j;
    const u32 w = 1u << (31 - __clz(d - 1));
    return n - 4 * w + 2 * (j - (n - 2 * w));
}

// the digest words (big-endian, FIPS order) of subcircuit j from / to its 32 bytes in hashlib's order
__device__ __forceinline__ void st_load_digest(const uint4* digests, u32 j, u32 (&d)[8]) {
    const uint4 a = digests[2 * (size_t)j], b = digests[2 * (size_t)j + 1];
    d[0] = __builtin_bswap32(a.x); d[1] = __builtin_bswap32(a.y); d[2] = __builtin_bswap32(a.z); d[3] = __builtin_bswap32(a.w);
    d[4] = __builtin_bswap32(b.x); d[5] = __builtin_bswap32(b.y); d[6] = __builtin_bswap32(b.z); d[7] = __builtin_bswap32(b.w);
}
__device__ __forceinline__ void st_store_digest(uint4* digests, u32 j, const u32 (&d)[8]) {
    digests[2 * (size_t)j] = make_uint4(__builtin_bswap32(d[0]), __builtin_bswap32(d[1]), __builtin_bswap32(d[2]), __builtin_bswap32(d[3]));
    digests[2 * (size_t)j + 1] = make_uint4(__builtin_bswap32(d[4]), __builtin_bswap32(d[5]), __builtin_bswap32(d[6]), __builtin_bswap32(d[7]));
}

// Lane t of a level.  w == 0: the leaf level - lane t < n / 2 hashes leaf t into digest t, lane n / 2 hashes 64 zero bytes
// into digest n - 1 (the padding subcircuit).  w > 0: the level of w nodes from n - 2 w - lane t < w hashes the truncated
// digests of its two children.  A lane past the level's end does the last lane's work and stores nothing.
__device__ __forceinline__ void st_level_lane(const uint4* leaves, uint4* digests, u32 n, u32 ns, u32 w, u32 t) {
    const u32 nl = n >> 1;
    const u32 count = w ? w : nl + 1;
    const u32 k = t < count ? t : count - 1;
    u32 b[16], dg[8], j;
    if (w == 0) {                                                  // uniform: w is the same in every lane
        const bool pad = k == nl;
        const uint4* src = leaves + 4 * (size_t)(pad ? 0 : k);
        HK_UNROLL for (int q = 0; q < 4; q++) {
            const uint4 x = src[q];
            b[4 * q + 0] = pad ? 0u : __builtin_bswap32(x.x);
            b[4 * q + 1] = pad ? 0u : __builtin_bswap32(x.y);
            b[4 * q + 2] = pad ? 0u : __builtin_bswap32(x.z);
            b[4 * q + 3] = pad ? 0u : __builtin_bswap32(x.w);
        }
        j = pad ? n - 1 : k;
    } else {
        j = n - 2 * w + k;
        const u32 c = n - 4 * w + 2 * k;
        u32 l[8], r[8];
        st_load_digest(digests, c, l);
        st_load_digest(digests, c + 1, r);
        sha_block_children(b, l, r);
    }
    iterated_sha256(dg, b, w == 0, ns);
    if (t < count) st_store_digest(digests, j, dg);
}

template <int UNUSED>
__global__ void __launch_bounds__(ST_LEVEL_LANES)
k_sha_tree_level(const uint4* __restrict__ leaves, uint4* digests, u32 n, u32 ns, u32 w) {
    st_level_lane(leaves, digests, n, ns, w, blockIdx.x * ST_LEVEL_LANES + threadIdx.x);
}

// Every remaining level in ONE workgroup, a barrier between levels: with_leaves runs the leaf level (n / 2 + 1 <=
// ST_WG_NODES lanes) first; then the levels of width w, w / 2, .. 1 (w <= ST_WG_NODES).  The loop bounds are uniform over the
// workgroup and every lane stays through every barrier; only the stores are guarded.
template <int UNUSED>
__global__ void __launch_bounds__(ST_WG_NODES)
k_sha_tree_tail(const uint4* __restrict__ leaves, uint4* digests, u32 n, u32 ns, u32 with_leaves, u32 w) {
    if (with_leaves) {
        st_level_lane(leaves, digests, n, ns, 0, threadIdx.x);
        __syncthreads();
    }
    HK_NOUNROLL for (; w >= 1; w >>= 1) {
        st_level_lane(leaves, digests, n, ns, w, threadIdx.x);
        __syncthreads();
    }
}

// entry g = (subcircuit g / np, slot g % np) of the flattened time-ordered trace: (addr, val) of the node it names, or the
// placeholder (0, 0).  Lane 0 also writes sha_root = val(n - 2).  Every lane forms the values of a node it may read and
// selects; only the address differs between a named node and none.
template <class Fr>
__global__ void __launch_bounds__(256)
k_sha_tree_trace(const uint4* __restrict__ digests, u32 n, u32 np, u32 total, Fr* __restrict__ time_e, Fr* __restrict__ sha_root) {
    const u32 g = blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const u32 idx = g / np, slot = g % np, nl = n >> 1;
    const bool has_kids = idx >= nl && idx <= n - 2;               // a parent or the root: two gets first
    const bool has_set = idx < n - 2;                              // a leaf or a parent: the set last
    const bool get = has_kids && slot < 2;
    const bool set = has_set && slot == np - 1;
    const u32 node = get ? st_left_child(n, has_kids ? idx : nl) + slot : idx;
    const bool named = get || set;
    u32 d[8];
    st_load_digest(digests, node, d);
    Fr a = Fr::zero();
    a.v[0] = 1 + node;
    a = Fr::to_mont(a);
    Fr v = sha_digest_field<Fr>(d);
    HK_UNROLL for (int i = 0; i < Fr::N; i++) {
        a.v[i] = named ? a.v[i] : 0u;
        v.v[i] = named ? v.v[i] : 0u;
    }
    fr_store(&time_e[2 * (size_t)g], a);
    fr_store(&time_e[2 * (size_t)g + 1], v);
    if (g == 0) {
        u32 r[8];
        st_load_digest(digests, n - 2, r);
        fr_store(sha_root, sha_digest_field<Fr>(r));
    }
}

// inputs[b][k], one lane each.  n_inputs 16: word k of leaf sub[b], big-endian (zero for the padding subcircuit n - 1);
// n_inputs 54: byte k % 27 of the digest of child k / 27 of node sub[b].  Bytes are read one by one: neither input needs
// an alignment.
template <int UNUSED>
__global__ void __launch_bounds__(256)
k_sha_tree_inputs(const unsigned char* __restrict__ leaves, const unsigned char* __restrict__ digests, u32 n, u32 n_inputs,
                  const u32* __restrict__ sub, u32 total, u32* __restrict__ out) {
    const u32 g = blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const u32 b = g / n_inputs, k = g % n_inputs, i = sub[b];
    u32 v;
    if (n_inputs == 16) {                                          // uniform
        const bool pad = i == n - 1;
        const unsigned char* p = leaves + 64 * (size_t)(pad ? 0 : i) + 4 * k;
        v = ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | (u32)p[3];
        v = pad ? 0u : v;
    } else {
        const u32 side = k / SHA_INNER_HASH_SIZE;
        v = digests[32 * (size_t)(st_left_child(n, i) + side) + (k - side * SHA_INNER_HASH_SIZE)];
    }
    out[g] = v;
}

#endif  // __HIPCC__

// n_sub a power of two in [4, 2^20]
static inline bool st_n_sub_ok(uint32_t n) { return n >= 4 && n <= (1u << 20) && (n & (n - 1)) == 0; }

template <class C>
hk_status Ops<C>::sha_tree(hk_ctx* ctx, const void* leaves, uint32_t n_sub, uint32_t ns, uint32_t n_portals,
                           const hk_sha_tree_out* o) {
    if (!leaves || !o || (!o->digests_out && !o->time_entries_mont_out && !o->sha_root_mont_out)) return HK_ERR_ARG;
    if (!st_n_sub_ok(n_sub) || ns == 0 || ns >= (1u << 16) || n_portals < 3) return HK_ERR_ARG;
    if ((u64)n_sub * n_portals >= ((u64)1 << 28)) return HK_ERR_ARG;                 // lanes of k_sha_tree_trace
    const size_t n = n_sub, nl = n / 2, np = n_portals;
    const size_t leaf_bytes = nl * 64, dig_bytes = n * 32, time_bytes = n * np * 2 * sizeof(Fr);
    if (bufs_overlap(o->digests_out, dig_bytes, leaves, leaf_bytes) ||
        bufs_overlap(o->time_entries_mont_out, time_bytes, leaves, leaf_bytes) ||
        bufs_overlap(o->sha_root_mont_out, sizeof(Fr), leaves, leaf_bytes))
        return HK_ERR_ARG;
    // the level lanes read a leaf as four 16-B words: device-resident leaves are read in place when they are aligned so
    const bool in_place = is_device_ptr(leaves) && ((uintptr_t)leaves & 15) == 0;
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    void* lv;
    uint4* dig;
    Fr *time_e, *root;
    HK_TRY(L->carve([&](Carve& c) {
        lv = c.take(in_place ? 0 : leaf_bytes);
        dig = c.n<uint4>(2 * n);
        time_e = c.n<Fr>(2 * n * np);
        root = c.n<Fr>(1);
    }));
    hipStream_t s = L->stream;
    if (in_place) lv = (void*)leaves;
    else HK_HIP(hipMemcpyAsync(lv, leaves, leaf_bytes, h2d_kind(leaves), s));
    const uint4* lp = (const uint4*)lv;
    const u32 nn = (u32)n;
    const bool fused_leaves = nl + 1 <= ST_WG_NODES;
    if (!fused_leaves)
        HK_LAUNCH((k_sha_tree_level<0>), dim3((u32)((nl + 1 + ST_LEVEL_LANES - 1) / ST_LEVEL_LANES)), dim3(ST_LEVEL_LANES), 0, s,
                  lp, dig, nn, ns, 0u);
    u32 w = (u32)(nl / 2);
    for (; w > ST_WG_NODES; w >>= 1)
        HK_LAUNCH((k_sha_tree_level<0>), dim3(w / ST_LEVEL_LANES), dim3(ST_LEVEL_LANES), 0, s, lp, dig, nn, ns, w);
    HK_LAUNCH((k_sha_tree_tail<0>), dim3(1), dim3(ST_WG_NODES), 0, s, lp, dig, nn, ns, fused_leaves ? 1u : 0u, w);
    const u32 total = (u32)(n * np);                               // < 2^28
    HK_LAUNCH((k_sha_tree_trace<Fr>), dim3((total + 255) / 256), dim3(256), 0, s, (const uint4*)dig, nn, (u32)np, total, time_e,
              root);
    struct { void* dst; const void* src; size_t bytes; } outs[] = {
        {o->digests_out, dig, dig_bytes}, {o->time_entries_mont_out, time_e, time_bytes}, {o->sha_root_mont_out, root, sizeof(Fr)}};
    for (auto& x : outs)
        if (x.dst)
            HK_HIP(hipMemcpyAsync(x.dst, x.src, x.bytes, is_device_ptr(x.dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    return L->settle();
}

template <class C>
hk_status Ops<C>::sha_tree_inputs(hk_ctx* ctx, const void* leaves, const void* digests, uint32_t n_sub, uint32_t n_inputs,
                                  const uint32_t* sub_index, size_t batch, uint32_t* inputs_out) {
    if (!st_n_sub_ok(n_sub) || (n_inputs != 16 && n_inputs != 2 * SHA_INNER_HASH_SIZE)) return HK_ERR_ARG;
    if (batch == 0) return HK_OK;
    if (!sub_index || !inputs_out || batch >= (1u << 20)) return HK_ERR_ARG;        // batch x 54 < 2^26: lanes of k_sha_tree_inputs
    const bool of_leaves = n_inputs == 16;
    if (of_leaves ? !leaves : !digests) return HK_ERR_ARG;
    const size_t n = n_sub, nl = n / 2;
    for (size_t b = 0; b < batch; b++) {
        const u32 i = sub_index[b];
        if (of_leaves ? !(i < nl || i == n - 1) : !(i >= nl && i <= n - 2)) return HK_ERR_ARG;
    }
    const void* src = of_leaves ? leaves : digests;                // the one input this kind reads
    const size_t src_bytes = of_leaves ? nl * 64 : n * 32, out_bytes = batch * n_inputs * 4;
    if (bufs_overlap(inputs_out, out_bytes, leaves, nl * 64) || bufs_overlap(inputs_out, out_bytes, digests, n * 32)) return HK_ERR_ARG;
    Staged in = staged(src, src_bytes);
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    u32 *sub_d, *out_d;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, &in, 1);
        sub_d = c.n<u32>(batch);
        out_d = c.n<u32>(batch * n_inputs);
    }));
    hipStream_t s = L->stream;
    HK_TRY(stage_upload(L, &in, 1));
    HK_HIP(hipMemcpyAsync(sub_d, sub_index, 4 * batch, hipMemcpyHostToDevice, s));
    const u32 total = (u32)(batch * n_inputs);
    const unsigned char* p = (const unsigned char*)in.p;
    HK_LAUNCH((k_sha_tree_inputs<0>), dim3((total + 255) / 256), dim3(256), 0, s, of_leaves ? p : nullptr, of_leaves ? nullptr : p,
              (u32)n, n_inputs, (const u32*)sub_d, total, out_d);
    HK_HIP(hipMemcpyAsync(inputs_out, out_d, out_bytes, is_device_ptr(inputs_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    return L->settle();
}

}  // namespace hk
