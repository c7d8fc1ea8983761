// trace_sort.cuh — the coordinator's address-ordered trace on the device (hk_trace_sort): the stable
// sort of the flattened time-ordered entries by addr (ROM) / (addr, timestamp) (RAM) that
// distributed-prover/src/coordinator.rs:92-123 `sort_subtraces_by_addr` does with sort_by_key, and the stage-0 witness rows
// (hk_stage0_witness) cut from the two traces where they lie.
//
//   keys     one lane per entry: the key fields out of Montgomery form, packed as W = 2 (ROM) or 3 (RAM) u32 planes, least
//            significant first (RAM: timestamp, addr low, addr high), next to the entry's index; a word of flags: an error bit
//            (addr >= 2^64 or timestamp >= 2^32) and the OR and the AND of every key, whose difference is the varying bits.
//   passes   LSD radix sort of (key, index), 8-bit digits, a pass per digit that varies.  A tile of TS_TILE entries is cut into
//            four consecutive quarters, one per wave; a wave walks its quarter 64 entries at a time and ranks each entry among
//            the equal digits in front of it: peers of the same step from __ballot masks, earlier steps from a count per
//            (wave, digit) in LDS that only that wave's one leader lane per digit advances.  No position depends on the order
//            in which anything lands: the counts of the histogram kernel go through LDS atomics, and a count is a count.
//   gather   the 64-B or 128-B entries by the final index vector, which is also perm_out.
// A trace of at most TS_TILE entries runs keys, every pass and the gather in one launch of one workgroup (k_ts_small).
#pragma once
#include "curve_ops_impl.cuh"
#include "ntt.cuh"           // fr_load
#include "scan.cuh"
#include "job_args.h"

namespace hk {

constexpr u32 TS_TILE = 2048;          // entries per workgroup of a pass: a power of two, four quarters of TS_ROUNDS x 64
constexpr u32 TS_ROUNDS = TS_TILE / 256;
constexpr u32 TS_FLAG_WORDS = 8;       // [0] error, [1 .. 3] OR of the key words, [4 .. 6] AND of the key words

#if defined(__HIPCC__)

// the key words of one entry (canonical integers of field 0 and, for RAM, field 2); false when one does not fit
template <class Fr, int K>
__device__ __forceinline__ bool ts_key_words(const Fr* __restrict__ e, u32* kw) {
    constexpr int W = K == 2 ? 2 : 3;
    const Fr a = Fr::from_mont(fr_load(&e[0]));
    u32 hi = 0;
    HK_UNROLL for (int i = 2; i < Fr::N; i++) hi |= a.v[i];
    kw[W - 2] = a.v[0];
    kw[W - 1] = a.v[1];
    if constexpr (K == 4) {
        const Fr t = Fr::from_mont(fr_load(&e[2]));
        HK_UNROLL for (int i = 1; i < Fr::N; i++) hi |= t.v[i];
        kw[0] = t.v[0];
    }
    return hi == 0;
}

// what a workgroup saw, into the call's flag words: s[0] error, s[1 + w] OR, s[4 + w] AND (LDS, atomics: order-free)
template <int W>
__device__ __forceinline__ void ts_note_key(u32* s, bool ok, const u32* kw) {
    if (!ok) atomicOr(&s[0], 1u);
    HK_UNROLL for (int w = 0; w < W; w++) {
        atomicOr(&s[1 + w], kw[w]);
        atomicAnd(&s[4 + w], kw[w]);
    }
}

// keys[w n + i] = key word w of entry i, idx[i] = i; flags as above (set up by the host: 0, 0 0 0, ~0 ~0 ~0)
template <class Fr, int K>
__global__ void __launch_bounds__(256)
k_ts_keys(const Fr* __restrict__ entries, u32 n, u32* __restrict__ keys, u32* __restrict__ idx, u32* __restrict__ flags) {
    constexpr int W = K == 2 ? 2 : 3;
    __shared__ u32 s[TS_FLAG_WORDS];
    const u32 tid = threadIdx.x;
    if (tid < TS_FLAG_WORDS) s[tid] = tid >= 4 ? ~0u : 0u;
    __syncthreads();
    const u32 i = blockIdx.x * 256 + tid;
    if (i < n) {
        u32 kw[W];
        const bool ok = ts_key_words<Fr, K>(entries + (size_t)i * K, kw);
        HK_UNROLL for (int w = 0; w < W; w++) keys[(size_t)w * n + i] = kw[w];
        idx[i] = i;
        ts_note_key<W>(s, ok, kw);
    }
    __syncthreads();
    if (tid == 0 && s[0]) atomicOr(&flags[0], 1u);
    if (tid >= 1 && tid < 1 + W) atomicOr(&flags[tid], s[tid]);
    if (tid >= 4 && tid < 4 + W) atomicAnd(&flags[tid], s[tid]);
}

// hist[d n_tiles + tile] = entries of the tile whose digit is d (digit-major, tile-minor: the order of the scan)
template <int UNUSED>
__global__ void __launch_bounds__(256)
k_ts_hist(const u32* __restrict__ kw, u32 n, u32 shift, u32 n_tiles, u32* __restrict__ hist) {
    __shared__ u32 s[256];
    const u32 tid = threadIdx.x;
    s[tid] = 0;
    __syncthreads();
    const u32 base = blockIdx.x * TS_TILE;
    HK_UNROLL for (u32 r = 0; r < TS_ROUNDS; r++) {
        const u32 i = base + r * 256 + tid;
        if (i < n) atomicAdd(&s[(kw[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)tid * n_tiles + blockIdx.x] = s[tid];
}

// One pass over one tile: entries [base, base + count) of (kin, iin) go to (kout, iout) at start(d) + their rank among the
// tile's entries of digit d, in index order.  start(d) = gbase[d n_tiles + tile], or with gbase == NULL (a one-tile sort) the
// exclusive scan of the tile's own digit counts.  Wave w owns entries [w TS_TILE / 4, (w + 1) TS_TILE / 4) of the tile.
// cnt: 4 x 256 u32 of LDS, woff: 4 x 256, sc: 256.  Every lane of the workgroup calls it; bounds are uniform.
template <int W>
__device__ __forceinline__ void ts_tile_pass(const u32* kin, const u32* iin, u32* kout, u32* iout, size_t n, u32 base, u32 count,
                                             u32 word, u32 shift, const u32* gbase, u32 n_tiles, u32 tile, u32* cnt, u32* woff,
                                             u32* sc) {
    const u32 tid = threadIdx.x, w = tid >> 6, lane = tid & 63u;
    HK_UNROLL for (u32 k = 0; k < 4; k++) cnt[k * 256 + tid] = 0;
    __syncthreads();
    const u32* kw = kin + (size_t)word * n;
    const u64 below_me = ((u64)1 << lane) - 1;
    u32 pk[TS_ROUNDS];                                             // digit << 16 | rank within the wave's quarter (< 512)
    HK_UNROLL for (u32 r = 0; r < TS_ROUNDS; r++) {
        const u32 t = w * (TS_TILE / 4) + r * 64 + lane;
        const bool valid = t < count;
        const u32 d = valid ? (kw[(size_t)base + t] >> shift) & 255u : 0u;
        u64 m = __ballot(valid);                                   // the valid lanes of this step with my digit
        HK_UNROLL for (u32 b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const u64 bb = __ballot(bit);
            m &= bit ? bb : ~bb;
        }
        // the wave's earlier steps: read by every peer, then advanced by the lowest one - one instruction after the other
        // for the whole wave, on a row of cnt no other wave touches.  Relaxed wave-scope atomics (a plain ds_read / ds_write
        // each, never cached in a register) between wave-scope fences (no code: they keep the compiler from moving either).
        const u32 old = __hip_atomic_load(&cnt[w * 256 + d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        const u32 before = (u32)__popcll(m & below_me);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (valid && before == 0)
            __hip_atomic_store(&cnt[w * 256 + d], old + (u32)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        pk[r] = (d << 16) | (old + before);
    }
    __syncthreads();
    // lane d of the workgroup: where digit d of each wave starts
    const u32 c0 = cnt[tid], c1 = cnt[256 + tid], c2 = cnt[512 + tid], c3 = cnt[768 + tid];
    u32 start;
    if (gbase) {
        start = gbase[(size_t)tid * n_tiles + tile];
    } else {
        const u32 tot = c0 + c1 + c2 + c3;
        start = wg_scan_u32(sc, tid, tot) - tot;       // gbase is the kernel's argument: the branch is uniform
    }
    woff[tid] = start;
    woff[256 + tid] = start + c0;
    woff[512 + tid] = start + c0 + c1;
    woff[768 + tid] = start + c0 + c1 + c2;
    __syncthreads();
    HK_UNROLL for (u32 r = 0; r < TS_ROUNDS; r++) {
        const u32 t = w * (TS_TILE / 4) + r * 64 + lane;
        if (t < count) {
            const u32 pos = woff[w * 256 + (pk[r] >> 16)] + (pk[r] & 0xffffu);
            HK_UNROLL for (int k = 0; k < W; k++) kout[(size_t)k * n + pos] = kin[(size_t)k * n + base + t];
            iout[pos] = iin[(size_t)base + t];
        }
    }
    __syncthreads();
}

template <int W>
__global__ void __launch_bounds__(256)
k_ts_scatter(const u32* __restrict__ kin, const u32* __restrict__ iin, u32* __restrict__ kout, u32* __restrict__ iout, u32 n,
             u32 word, u32 shift, const u32* __restrict__ gbase, u32 n_tiles) {
    __shared__ u32 cnt[4 * 256], woff[4 * 256], sc[256];
    const u32 base = blockIdx.x * TS_TILE;
    const u32 count = n - base < TS_TILE ? n - base : TS_TILE;
    ts_tile_pass<W>(kin, iin, kout, iout, n, base, count, word, shift, gbase, n_tiles, blockIdx.x, cnt, woff, sc);
}

// out entry j = in entry idx[j], 16 B per lane
template <int K>
__global__ void __launch_bounds__(256)
k_ts_gather(const uint4* __restrict__ in, const u32* __restrict__ idx, u32 n, uint4* __restrict__ out) {
    constexpr u32 Q = 2 * K;                                       // 16-B quarters of an entry
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= (u64)n * Q) return;
    const u32 j = (u32)(g / Q), q = (u32)(g % Q);
    out[g] = in[(size_t)idx[j] * Q + q];
}

// The whole sort of n <= TS_TILE entries in ONE workgroup, a barrier between the steps (as k_et_tree_tail does): keys, every
// pass whose digit varies, the gather.  ka / kb, ia / ib: the ping-pong buffers; perm: the final index vector.  On a key
// that does not fit: flags[0] = 1 and nothing else is written to out / perm.
template <class Fr, int K>
__global__ void __launch_bounds__(256)
k_ts_small(const Fr* entries, u32 n, u32* ka, u32* kb, u32* ia, u32* ib, u32* flags, Fr* out, u32* perm) {
    constexpr int W = K == 2 ? 2 : 3;
    __shared__ u32 cnt[4 * 256], woff[4 * 256], sc[256], s[TS_FLAG_WORDS];
    const u32 tid = threadIdx.x;
    if (tid < TS_FLAG_WORDS) s[tid] = tid >= 4 ? ~0u : 0u;
    __syncthreads();
    HK_NOUNROLL for (u32 i = tid; i < n; i += 256) {
        u32 kw[W];
        const bool ok = ts_key_words<Fr, K>(entries + (size_t)i * K, kw);
        HK_UNROLL for (int w = 0; w < W; w++) ka[(size_t)w * n + i] = kw[w];
        ia[i] = i;
        ts_note_key<W>(s, ok, kw);
    }
    __syncthreads();
    if (tid < TS_FLAG_WORDS) flags[tid] = s[tid];
    if (s[0]) return;                                              // uniform: every lane reads the same word
    HK_NOUNROLL for (u32 p = 0; p < 4 * W; p++) {
        const u32 word = p >> 2, shift = (p & 3u) * 8;
        if ((((s[1 + word] & ~s[4 + word]) >> shift) & 255u) == 0) continue;      // uniform
        ts_tile_pass<W>(ka, ia, kb, ib, n, 0, n, word, shift, nullptr, 1, 0, cnt, woff, sc);
        u32* t = ka; ka = kb; kb = t;
        t = ia; ia = ib; ib = t;
    }
    const uint4* in4 = reinterpret_cast<const uint4*>(entries);
    uint4* out4 = reinterpret_cast<uint4*>(out);
    constexpr u32 Q = 2 * K;
    HK_NOUNROLL for (u32 g = tid; g < n * Q; g += 256) out4[g] = in4[(size_t)ia[g / Q] * Q + g % Q];
    HK_NOUNROLL for (u32 i = tid; i < n; i += 256) perm[i] = ia[i];
}

// row b <- (addr, val) of the K time-ordered entries from offs[b], then of the K address-ordered ones; 16 B per lane
template <int UNUSED>
__global__ void __launch_bounds__(256)
k_s0_rows(const uint4* __restrict__ time_e, const uint4* __restrict__ addr_e, const u32* __restrict__ offs, u64 total, u32 K,
          uint4* __restrict__ w_out) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const u32 per = 8 * K;                                         // 16-B quarters of a row: 4 K Fr
    const u32 b = (u32)(g / per), c = (u32)(g % per);
    const u64 from = (u64)offs[b] * 4;                             // an entry is 2 Fr = 4 quarters
    const bool first = c < 4 * K;                                  // one load through a selected address: no if / else join
    const uint4* src = first ? time_e : addr_e;
    w_out[g] = src[from + (first ? c : c - 4 * K)];
}

#endif  // __HIPCC__

template <class C>
hk_status Ops<C>::trace_sort(hk_ctx* ctx, uint32_t entry_fields, const void* time_entries, size_t n, void* addr_out,
                             uint32_t* perm_out) {
    const size_t K = entry_fields;
    if (K != 2 && K != 4) return HK_ERR_ARG;
    if (n >= ((size_t)1 << 31)) return HK_ERR_ARG;
    if (n == 0) return HK_OK;
    if (!time_entries || !addr_out) return HK_ERR_ARG;
    const size_t bytes = n * K * sizeof(Fr);
    if (bufs_overlap(addr_out, bytes, time_entries, bytes) || bufs_overlap(perm_out, 4 * n, time_entries, bytes)) return HK_ERR_ARG;

    const u32 W = K == 2 ? 2 : 3, nn = (u32)n;
    const u32 n_tiles = (nn + TS_TILE - 1) / TS_TILE, n_hist = 256 * n_tiles;
    Staged in = staged(time_entries, bytes);
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    u32 *keys[2], *idx[2], *hist, *gbase, *tops, *flags;
    Fr* sorted;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, &in, 1);
        for (int k = 0; k < 2; k++) keys[k] = c.n<u32>((size_t)W * n);
        for (int k = 0; k < 2; k++) idx[k] = c.n<u32>(n + (k ? n : 0));     // the second one: + the small form's perm
        hist = c.n<u32>(n_hist);
        gbase = c.n<u32>(n_hist);
        tops = c.n<u32>(scan_u32_tops_len(n_hist));
        flags = c.n<u32>(TS_FLAG_WORDS);
        sorted = c.n<Fr>(n * K);
    }));
    hipStream_t s = L->stream;
    HK_TRY(stage_upload(L, &in, 1));
    const Fr* tp = (const Fr*)in.p;
    u32 fl[TS_FLAG_WORDS] = {0, 0, 0, 0, ~0u, ~0u, ~0u, 0};
    const u32* perm = nullptr;
    if (n_tiles == 1) {
        u32* perm_s = idx[1] + n;
        if (K == 2)
            HK_LAUNCH((k_ts_small<Fr, 2>), dim3(1), dim3(256), 0, s, tp, nn, keys[0], keys[1], idx[0], idx[1], flags, sorted, perm_s);
        else
            HK_LAUNCH((k_ts_small<Fr, 4>), dim3(1), dim3(256), 0, s, tp, nn, keys[0], keys[1], idx[0], idx[1], flags, sorted, perm_s);
        HK_HIP(hipMemcpyAsync(fl, flags, sizeof(fl), hipMemcpyDeviceToHost, s));
        HK_HIP(hipStreamSynchronize(s));
        if (fl[0]) { HK_TRY(L->settle()); return HK_ERR_ARG; }
        perm = perm_s;
    } else {
        HK_HIP(hipMemcpyAsync(flags, fl, sizeof(fl), hipMemcpyHostToDevice, s));
        if (K == 2)
            HK_LAUNCH((k_ts_keys<Fr, 2>), dim3((nn + 255) / 256), dim3(256), 0, s, tp, nn, keys[0], idx[0], flags);
        else
            HK_LAUNCH((k_ts_keys<Fr, 4>), dim3((nn + 255) / 256), dim3(256), 0, s, tp, nn, keys[0], idx[0], flags);
        HK_HIP(hipMemcpyAsync(fl, flags, sizeof(fl), hipMemcpyDeviceToHost, s));
        HK_HIP(hipStreamSynchronize(s));                           // the one read-back: the error bit and the varying bits
        if (fl[0]) { HK_TRY(L->settle()); return HK_ERR_ARG; }
        int cur = 0;
        for (u32 p = 0; p < 4 * W; p++) {
            const u32 word = p >> 2, shift = (p & 3u) * 8;
            if ((((fl[1 + word] & ~fl[4 + word]) >> shift) & 255u) == 0) continue;        // this digit is the same in every key
            const u32 *kin = keys[cur], *iin = idx[cur];
            HK_LAUNCH((k_ts_hist<0>), dim3(n_tiles), dim3(256), 0, s, kin + (size_t)word * n, nn, shift, n_tiles, hist);
            HK_TRY(scan_u32(s, hist, gbase, tops, n_hist));
            if (W == 2)
                HK_LAUNCH((k_ts_scatter<2>), dim3(n_tiles), dim3(256), 0, s, kin, iin, keys[cur ^ 1], idx[cur ^ 1], nn, word,
                          shift, (const u32*)gbase, n_tiles);
            else
                HK_LAUNCH((k_ts_scatter<3>), dim3(n_tiles), dim3(256), 0, s, kin, iin, keys[cur ^ 1], idx[cur ^ 1], nn, word,
                          shift, (const u32*)gbase, n_tiles);
            cur ^= 1;
        }
        const u32 blocks = (u32)((n * 2 * K + 255) / 256);
        if (K == 2)
            HK_LAUNCH((k_ts_gather<2>), dim3(blocks), dim3(256), 0, s, (const uint4*)tp, (const u32*)idx[cur], nn, (uint4*)sorted);
        else
            HK_LAUNCH((k_ts_gather<4>), dim3(blocks), dim3(256), 0, s, (const uint4*)tp, (const u32*)idx[cur], nn, (uint4*)sorted);
        perm = idx[cur];
    }
    HK_HIP(hipMemcpyAsync(addr_out, sorted, bytes, is_device_ptr(addr_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (perm_out)
        HK_HIP(hipMemcpyAsync(perm_out, perm, 4 * n, is_device_ptr(perm_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    return L->settle();
}

template <class C>
hk_status Ops<C>::stage0_witness(hk_ctx* ctx, const uint32_t* offsets, uint32_t n_sub, uint32_t n_portals, const void* time_entries,
                                 const void* addr_entries, const uint32_t* sub_index, size_t batch, void* w_out) {
    if (!offsets || !time_entries || !addr_entries || (batch && (!sub_index || !w_out))) return HK_ERR_ARG;
    const size_t K = n_portals;
    if (K == 0 || K > (1u << 16) || batch >= (1u << 20) || batch * K >= ((size_t)1 << 28)) return HK_ERR_ARG;   // lanes of k_s0_rows
    std::vector<u32> rows, offs(batch);                    // each row's first entry; outlives the lane's copy
    HK_TRY(portal_rows(offsets, n_sub, K, sub_index, batch, rows));
    for (size_t b = 0; b < batch; b++) offs[b] = rows[2 * b + 1];
    if (batch == 0) return HK_OK;
    if (!is_device_ptr(w_out)) return HK_ERR_ARG;
    const size_t bytes = (size_t)offsets[n_sub] * 2 * sizeof(Fr);
    Staged in[2] = {staged(time_entries, bytes), staged(addr_entries, bytes)};
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    u32* offs_d;
    HK_TRY(L->carve([&](Carve& c) {
        stage_carve(c, in, 2);
        offs_d = c.n<u32>(batch);
    }));
    hipStream_t s = L->stream;
    HK_TRY(stage_upload(L, in, 2));
    const void *te = in[0].p, *ae = in[1].p;
    HK_HIP(hipMemcpyAsync(offs_d, offs.data(), 4 * batch, hipMemcpyHostToDevice, s));
    const u64 total = (u64)batch * 8 * K;                  // < 2^31
    HK_LAUNCH((k_s0_rows<0>), dim3((u32)((total + 255) / 256)), dim3(256), 0, s, (const uint4*)te, (const uint4*)ae,
              (const u32*)offs_d, total, (u32)K, (uint4*)w_out);
    return L->settle();
}

}  // namespace hk
