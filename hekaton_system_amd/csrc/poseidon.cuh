// poseidon.cuh — Poseidon on the device, stated once (DESIGN.md section 4h "Poseidon on a quad of lanes"): the permutation with
// the state spread over the four lanes of a quad, with or without the trace of its witnesses; the two absorb patterns of the
// execution tree (the two-to-one input and the rate-3 leaf sponge); and the membership walk every job's stage-1 witness and
// hk_poseidon_path run.  PoseidonDesc and the lengths of a trace: job_args.h (host only).
#pragma once
#include "hk_internal.h"
#include "job_args.h"
#include "ntt.cuh"           // fr_load, fr_store

namespace hk {

constexpr u32 S1_WG_ROWS = 64;         // rows of one 256-lane workgroup of k_poseidon_membership (a quad each)

#if defined(__HIPCC__)

template <class Fr>
__device__ __forceinline__ Fr fr_select(bool take, const Fr& a, const Fr& b) {
    Fr r;
    HK_UNROLL for (int i = 0; i < Fr::N; i++) r.v[i] = take ? a.v[i] : b.v[i];
    return r;
}

// ---- Poseidon on a quad of lanes ---------------------------------------------------------------------------------------
// State element i lives on lane i of a quad (lanes 4 t .. 4 t + 3); with T = 3 the fourth lane computes along on element 0's
// constants and its value is never read.  A round per lane: add its own round constant, raise its own element to ALPHA
// (in a partial round every lane still does, and lanes != 0 then keep their input: a select, no branch), read the T S-box
// outputs of the quad over DPP quad_perm broadcasts and form its own MDS row - 3 + 4 dependent products at T = 4,
// ALPHA = 5 and 5 + 3 at T = 3, ALPHA = 17, instead of 28 / 24 with one lane per state.  All four lanes of a quad must be
// active at every call (DPP reads an inactive lane as 0): callers guard their stores, never the call.
template <class Fr, int CTRL>
__device__ __forceinline__ Fr quad_bcast(const Fr& v) {
    Fr r;
    HK_UNROLL for (int i = 0; i < Fr::N; i++) r.v[i] = (u32)__builtin_amdgcn_update_dpp(0, (int)v.v[i], CTRL, 0xf, 0xf, true);
    return r;
}

// TRACE: the witnesses go to w in sha_circuit.poseidon_trace's order.  In a round that starts at w, lane i < T stores its S-box
// chain (L = 3 values at ALPHA 5, 5 at 17) at w + i L + step when the round is full or i = 0, and its new state element at
// w + (full ? T : 1) L + i; w advances by the same amount on every lane.  `store` is false on the lanes of a quad past the
// batch: they and the fourth lane at T = 3 compute along (every lane of a quad is in every DPP exchange) and write nothing.
// Without TRACE, `store` and w are not looked at.
// Zero rounds (hk_poseidon_path admits them): the loop does not run and the prefetch of the first round constant reads ark[qc],
// which is then element qc of the first MDS row - inside n_consts by the entry's bound off + (rf + rp) T + T T <= n_consts.
// Besides it only the lane's MDS row is loaded.
template <class Fr, int T, int ALPHA, bool TRACE>
__device__ __forceinline__ Fr poseidon_permute_quad(const Fr* __restrict__ consts, const PoseidonDesc& d, Fr s, bool store, Fr*& w) {
    static_assert(T == 3 || T == 4, "one state element per lane of a quad");
    constexpr u32 L = ALPHA == 5 ? 3 : 5;
    const u32 q = threadIdx.x & 3u;
    const u32 qc = q < (u32)T ? q : 0u;
    const Fr* ark = consts + d.off;
    const Fr* mds = ark + (size_t)(d.rf + d.rp) * T;
    const u32 rounds = d.rf + d.rp, half = d.rf / 2;
    const bool mine = store && q < (u32)T;
    Fr m[T];
    HK_UNROLL for (int j = 0; j < T; j++) m[j] = fr_load(&mds[qc * T + j]);
    Fr k = fr_load(&ark[qc]);
    HK_NOUNROLL for (u32 r = 0; r < rounds; r++) {
        const bool full = r < half || r >= half + d.rp;
        const bool keep = full || q == 0;
        const bool trace = mine && keep;
        Fr* c = w + qc * L;
        Fr y = Fr::add(s, k);
        k = fr_load(&ark[(r + 1 < rounds ? r + 1 : r) * T + qc]);       // the next round's constant, under this round's products
        Fr x = Fr::mul(y, y);
        if constexpr (TRACE) if (trace) fr_store(c++, x);
        HK_UNROLL for (int e = 0; e < (ALPHA == 5 ? 1 : 3); e++) {
            x = Fr::mul(x, x);
            if constexpr (TRACE) if (trace) fr_store(c++, x);
        }
        x = Fr::mul(x, y);
        if constexpr (TRACE) if (trace) fr_store(c, x);
        x = fr_select(keep, x, y);
        s = Fr::mul(m[0], quad_bcast<Fr, 0x00>(x));
        s = Fr::add(s, Fr::mul(m[1], quad_bcast<Fr, 0x55>(x)));
        s = Fr::add(s, Fr::mul(m[2], quad_bcast<Fr, 0xAA>(x)));
        if constexpr (T == 4) s = Fr::add(s, Fr::mul(m[3], quad_bcast<Fr, 0xFF>(x)));
        if constexpr (TRACE) {
            w += (full ? (u32)T : 1u) * L;
            if (mine) fr_store(&w[qc], s);
            w += T;
        }
    }
    return s;
}
template <class Fr, int T, int ALPHA>
__device__ __forceinline__ Fr poseidon_permute_quad(const Fr* __restrict__ consts, const PoseidonDesc& d, Fr s) {
    Fr* none = nullptr;
    return poseidon_permute_quad<Fr, T, ALPHA, false>(consts, d, s, false, none);
}

// the input of a two-to-one hash, (0, left, right, -) on lanes 0 .. 3: `left` is read on lane 1 and `right` on lane 2 alone, so
// a caller whose lanes each hold one of the two passes that value for both
template <class Fr>
__device__ __forceinline__ Fr poseidon_pair_input(const Fr& left, const Fr& right) {
    const u32 q = threadIdx.x & 3u;
    return fr_select(q == 1, left, fr_select(q == 2, right, Fr::zero()));
}

// the rate-3 sponge over the nf = 4 or 6 fields of a leaf (poseidon.PoseidonConfig.crh: capacity element first, absorb three,
// permute, absorb the rest, permute); the digest is state[1], on lane 1 of what this returns
template <class Fr, bool TRACE>
__device__ __forceinline__ Fr poseidon_leaf_sponge(const Fr* __restrict__ consts, const PoseidonDesc& d, const Fr* __restrict__ leaf,
                                                   u32 nf, bool store, Fr*& w) {
    const u32 q = threadIdx.x & 3u;
    // every lane loads (an index it may read) and selects: no branch inside the quad
    Fr s = fr_select(q != 0, fr_load(&leaf[q ? q - 1 : 0]), Fr::zero());
    s = poseidon_permute_quad<Fr, 4, 5, TRACE>(consts, d, s, store, w);
    const bool more = q != 0 && 2 + q < nf;
    s = Fr::add(s, fr_select(more, fr_load(&leaf[more ? 2 + q : 0]), Fr::zero()));
    return poseidon_permute_quad<Fr, 4, 5, TRACE>(consts, d, s, store, w);
}
template <class Fr>
__device__ __forceinline__ Fr poseidon_leaf_sponge(const Fr* __restrict__ consts, const PoseidonDesc& d, const Fr* __restrict__ leaf,
                                                   u32 nf) {
    Fr* none = nullptr;
    return poseidon_leaf_sponge<Fr, false>(consts, d, leaf, nf, false, none);
}

// ---- the membership walk -----------------------------------------------------------------------------------------------
// One quad per row b of z: the membership block - leaf leaves[i] of NF fields, path siblings[i], direction bits from idx - in
// the order of sha_circuit.poseidon_path_trace, at column col0 of the row.  i = src[stride b], or b itself without src;
// idx = index[stride b].  A quad past the batch recomputes the last row and stores nothing: no lane leaves in front of a DPP read
// (DESIGN.md section 3b).  NF = 4 (a ROM leaf) or 6 (a RAM leaf).
// idx is any u32 and depth may be 32 (hk_poseidon_path): (idx >> l) & 1 is evaluated for l < depth <= 32 only, so no shift
// reaches the word's width.
template <class Fr, int NF>
__global__ void __launch_bounds__(256)
k_poseidon_membership(const Fr* __restrict__ consts, PoseidonDesc leaf_d, PoseidonDesc node_d, const Fr* __restrict__ leaves,
                      const Fr* __restrict__ siblings, const u32* __restrict__ src, const u32* __restrict__ index, u32 stride,
                      u32 depth, u32 batch, size_t n_v, size_t col0, Fr* __restrict__ z_out) {
    static_assert(NF == 4 || NF == 6, "an execution leaf has 2 + entry_fields fields");
    const u32 t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const u32 q = threadIdx.x & 3u;
    const bool store = t < batch;
    const u32 b = store ? t : batch - 1;
    const u32 i = src ? src[stride * b] : b;
    const u32 idx = index[stride * b];
    Fr* w = z_out + (size_t)b * n_v + col0;
    Fr s = poseidon_leaf_sponge<Fr, true>(consts, leaf_d, leaves + (size_t)i * NF, NF, store, w);
    Fr cur = quad_bcast<Fr, 0x55>(s);
    HK_NOUNROLL for (u32 l = 0; l < depth; l++) {
        const Fr sib = fr_load(&siblings[(size_t)i * depth + l]);
        const bool bit = (idx >> l) & 1u;
        const Fr left = fr_select(bit, sib, cur), right = fr_select(bit, cur, sib);
        // bit / sibling / left: lane 0, 1, 2 one each
        Fr v = fr_select(q == 1, sib, left);
        v = fr_select(q == 0, bit ? Fr::one() : Fr::zero(), v);
        if (store && q < 3) fr_store(&w[q], v);
        w += 3;
        s = poseidon_permute_quad<Fr, 3, 17, true>(consts, node_d, poseidon_pair_input(left, right), store, w);
        cur = quad_bcast<Fr, 0x55>(s);
    }
}

#endif  // __HIPCC__

// the membership block of every row on stream s: behind the kernels that fill the row's other columns in a job entry (src =
// index = its rows, stride 2: no table of its own), the whole of hk_poseidon_path (src NULL, stride 1)
template <class Fr, int NF>
hk_status poseidon_membership(hipStream_t s, const void* consts, const hk_poseidon_desc* leaf_hash, const hk_poseidon_desc* node_hash,
                              const void* leaves, const void* siblings, const u32* src, const u32* index, u32 stride, size_t depth,
                              size_t batch, size_t n_v, size_t col0, void* z_out) {
    const u32 nb = (u32)batch;
    HK_LAUNCH((k_poseidon_membership<Fr, NF>), dim3((nb + S1_WG_ROWS - 1) / S1_WG_ROWS), dim3(256), 0, s, (const Fr*)consts,
              poseidon_desc(leaf_hash), poseidon_desc(node_hash), (const Fr*)leaves, (const Fr*)siblings, src, index,
              stride, (u32)depth, nb, n_v, col0, (Fr*)z_out);
    return HK_OK;
}

}  // namespace hk
