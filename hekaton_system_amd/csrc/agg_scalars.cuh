// agg_scalars.cuh — the aggregator's scalar vectors on the device (hk_scalar_powers, hk_ipa_quotient):
// the twist / trapdoor powers of `structured_scalar_power` (distributed-prover/src/pairing_ops.rs:42-48) and the KZG witness
// polynomials of the folded keys (kzg.rs:122-155: `ipa_polynomial`, `&poly / (X - z)`, resize).
//
//   powers     one lane per chunk of AQ_CHUNK consecutive exponents: x^(8 t) from the bits of t over the host's table
//              x^(8 2^k), then seven products by x.  reps on grid.y.
//   quotient   f(X) = X^shift prod_k (1 + a_k X^(2^k)), a_k = c_k rho^(2^k) (host).  Coefficient i is 0 below shift, else the
//              product of the a_k over the set bits of i - shift: the bits above the third once per lane, the three low bits
//              from a table of their eight combinations (host).  With S(i) = sum_{j >= i} f_j z^(j - i) the quotient is
//              q[m] = S(m + 1) (q[len - 1] = S(len) = 0), and over chunks of AQ_CHUNK coefficients S(8 t) = P_t + z^8 S(8 t + 8):
//              (1) k_ipaq_chunk      P_t = sum_j f_(8 t + j) z^j
//              (2) k_ipaq_scan_tile  per tile of AQ_TILE chunks the suffix sums V_t = sum_j z^(8 j) P_(t + j) within the tile
//                                    (Kogge-Stone: the multiplier is constant, so a step over distance d is one product by
//                                    z^(8 d)), in place; V of the tile's first chunk into tops
//                  k_ipaq_scan_tops  tops[b] <- the suffix over the tiles AFTER b (one workgroup, ceil(tiles / 64)
//                                    consecutive tiles per lane)
//              (3) k_ipaq_walk       S(8 t + 8) = V_(t + 1) + z^(8 (255 - tid)) tops[tile], then down the chunk:
//                                    acc = f_i + z acc, q[i - 1] = acc
//              k_ipaq_tail runs all three in one workgroup when the whole length is one tile.
//
// The chunk-level bodies are HK_HD functions of (table, shape, chunk index), so a host program runs them chunk by chunk with a
// serial scan in between (tests/host_shim/agg_scalars_shim.cpp); only the LDS scans are device-only.
#pragma once
#include "ec.cuh"
#include "ntt.cuh"

namespace hk {

constexpr u32 AQ_CHUNK = 8;            // exponents / coefficients per lane
constexpr u32 AQ_TILE = 256;           // chunks per scan tile (one per lane of a workgroup)
constexpr u32 AQ_TOPS_LANES = 64;      // lanes of the scan over the tile totals: each takes ceil(tiles / 64) consecutive tiles
constexpr u32 AQ_MAX_L = 26;           // challenges of a quotient
constexpr u32 AQ_MAX_LOG = 27;         // log2 of the longest vector of either call

// the powers' table: x, then x^(8 2^k)
constexpr u32 AQ_PW_X = 0, AQ_PW_SQ = 1, AQ_PW_BITS = AQ_MAX_LOG - 3, AQ_PW_LEN = AQ_PW_SQ + AQ_PW_BITS;
// the quotient's table: z; the eight products of a_0, a_1, a_2; a_k; z^(8 2^k), k < 8; (z^(8 256))^(per 2^k), k < 6; z^(8 j),
// j <= AQ_TILE.  A single-tile quotient reads nothing from AQ_QP on.
constexpr u32 AQ_Z = 0, AQ_LOW = 1, AQ_A = AQ_LOW + 8, AQ_ZS = AQ_A + AQ_MAX_L, AQ_QP = AQ_ZS + 8, AQ_PZ = AQ_QP + 6,
              AQ_LEN = AQ_PZ + AQ_TILE + 1;

struct AqShape {
    u64 shift, len;                    // len = shift + 2^l
    u32 l, n_chunks;                   // n_chunks = ceil(len / AQ_CHUNK)
};

template <class Fr>
HK_HD Fr aq_ld(const Fr* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fr_load(p);
#else
    return *p;
#endif
}
template <class Fr>
HK_HD void aq_st(Fr* p, const Fr& v) {             // memory is always canonical
#if defined(__HIP_DEVICE_COMPILE__)
    fr_store(p, v);
#else
    *p = v;
#endif
}
template <class Fr>
HK_HD Fr aq_select(bool take, const Fr& a, const Fr& b) {
    Fr r;
    HK_UNROLL for (int i = 0; i < Fr::N; i++) r.v[i] = take ? a.v[i] : b.v[i];
    return r;
}

// product of tab[k] over the set bits k < nbits of e.  Every lane multiplies at every bit (by one where the bit is clear).
template <class Fr>
HK_HD Fr aq_bits_product(const Fr* tab, u64 e, u32 nbits) {
    Fr acc = Fr::one();
    HK_NOUNROLL for (u32 k = 0; k < nbits; k++)
        acc = Fr::mul(acc, aq_select<Fr>((e >> k) & 1u, aq_ld(&tab[k]), Fr::one()));
    return acc;
}

// out[i] = x^i for the exponents i of chunk t below n; nbits: the bit length of the last chunk's index
template <class Fr>
HK_HD void aq_power_chunk(const Fr* tab, u32 t, u32 nbits, u64 n, Fr* out) {
    Fr pw = aq_bits_product<Fr>(tab + AQ_PW_SQ, t, nbits);
    const Fr x = aq_ld(&tab[AQ_PW_X]);
    HK_NOUNROLL for (u32 j = 0; j < AQ_CHUNK; j++) {
        const u64 i = (u64)t * AQ_CHUNK + j;
        if (i < n) aq_st(&out[i], pw);
        if (j + 1 < AQ_CHUNK) pw = Fr::mul(pw, x);
    }
}

// what a lane keeps for the coefficients of its chunk: the products over the high bits of the (at most two) groups of eight
// exponents i - shift that the chunk meets - one group when shift is a multiple of AQ_CHUNK
template <class Fr>
struct AqChunk {
    Fr h0, h1;
    u64 g0;
};
template <class Fr>
HK_HD AqChunk<Fr> aq_chunk_begin(const Fr* tab, const AqShape& s, u32 t) {
    const u64 i0 = (u64)t * AQ_CHUNK;
    const u32 nbits = s.l > 3 ? s.l - 3 : 0;
    AqChunk<Fr> c;
    c.g0 = ((i0 > s.shift ? i0 : s.shift) - s.shift) >> 3;
    c.h0 = aq_bits_product<Fr>(tab + AQ_A + 3, c.g0, nbits);
    c.h1 = c.h0;
    if (s.shift & (AQ_CHUNK - 1)) c.h1 = aq_bits_product<Fr>(tab + AQ_A + 3, c.g0 + 1, nbits);    // uniform over the launch
    return c;
}
// coefficient i of f, i in chunk c's range (or one past it); 0 outside [shift, len)
template <class Fr>
HK_HD Fr aq_coeff(const Fr* tab, const AqShape& s, const AqChunk<Fr>& c, u64 i) {
    const bool in = i >= s.shift && i < s.len;
    const u64 u = in ? i - s.shift : 0;
    const Fr h = aq_select<Fr>((u >> 3) == c.g0, c.h0, c.h1);
    return aq_select<Fr>(in, Fr::mul(h, aq_ld(&tab[AQ_LOW + (u32)(u & 7u)])), Fr::zero());
}
// coefficient of one index on its own (tests)
template <class Fr>
HK_HD Fr aq_coeff_at(const Fr* tab, const AqShape& s, u64 i) {
    return aq_coeff<Fr>(tab, s, aq_chunk_begin<Fr>(tab, s, (u32)(i / AQ_CHUNK)), i);
}

// P_t = sum_j f_(8 t + j) z^j
template <class Fr>
HK_HD Fr aq_chunk_horner(const Fr* tab, const AqShape& s, u32 t) {
    const AqChunk<Fr> c = aq_chunk_begin<Fr>(tab, s, t);
    const Fr z = aq_ld(&tab[AQ_Z]);
    Fr acc = Fr::zero();
    HK_NOUNROLL for (u32 j = AQ_CHUNK; j-- > 0;)
        acc = Fr::add(aq_coeff<Fr>(tab, s, c, (u64)t * AQ_CHUNK + j), Fr::mul(z, acc));
    return acc;
}

// q[m] = S(m + 1) for the m of chunk t below len, walking down from next = S(8 t + 8): the suffix value of the NEXT chunk
template <class Fr>
HK_HD void aq_chunk_walk(const Fr* tab, const AqShape& s, u32 t, const Fr& next, Fr* q) {
    const AqChunk<Fr> c = aq_chunk_begin<Fr>(tab, s, t);
    const Fr z = aq_ld(&tab[AQ_Z]);
    Fr acc = next;
    HK_NOUNROLL for (u32 j = AQ_CHUNK; j-- > 0;) {
        const u64 m = (u64)t * AQ_CHUNK + j;
        if (j + 1 < AQ_CHUNK) acc = Fr::add(aq_coeff<Fr>(tab, s, c, m + 1), Fr::mul(z, acc));
        if (m < s.len) aq_st(&q[m], acc);
    }
}

// ---- the tables, on the host -------------------------------------------------------------------------------------------
template <class Fr>
inline void aq_powers_table(const Fr& x, Fr* tab) {
    tab[AQ_PW_X] = x;
    Fr p = x;
    for (int i = 0; i < 3; i++) p = Fr::mul(p, p);
    for (u32 k = 0; k < AQ_PW_BITS; k++) {
        tab[AQ_PW_SQ + k] = p;
        p = Fr::mul(p, p);
    }
}
// tab: AQ_LEN Fr; per: the tiles per lane of the scan over the tile totals (the AQ_QP entries), or 0 for a single-tile
// quotient, whose kernel reads nothing from AQ_QP on: those entries stay zero
template <class Fr>
inline void aq_quotient_table(const Fr* challenges, u32 l, const Fr& rho, const Fr& z, u32 per, Fr* tab) {
    for (u32 i = 0; i < AQ_LEN; i++) tab[i] = Fr::zero();
    tab[AQ_Z] = z;
    Fr pw = rho;
    for (u32 k = 0; k < l; k++) {
        tab[AQ_A + k] = Fr::mul(challenges[k], pw);
        pw = Fr::mul(pw, pw);
    }
    for (u32 m = 0; m < 8; m++) {
        Fr p = Fr::one();
        for (u32 k = 0; k < 3 && k < l; k++)
            if ((m >> k) & 1u) p = Fr::mul(p, tab[AQ_A + k]);
        tab[AQ_LOW + m] = p;
    }
    Fr z8 = z;
    for (int i = 0; i < 3; i++) z8 = Fr::mul(z8, z8);
    Fr p = z8;
    for (u32 k = 0; k < 8; k++) {
        tab[AQ_ZS + k] = p;
        p = Fr::mul(p, p);
    }
    if (!per) return;
    tab[AQ_PZ] = Fr::one();
    for (u32 j = 1; j <= AQ_TILE; j++) tab[AQ_PZ + j] = Fr::mul(tab[AQ_PZ + j - 1], z8);
    Fr qp = Fr::one(), sq = tab[AQ_PZ + AQ_TILE];
    for (u32 e = per; e; e >>= 1) {
        if (e & 1u) qp = Fr::mul(qp, sq);
        sq = Fr::mul(sq, sq);
    }
    for (u32 k = 0; k < 6; k++) {
        tab[AQ_QP + k] = qp;
        qp = Fr::mul(qp, qp);
    }
}

}  // namespace hk

#if defined(__HIPCC__)
#include "curve_ops_impl.cuh"

namespace hk {

template <class Fr>
__global__ void __launch_bounds__(256) k_powers(const Fr* __restrict__ tab, u32 n_chunks, u32 nbits, u64 n, Fr* __restrict__ out) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_chunks) return;
    aq_power_chunk<Fr>(tab, t, nbits, n, out + (size_t)blockIdx.y * n);
}

// (1)
template <class Fr>
__global__ void __launch_bounds__(256) k_ipaq_chunk(const Fr* __restrict__ tab, AqShape s, Fr* __restrict__ part) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= s.n_chunks) return;
    fr_store(&part[t], aq_chunk_horner<Fr>(tab, s, t));
}

// inclusive suffix scan of v_t + m v_(t + 1) + m^2 v_(t + 2) + ... over a workgroup of W lanes (W a power of two <= 256);
// mult[k] = m^(2^k); s: W Fr of LDS.  Every lane multiplies in every step (a lane with nothing at that distance by zero),
// so no lane leaves the barriers.
template <class Fr, u32 W>
__device__ __forceinline__ Fr aq_wg_scan(Fr* s, u32 tid, Fr v, const Fr* __restrict__ mult) {
    s[tid] = v;
    __syncthreads();
    u32 k = 0;
    HK_NOUNROLL for (u32 off = 1; off < W; off <<= 1, k++) {
        const bool has = tid + off < W;
        Fr x = s[has ? tid + off : tid];
        x = aq_select<Fr>(has, x, Fr::zero());
        __syncthreads();
        v = Fr::add(v, Fr::mul(x, fr_load(&mult[k])));
        s[tid] = v;
        __syncthreads();
    }
    return v;
}

// (2a) per tile: part[t] <- V_t (in place), the first lane's V into tops
template <class Fr>
__global__ void __launch_bounds__(AQ_TILE)
k_ipaq_scan_tile(const Fr* __restrict__ tab, Fr* __restrict__ part, Fr* __restrict__ tops, u32 n_chunks) {
    __shared__ Fr s[AQ_TILE];
    const u32 tid = threadIdx.x;
    const u32 t = blockIdx.x * AQ_TILE + tid;
    const bool in = t < n_chunks;
    Fr v = Fr::zero();
    if (in) v = fr_load(&part[t]);
    v = aq_wg_scan<Fr, AQ_TILE>(s, tid, v, tab + AQ_ZS);
    if (in) fr_store(&part[t], v);
    if (tid == 0) fr_store(&tops[blockIdx.x], v);
}

// (2b) tops[b] <- sum_{j >= 1} Q^(j - 1) tops[b + j], Q = z^(8 AQ_TILE): the suffix value at the first chunk after tile b.
// One workgroup: lane t takes the `per` consecutive tiles [t per, (t + 1) per) - their Horner value, a scan over the lanes
// with the multiplier Q^per, then the running value back down its tiles.
template <class Fr>
__global__ void __launch_bounds__(AQ_TOPS_LANES) k_ipaq_scan_tops(const Fr* __restrict__ tab, Fr* __restrict__ tops, u32 n_tiles) {
    __shared__ Fr s[AQ_TOPS_LANES];
    const u32 tid = threadIdx.x;
    const u32 per = (n_tiles + AQ_TOPS_LANES - 1) / AQ_TOPS_LANES;
    const Fr Q = fr_load(&tab[AQ_PZ + AQ_TILE]);
    Fr acc = Fr::zero();
    HK_NOUNROLL for (u32 j = per; j-- > 0;) {
        const u32 i = tid * per + j;
        Fr x = Fr::zero();
        if (i < n_tiles) x = fr_load(&tops[i]);
        acc = Fr::add(x, Fr::mul(Q, acc));
    }
    aq_wg_scan<Fr, AQ_TOPS_LANES>(s, tid, acc, tab + AQ_QP);
    const bool has = tid + 1 < AQ_TOPS_LANES;
    Fr run = aq_select<Fr>(has, s[has ? tid + 1 : tid], Fr::zero());
    HK_NOUNROLL for (u32 j = per; j-- > 0;) {
        const u32 i = tid * per + j;
        Fr x = Fr::zero();
        if (i < n_tiles) {
            x = fr_load(&tops[i]);
            fr_store(&tops[i], run);
        }
        run = Fr::add(x, Fr::mul(Q, run));
    }
}

// (3) one lane per chunk, a workgroup per tile
template <class Fr>
__global__ void __launch_bounds__(AQ_TILE)
k_ipaq_walk(const Fr* __restrict__ tab, AqShape s, const Fr* __restrict__ part, const Fr* __restrict__ tops, Fr* __restrict__ q) {
    const u32 tid = threadIdx.x;
    const u32 t = blockIdx.x * AQ_TILE + tid;
    if (t >= s.n_chunks) return;
    const bool has = tid + 1 < AQ_TILE && t + 1 < s.n_chunks;
    Fr next = Fr::zero();
    if (has) next = fr_load(&part[t + 1]);
    next = Fr::add(next, Fr::mul(fr_load(&tab[AQ_PZ + AQ_TILE - 1 - tid]), fr_load(&tops[blockIdx.x])));
    aq_chunk_walk<Fr>(tab, s, t, next, q);
}

// all of it in ONE workgroup when n_chunks <= AQ_TILE: a chunk past the end has zero coefficients and stores nothing, so
// every lane runs every phase and meets every barrier
template <class Fr>
__global__ void __launch_bounds__(AQ_TILE) k_ipaq_tail(const Fr* __restrict__ tab, AqShape s, Fr* __restrict__ q) {
    __shared__ Fr sm[AQ_TILE];
    const u32 tid = threadIdx.x;
    aq_wg_scan<Fr, AQ_TILE>(sm, tid, aq_chunk_horner<Fr>(tab, s, tid), tab + AQ_ZS);
    const bool has = tid + 1 < AQ_TILE;
    const Fr next = aq_select<Fr>(has, sm[has ? tid + 1 : tid], Fr::zero());
    aq_chunk_walk<Fr>(tab, s, tid, next, q);
}

template <class C>
hk_status Ops<C>::scalar_powers(hk_ctx* ctx, const void* x_mont, size_t n, size_t reps, void* out) {
    if (n == 0 || reps == 0) return HK_OK;
    if (!x_mont || !out) return HK_ERR_ARG;
    const size_t cap = (size_t)1 << AQ_MAX_LOG;
    if (n > cap || reps > 65535 || reps > cap / n) return HK_ERR_ARG;       // reps rides on grid.y
    Fr x, tab[AQ_PW_LEN];
    memcpy(&x, x_mont, sizeof(Fr));
    aq_powers_table<Fr>(x, tab);
    const u32 n_chunks = (u32)((n + AQ_CHUNK - 1) / AQ_CHUNK);
    u32 nbits = 0;
    while (((u64)1 << nbits) < n_chunks) nbits++;
    Staged to = staged(out, reps * n * sizeof(Fr));
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    Fr* tab_d;
    HK_TRY(L->carve([&](Carve& c) {
        tab_d = c.n<Fr>(AQ_PW_LEN);
        stage_carve(c, &to, 1);
    }));
    hipStream_t s = L->stream;
    HK_HIP(hipMemcpyAsync(tab_d, tab, sizeof(tab), hipMemcpyHostToDevice, s));
    HK_LAUNCH((k_powers<Fr>), dim3((n_chunks + 255) / 256, (u32)reps), dim3(256), 0, s, (const Fr*)tab_d, n_chunks, nbits,
              (u64)n, (Fr*)to.p);
    HK_TRY(stage_download(L, &to, 1));
    return L->settle();                                                     // `tab` is read until here
}

template <class C>
hk_status Ops<C>::ipa_quotient(hk_ctx* ctx, const void* challenges_mont, size_t l, const void* rho_mont, const void* z_mont,
                               size_t shift, void* q_out) {
    const size_t cap = (size_t)1 << AQ_MAX_LOG;
    if ((l && !challenges_mont) || !rho_mont || !z_mont || !q_out) return HK_ERR_ARG;
    if (l > AQ_MAX_L || shift > cap || shift + ((size_t)1 << l) > cap) return HK_ERR_ARG;
    AqShape sh;
    sh.shift = shift;
    sh.len = shift + ((u64)1 << l);
    sh.l = (u32)l;
    sh.n_chunks = (u32)((sh.len + AQ_CHUNK - 1) / AQ_CHUNK);
    const u32 n_tiles = (sh.n_chunks + AQ_TILE - 1) / AQ_TILE, per = (n_tiles + AQ_TOPS_LANES - 1) / AQ_TOPS_LANES;
    const bool fused = n_tiles == 1;
    Fr ch[AQ_MAX_L], rho, z;
    memcpy(ch, challenges_mont, l * sizeof(Fr));
    memcpy(&rho, rho_mont, sizeof(Fr));
    memcpy(&z, z_mont, sizeof(Fr));
    std::vector<Fr> tab(AQ_LEN);
    aq_quotient_table<Fr>(ch, sh.l, rho, z, fused ? 0 : per, tab.data());
    const size_t n_tab = fused ? AQ_QP : AQ_LEN;
    Staged to = staged(q_out, sh.len * sizeof(Fr));
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    Fr *tab_d, *part = nullptr, *tops = nullptr;
    HK_TRY(L->carve([&](Carve& c) {
        tab_d = c.n<Fr>(n_tab);
        if (!fused) {
            part = c.n<Fr>(sh.n_chunks);
            tops = c.n<Fr>(n_tiles);
        }
        stage_carve(c, &to, 1);
    }));
    hipStream_t s = L->stream;
    HK_HIP(hipMemcpyAsync(tab_d, tab.data(), n_tab * sizeof(Fr), hipMemcpyHostToDevice, s));
    Fr* q = (Fr*)to.p;
    const Fr* tp = tab_d;
    if (fused) {
        HK_LAUNCH((k_ipaq_tail<Fr>), dim3(1), dim3(AQ_TILE), 0, s, tp, sh, q);
    } else {
        HK_LAUNCH((k_ipaq_chunk<Fr>), dim3(n_tiles), dim3(AQ_TILE), 0, s, tp, sh, part);
        HK_LAUNCH((k_ipaq_scan_tile<Fr>), dim3(n_tiles), dim3(AQ_TILE), 0, s, tp, part, tops, sh.n_chunks);
        HK_LAUNCH((k_ipaq_scan_tops<Fr>), dim3(1), dim3(AQ_TOPS_LANES), 0, s, tp, tops, n_tiles);
        HK_LAUNCH((k_ipaq_walk<Fr>), dim3(n_tiles), dim3(AQ_TILE), 0, s, tp, sh, (const Fr*)part, (const Fr*)tops, q);
    }
    HK_TRY(stage_download(L, &to, 1));
    return L->settle();                                                     // `tab` is read until here
}

}  // namespace hk
#endif  // __HIPCC__
