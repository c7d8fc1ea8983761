// keygen.cuh — CP-Groth16 trusted setup past synthesis on the device: hk_qap_eval and hk_keygen.
//
// Reference path restated (all scalar-field arithmetic on the device; this file sequences launches):
//   LibsnarkReduction::instance_map_with_evaluation     cp-groth16/src/generator.rs:75-76
//   the per-variable scalars (beta a_i + alpha b_i + c_i) / delta_k, / gamma    generator.rs:93-117
//   the h query t^i zt / delta_last                     generator.rs:182
//   FixedBase::msm + normalize_batch of every query     generator.rs:126-224
//
// Phases:
//   (a) Lagrange coefficients at t:  u_i = (zt / m) w^i / (t - w^i) for the n_c + n_inst rows that exist, KG_CHUNK
//       consecutive rows per lane starting from w^(first row), one inversion per lane (Montgomery's trick).
//   (b) out_j = sum_i M_ij u_i for each matrix, column-wise without field atomics: per-column counts (u32 atomics), an
//       exclusive scan, a scatter of u_i M_ij into column order, then bounded segmented sums - a column longer than
//       KG_SEG entries is cut into chunks of KG_SEG, each chunk summed by one lane into a partial, and the partials (again
//       in column order) go through the same step until no column is longer than KG_SEG; one lane per column finishes.
//       Field addition is exact, so the order of the terms does not change a bit of the result.
//   (c) one lane per variable: the canonical scalars of the bulk sweeps, gamma_abc and the committer-key scalars; the
//       h query per chunk of powers of t.
//   (d) the fixed-base sweeps of fixed_base.cuh over those device-resident scalars, one per output, each written into
//       the caller's buffer (device) or copied there (host).
#pragma once
#include "ntt_host.cuh"
#include "group_ops.cuh"
#include "csr.cuh"
#include "scan.cuh"

namespace hk {

constexpr u32 KG_CHUNK = 64;                 // consecutive powers per lane (Lagrange coefficients, h query)
constexpr u32 KG_SEG = 256;                  // longest run of one column a lane sums

// indices into the Fr constants a keygen / QAP call uploads (Montgomery)
enum { KC_ALPHA, KC_BETA, KC_G1S, KC_G2S, KC_GAMMA_INV_G1S, KC_H0, KC_T, KC_K, KC_WSQ, KC_TSQ = KC_WSQ + 32, KC_N = KC_TSQ + 32 };

#if defined(__HIPCC__)

// x^e from sq[j] = x^(2^j)
template <class Fr>
__device__ __forceinline__ Fr kg_pow(const Fr* __restrict__ sq, u32 e) {
    Fr acc = Fr::one();
    for (u32 j = 0; e; j++, e >>= 1)
        if (e & 1) acc = Fr::mul(acc, fr_load(&sq[j]));
    return acc;
}

// (a) u[i] = k w^i / (t - w^i), i < n (k = zt / m).  pref: n Fr of scratch (the lane's prefix products).  t is outside
// the domain (checked on the host), so no factor is zero.
template <class Fr>
__global__ void __launch_bounds__(64)
k_kg_lagrange(const Fr* __restrict__ kc, u32 n, Fr* __restrict__ u, Fr* __restrict__ pref) {
    u32 lane = blockIdx.x * blockDim.x + threadIdx.x;
    if ((u64)lane * KG_CHUNK >= n) return;
    u32 lo = lane * KG_CHUNK, hi = min(lo + KG_CHUNK, n);
    const Fr t = fr_load(&kc[KC_T]), w = fr_load(&kc[KC_WSQ]);
    Fr wi = kg_pow(kc + KC_WSQ, lo);
    Fr acc = Fr::one();
    for (u32 i = lo; i < hi; i++) {
        fr_store(&u[i], wi);
        fr_store(&pref[i], acc);
        acc = Fr::mul(acc, Fr::sub(t, wi));
        wi = Fr::mul(wi, w);
    }
    Fr inv = fp_inv(acc);
    const Fr k = fr_load(&kc[KC_K]);
    for (u32 i = hi; i-- > lo;) {
        Fr x = fr_load(&u[i]);
        Fr d_inv = Fr::mul(inv, fr_load(&pref[i]));
        inv = Fr::mul(inv, Fr::sub(t, x));
        fr_store(&u[i], Fr::mul(Fr::mul(k, x), d_inv));
    }
}

// (b) cnt[col[e]] += 1 for every entry
template <int UNUSED>
__global__ void __launch_bounds__(256) k_kg_col_count(const u32* __restrict__ col, u32 nnz, u32* __restrict__ cnt) {
    u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nnz) atomicAdd(&cnt[col[e]], 1u);
}

// sorted[cursor[col]++] = val * u[row] for every entry; the row of entry e is found by bisection over row_ptr (validated:
// non-decreasing, row_ptr[0] = 0, row_ptr[n_rows] = nnz), so a long row does not serialise on one lane
template <class Fr>
__global__ void __launch_bounds__(256)
k_kg_scatter(const u64* __restrict__ row_ptr, u32 n_rows, const u32* __restrict__ col, const Fr* __restrict__ val, u32 nnz,
             const Fr* __restrict__ u, u32* __restrict__ cursor, Fr* __restrict__ sorted) {
    u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    u32 lo = 0, hi = n_rows;                   // row_ptr[lo] <= e < row_ptr[hi]
    while (hi - lo > 1) {
        u32 mid = lo + (hi - lo) / 2;
        if (row_ptr[mid] <= e) lo = mid; else hi = mid;
    }
    u32 slot = atomicAdd(&cursor[col[e]], 1u);
    fr_store(&sorted[slot], Fr::mul(fr_load(&val[e]), fr_load(&u[lo])));
}

// cnt[j] = number of KG_SEG-entry chunks of column j (cnt[n_cols] = 0: the scan's total lands there)
template <int UNUSED>
__global__ void __launch_bounds__(256) k_kg_chunk_count(const u32* __restrict__ start, u32 n_cols, u32* __restrict__ cnt) {
    u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_cols) cnt[j] = (start[j + 1] - start[j] + KG_SEG - 1) / KG_SEG;
    else if (j == n_cols) cnt[j] = 0;
}

// out[c] = sum of chunk c (at most KG_SEG entries of one column); chunk c belongs to the last column j with cstart[j] <= c
template <class Fr>
__global__ void __launch_bounds__(256)
k_kg_chunk_sum(const u32* __restrict__ start, const u32* __restrict__ cstart, u32 n_cols, const Fr* __restrict__ vals,
               Fr* __restrict__ out) {
    u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cstart[n_cols]) return;
    u32 lo = 0, hi = n_cols;                   // cstart[lo] <= c < cstart[hi]
    while (hi - lo > 1) {
        u32 mid = lo + (hi - lo) / 2;
        if (cstart[mid] <= c) lo = mid; else hi = mid;
    }
    u32 k0 = start[lo] + (c - cstart[lo]) * KG_SEG, k1 = min(k0 + KG_SEG, start[lo + 1]);
    Fr acc = Fr::zero();
    for (u32 k = k0; k < k1; k++) acc = Fr::add(acc, fr_load(&vals[k]));
    fr_store(&out[c], acc);
}

// out[j] = sum of column j (at most KG_SEG entries by now) + u[n_c + j] for j < n_copy (A's instance rows)
template <class Fr>
__global__ void __launch_bounds__(256)
k_kg_col_final(const u32* __restrict__ start, u32 n_cols, const Fr* __restrict__ vals, const Fr* __restrict__ u, u32 n_c,
               u32 n_copy, Fr* __restrict__ out) {
    u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_cols) return;
    Fr acc = j < n_copy ? fr_load(&u[n_c + j]) : Fr::zero();
    for (u32 k = start[j]; k < start[j + 1]; k++) acc = Fr::add(acc, fr_load(&vals[k]));
    fr_store(&out[j], acc);
}

template <class Fr>
__device__ __forceinline__ void kg_store_canon(Fr* p, const Fr& x) { fr_store(p, Fr::from_mont(x)); }

// (c) one lane per variable: a g1s, b g1s, b g2s, and (beta a + alpha b + c) times gamma^-1 g1s (instance variables) or
// delta_k^-1 g1s (witness variable w of stage k: the last stage with begin <= w).  abc: a | b | c, n_v each.  Canonical.
template <class Fr>
__global__ void __launch_bounds__(64)
k_kg_scalars(const Fr* __restrict__ abc, const Fr* __restrict__ kc, const Fr* __restrict__ dinv_g1s,
             const u32* __restrict__ stage_begin, u32 n_stages, u32 n_inst, u32 n_v, Fr* __restrict__ sa, Fr* __restrict__ sb1,
             Fr* __restrict__ sb2, Fr* __restrict__ sgabc, Fr* __restrict__ sck) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_v) return;
    const Fr a = fr_load(&abc[i]), b = fr_load(&abc[(size_t)n_v + i]), c = fr_load(&abc[2 * (size_t)n_v + i]);
    const Fr g1s = fr_load(&kc[KC_G1S]);
    kg_store_canon(&sa[i], Fr::mul(a, g1s));
    kg_store_canon(&sb1[i], Fr::mul(b, g1s));
    kg_store_canon(&sb2[i], Fr::mul(b, fr_load(&kc[KC_G2S])));
    Fr s = Fr::add(Fr::add(Fr::mul(fr_load(&kc[KC_BETA]), a), Fr::mul(fr_load(&kc[KC_ALPHA]), b)), c);
    if (i < n_inst) {
        kg_store_canon(&sgabc[i], Fr::mul(s, fr_load(&kc[KC_GAMMA_INV_G1S])));
        return;
    }
    u32 w = i - n_inst, lo = 0, hi = n_stages;  // stage_begin[lo] <= w (stage_begin[0] = 0)
    while (hi - lo > 1) {
        u32 mid = lo + (hi - lo) / 2;
        if (stage_begin[mid] <= w) lo = mid; else hi = mid;
    }
    kg_store_canon(&sck[w], Fr::mul(s, fr_load(&dinv_g1s[lo])));
}

// (c) h query: out[i] = h0 t^i (h0 = zt delta_last^-1 g1s), i < n, KG_CHUNK powers per lane from t^(first).  Canonical.
template <class Fr>
__global__ void __launch_bounds__(64) k_kg_hquery(const Fr* __restrict__ kc, u32 n, Fr* __restrict__ out) {
    u32 lane = blockIdx.x * blockDim.x + threadIdx.x;
    if ((u64)lane * KG_CHUNK >= n) return;
    u32 lo = lane * KG_CHUNK, hi = min(lo + KG_CHUNK, n);
    const Fr t = fr_load(&kc[KC_T]);
    Fr x = Fr::mul(fr_load(&kc[KC_H0]), kg_pow(kc + KC_TSQ, lo));
    for (u32 i = lo; i < hi; i++) {
        kg_store_canon(&out[i], x);
        x = Fr::mul(x, t);
    }
}

#endif  // __HIPCC__

// ---- host side --------------------------------------------------------------------------------------------------

// the standard generators (canonical coordinates, little-endian u32 limbs): the bases of every sweep, so the context's
// window-table cache of hk_fixed_base serves these calls and the bindings' own setup alike
template <class C> struct KgGenerators;
template <> struct KgGenerators<CurveBn254> {
    static constexpr u32 G1[2][8] = {{1, 0, 0, 0, 0, 0, 0, 0}, {2, 0, 0, 0, 0, 0, 0, 0}};
    static constexpr u32 G2[4][8] = {
        {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu},
        {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u},
        {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u},
        {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u}};
};
template <> struct KgGenerators<CurveBls381> {
    static constexpr u32 G1[2][12] = {
        {0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu, 0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu,
         0x2695638cu, 0x3197d794u, 0x17f1d3a7u},
        {0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu, 0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u,
         0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u}};
    static constexpr u32 G2[4][12] = {
        {0xc121bdb8u, 0xd48056c8u, 0xa805bbefu, 0x0bac0326u, 0x7ae3d177u, 0xb4510b64u, 0xfa403b02u, 0xc6e47ad4u, 0x2dc51051u,
         0x26080527u, 0xf08f0a91u, 0x024aa2b2u},
        {0x5d042b7eu, 0xe5ac7d05u, 0x13945d57u, 0x334cf112u, 0xdc7f5049u, 0xb5da61bbu, 0x9920b61au, 0x596bd0d0u, 0x88274f65u,
         0x7dacd3a0u, 0x52719f60u, 0x13e02b60u},
        {0x08b82801u, 0xe1935486u, 0x3baca289u, 0x923ac9ccu, 0x5160d12cu, 0x6d429a69u, 0x8cbdd3a7u, 0xadfd9baau, 0xda2e351au,
         0x8cc9cdc6u, 0x727d6e11u, 0x0ce5d527u},
        {0xf05f79beu, 0xaaa9075fu, 0x5cec1da1u, 0x3f370d27u, 0x572e99abu, 0x267492abu, 0x85a763afu, 0xcb3e287eu, 0x2bc28b99u,
         0x32acd2b0u, 0x2ea734ccu, 0x0606c4a0u}};
};

template <class C>
struct KgHost {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;

    static Fr load(const void* p) {
        Fr x;
        memcpy(x.v, p, sizeof(Fr));
        return Fr::canon(x);
    }
    static Fq mont_q(const u32* limbs) {
        Fq x;
        for (int i = 0; i < Fq::N; i++) x.v[i] = limbs[i];
        return Fq::canon(Fq::to_mont(x));
    }
    static Affine<Fq> g1() {
        Affine<Fq> p;
        p.x = mont_q(KgGenerators<C>::G1[0]);
        p.y = mont_q(KgGenerators<C>::G1[1]);
        return p;
    }
    static Affine<Fq2> g2() {
        Affine<Fq2> p;
        p.x.c0 = mont_q(KgGenerators<C>::G2[0]);
        p.x.c1 = mont_q(KgGenerators<C>::G2[1]);
        p.y.c0 = mont_q(KgGenerators<C>::G2[2]);
        p.y.c1 = mont_q(KgGenerators<C>::G2[3]);
        return p;
    }

    // the checks both entry points make on the host, in the documented order (1: the domain from the sizes alone; 2: NULL
    // pointers, row counts, 32-bit sizes)
    static hk_status check_sizes(const hk_csr* const Ms[3], size_t n_inst, size_t n_c, size_t n_v, u32* log_m) {
        *log_m = QapHost<C>::domain_log(n_c, n_inst);
        if (*log_m > C::TWO_ADICITY) return HK_ERR_DOMAIN_TOO_LARGE;
        const u64 lim = (u64)1 << 32;
        if ((u64)1 << *log_m >= lim || n_v >= lim || n_inst < 1 || n_inst > n_v) return HK_ERR_ARG;
        for (int k = 0; k < 3; k++) {
            const hk_csr* M = Ms[k];
            if (!csr_host_ok(M) || M->n_rows != n_c || M->nnz >= lim) return HK_ERR_ARG;
        }
        return HK_OK;
    }

    // the Fr constants of a call (KC_*), Montgomery; false when t lies in the domain (zt = 0)
    static bool constants(u32 log_m, const Fr& t, Fr* kc, Fr* zt_out) {
        Fr tm = t;
        for (u32 k = 0; k < log_m; k++) tm = Fr::sqr(tm);
        Fr zt = Fr::canon(Fr::sub(tm, Fr::one()));
        *zt_out = zt;
        if (zt.is_zero()) return false;
        Fr w = host_from_limbs<Fr>(C::ROOT);
        for (u32 k = 0; k < C::TWO_ADICITY - log_m; k++) w = Fr::sqr(w);
        Fr tp = t;
        for (int j = 0; j < 32; j++) {
            kc[KC_WSQ + j] = Fr::canon(w);
            kc[KC_TSQ + j] = Fr::canon(tp);
            w = Fr::sqr(w);
            tp = Fr::sqr(tp);
        }
        kc[KC_T] = t;
        kc[KC_K] = Fr::canon(Fr::mul(zt, NttHost<C>::size_inv(log_m)));
        return true;
    }
};

// Phases (a) and (b) on a lane: a | b | c at t into `abc` (3 n_v Fr, Montgomery).  carve() lists the phase's scratch
// (matrix copies of host inputs, u, the column-order buffers); run() validates the matrices first (HK_ERR_ARG for a column
// >= n_v or a malformed row_ptr, before anything reads them) and returns HK_ERR_ARG when zt = 0.
template <class C>
struct KgQap {
    typedef typename C::Fr Fr;
    const hk_csr* Ms[3];
    size_t n_inst, n_c, n_v, nnz_max = 0, n_y = 0;
    u32 log_m;
    R1csStage stage;
    u32 *cnt, *st[2], *cursor, *tops;
    Fr *u, *pref, *X, *Y;

    void init() {                                // after KgHost::check_sizes
        stage = R1csStage(Ms[0], Ms[1], Ms[2], n_v, sizeof(Fr));
        for (int k = 0; k < 3; k++) nnz_max = std::max(nnz_max, Ms[k]->nnz);
        n_y = std::min(nnz_max, nnz_max / KG_SEG + n_v);
    }
    void carve(Carve& c) {
        stage.carve(c);
        u = c.n<Fr>(n_c + n_inst);
        pref = c.n<Fr>(n_c + n_inst);
        cnt = c.n<u32>(n_v + 1);
        st[0] = c.n<u32>(n_v + 1);
        st[1] = c.n<u32>(n_v + 1);
        cursor = c.n<u32>(n_v + 1);
        tops = c.n<u32>(scan_u32_tops_len(n_v + 1));
        X = c.n<Fr>(nnz_max);
        Y = c.n<Fr>(n_y);
    }
    // kc_d: the call's constants on the device (KC_*)
    hk_status run(Lane* L, const Fr* kc_d, bool zt_zero, Fr* abc) {
        hipStream_t s = L->stream;
        CsrDev D[3];
        HK_TRY(stage.upload(L, D));
        if (zt_zero) return HK_ERR_ARG;                                  // t in the domain (generator.rs:68 never draws one)
        const u32 nu = (u32)(n_c + n_inst), nv = (u32)n_v;
        HK_LAUNCH((k_kg_lagrange<Fr>), dim3((nu / KG_CHUNK + 1 + 63) / 64), dim3(64), 0, s, kc_d, nu, u, pref);
        for (int k = 0; k < 3; k++) {
            const u32 nnz = (u32)D[k].nnz;
            HK_HIP(hipMemsetAsync(cnt, 0, sizeof(u32) * (n_v + 1), s));
            if (nnz) HK_LAUNCH((k_kg_col_count<0>), dim3((nnz + 255) / 256), dim3(256), 0, s, D[k].col, nnz, cnt);
            HK_TRY(scan_u32(s, cnt, st[0], tops, nv + 1));
            HK_HIP(hipMemcpyAsync(cursor, st[0], sizeof(u32) * (n_v + 1), hipMemcpyDeviceToDevice, s));
            if (nnz)
                HK_LAUNCH((k_kg_scatter<Fr>), dim3((nnz + 255) / 256), dim3(256), 0, s, D[k].row_ptr, (u32)n_c, D[k].col,
                          (const Fr*)D[k].val, nnz, (const Fr*)u, cursor, X);
            // bounded chunk levels: after each, no column holds more than ceil(bound / KG_SEG) entries
            const u32* start = st[0];
            const Fr* vals = X;
            u64 bound = nnz, entries = nnz;
            for (int lvl = 0; bound > KG_SEG; lvl++) {
                u32* next_start = st[(lvl + 1) & 1];
                Fr* next = (lvl & 1) ? X : Y;
                HK_LAUNCH((k_kg_chunk_count<0>), dim3((nv + 1 + 255) / 256), dim3(256), 0, s, start, nv, cnt);
                HK_TRY(scan_u32(s, cnt, next_start, tops, nv + 1));
                entries = std::min<u64>(entries, entries / KG_SEG + n_v);     // chunks <= entries / KG_SEG + non-empty columns
                HK_LAUNCH((k_kg_chunk_sum<Fr>), dim3((u32)((entries + 255) / 256)), dim3(256), 0, s, start,
                          (const u32*)next_start, nv, vals, next);
                start = next_start;
                vals = next;
                bound = (bound + KG_SEG - 1) / KG_SEG;
            }
            HK_LAUNCH((k_kg_col_final<Fr>), dim3((nv + 255) / 256), dim3(256), 0, s, start, nv, vals, (const Fr*)u,
                      (u32)n_c, k == 0 ? (u32)n_inst : 0u, abc + k * n_v);
        }
        return HK_OK;
    }
};

template <class C>
hk_status Ops<C>::qap_eval(hk_ctx* ctx, const hk_csr* A, const hk_csr* B, const hk_csr* Cm, size_t n_inst, size_t n_c,
                           size_t n_v, const void* t_mont, void* a_out, void* b_out, void* c_out, void* zt_out, size_t* m_out) {
    typedef KgHost<C> H;
    KgQap<C> q{{A, B, Cm}, n_inst, n_c, n_v};
    HK_TRY(H::check_sizes(q.Ms, n_inst, n_c, n_v, &q.log_m));
    if (!t_mont || !a_out || !b_out || !c_out || !zt_out) return HK_ERR_ARG;
    if (m_out) *m_out = (size_t)1 << q.log_m;
    std::vector<Fr> kc(KC_N, Fr::zero());                  // outlives the lane's copies of it
    Fr zt;
    const bool zt_zero = !H::constants(q.log_m, H::load(t_mont), kc.data(), &zt);
    q.init();
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    Fr *kc_d, *abc;
    HK_TRY(L->carve([&](Carve& c) {
        kc_d = c.n<Fr>(KC_N);
        abc = c.n<Fr>(3 * n_v);
        q.carve(c);
    }));
    HK_HIP(hipMemcpyAsync(kc_d, kc.data(), sizeof(Fr) * KC_N, hipMemcpyHostToDevice, L->stream));
    HK_TRY(q.run(L, kc_d, zt_zero, abc));
    void* outs[3] = {a_out, b_out, c_out};
    for (int k = 0; k < 3; k++)
        HK_HIP(hipMemcpyAsync(outs[k], abc + k * n_v, n_v * sizeof(Fr),
                              is_device_ptr(outs[k]) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, L->stream));
    HK_TRY(L->settle());
    memcpy(zt_out, &zt, sizeof(Fr));
    return HK_OK;
}

template <class C>
hk_status Ops<C>::keygen(hk_ctx* ctx, const hk_keygen_desc* d, const hk_keygen_out* o, size_t* m_out) {
    typedef KgHost<C> H;
    const size_t n_inst = d->n_inst, n_c = d->n_constraints, n_v = d->n_v, n_st = d->n_stages;
    KgQap<C> q{{d->A, d->B, d->C}, n_inst, n_c, n_v};
    HK_TRY(H::check_sizes(q.Ms, n_inst, n_c, n_v, &q.log_m));
    const size_t m = (size_t)1 << q.log_m;
    const void* required[] = {d->alpha, d->beta, d->gamma, d->t, d->g1_scalar, d->g2_scalar, o->a_g, o->b_g, o->b_h, o->alpha_g,
                              o->beta_g, o->beta_h, o->gamma_h};
    for (const void* p : required)
        if (!p) return HK_ERR_ARG;
    if (n_st < 1 || !d->stage_ranges || !d->deltas || !o->ck_stage || !o->deltas_g || !o->deltas_h || !o->gamma_abc_g ||
        (m > 1 && !o->h_g))
        return HK_ERR_ARG;
    // the stage ranges tile [0, n_v - n_inst) in order (variable_range_for_stage)
    std::vector<u32> begin(n_st);
    u64 at = 0;
    for (size_t k = 0; k < n_st; k++) {
        u64 b = d->stage_ranges[2 * k], e = d->stage_ranges[2 * k + 1];
        if (b != at || e < b) return HK_ERR_ARG;
        if (e > b && !o->ck_stage[k]) return HK_ERR_ARG;
        begin[k] = (u32)b;
        at = e;
    }
    if (at != n_v - n_inst) return HK_ERR_ARG;
    const Fr alpha = H::load(d->alpha), beta = H::load(d->beta), gamma = H::load(d->gamma), g1s = H::load(d->g1_scalar),
             g2s = H::load(d->g2_scalar);
    std::vector<Fr> deltas(n_st);
    for (size_t k = 0; k < n_st; k++) deltas[k] = H::load((const char*)d->deltas + k * sizeof(Fr));
    if (gamma.is_zero()) return HK_ERR_ARG;
    for (const Fr& x : deltas)
        if (x.is_zero()) return HK_ERR_ARG;
    if (m_out) *m_out = m;

    // host constants: kc (KC_* then delta_k^-1 g1s per stage), the small sets [alpha, beta, delta_k] g1s and
    // [beta, gamma, delta_k] g2s (Montgomery); all of it outlives the lane's copies
    std::vector<Fr> kc(KC_N + n_st, Fr::zero()), s1(2 + n_st), s2(2 + n_st);
    Fr zt;
    const bool zt_zero = !H::constants(q.log_m, H::load(d->t), kc.data(), &zt);
    kc[KC_ALPHA] = alpha;
    kc[KC_BETA] = beta;
    kc[KC_G1S] = g1s;
    kc[KC_G2S] = g2s;
    kc[KC_GAMMA_INV_G1S] = Fr::canon(Fr::mul(fp_inv(gamma), g1s));
    kc[KC_H0] = Fr::canon(Fr::mul(Fr::mul(zt, fp_inv(deltas[n_st - 1])), g1s));
    for (size_t k = 0; k < n_st; k++) kc[KC_N + k] = Fr::canon(Fr::mul(fp_inv(deltas[k]), g1s));
    s1[0] = Fr::canon(Fr::mul(alpha, g1s));
    s1[1] = Fr::canon(Fr::mul(beta, g1s));
    s2[0] = Fr::canon(Fr::mul(beta, g2s));
    s2[1] = Fr::canon(Fr::mul(gamma, g2s));
    for (size_t k = 0; k < n_st; k++) {
        s1[2 + k] = Fr::canon(Fr::mul(deltas[k], g1s));
        s2[2 + k] = Fr::canon(Fr::mul(deltas[k], g2s));
    }
    const Affine<Fq> G1 = H::g1();
    const Affine<Fq2> G2 = H::g2();
    q.init();
    const size_t n_w = n_v - n_inst, n_h = m - 1;
    const size_t n_sweep = std::max<size_t>(std::max(n_v, n_h), n_st + 2);
    // the window tables of the two generators (fixed_base: the context's cache, else the call's scratch)
    FbCacheUse t1(ctx, 1, &G1, sizeof(G1), sizeof(Affine<Fq>) * FB_WINDOWS * 256);
    FbCacheUse t2(ctx, 2, &G2, sizeof(G2), sizeof(Affine<Fq2>) * FB_WINDOWS * 256);
    // where each output lives, decided before the carve
    struct Out { void* p; bool dev; };
    auto out = [](void* p) { return Out{p, is_device_ptr(p)}; };
    std::vector<Out> ck(n_st);
    for (size_t k = 0; k < n_st; k++) ck[k] = out(o->ck_stage[k]);
    const Out a_g = out(o->a_g), b_g = out(o->b_g), b_h = out(o->b_h), h_g = out(o->h_g), deltas_g = out(o->deltas_g),
              alpha_g = out(o->alpha_g), beta_g = out(o->beta_g), gamma_abc_g = out(o->gamma_abc_g), beta_h = out(o->beta_h),
              gamma_h = out(o->gamma_h), deltas_h = out(o->deltas_h), qap_abc = out(o->qap_abc);

    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    hipStream_t s = L->stream;
    const bool prof = ctx->profiling != 0;
    Fr *kc_d, *abc, *sa, *sb1, *sb2, *sgabc, *sck, *sh, *s1_d, *s2_d;
    u32* begin_d;
    Affine<Fq>*g1_d, *tab1;
    Affine<Fq2>*g2_d, *tab2;
    void *xy, *pref, *out_s;
    HK_TRY(L->carve([&](Carve& c) {
        kc_d = c.n<Fr>(KC_N + n_st);
        begin_d = c.n<u32>(n_st);
        s1_d = c.n<Fr>(2 + n_st);
        s2_d = c.n<Fr>(2 + n_st);
        g1_d = c.n<Affine<Fq>>(1);
        g2_d = c.n<Affine<Fq2>>(1);
        tab1 = c.n<Affine<Fq>>(FB_WINDOWS * 256);
        tab2 = c.n<Affine<Fq2>>(FB_WINDOWS * 256);
        abc = c.n<Fr>(3 * n_v);
        sa = c.n<Fr>(n_v);
        sb1 = c.n<Fr>(n_v);
        sb2 = c.n<Fr>(n_v);
        sgabc = c.n<Fr>(n_inst);
        sck = c.n<Fr>(n_w);
        sh = c.n<Fr>(n_h);
        // the QAP phase's buffers and the sweeps' share the rest of the arena: the sweeps start after the QAP phase ends
        const size_t mark = c.off;
        q.carve(c);
        const size_t qap_end = c.off;
        c.off = mark;
        xy = c.take(n_sweep * sizeof(XYZZ<Fq2>));
        pref = c.take(n_sweep * sizeof(Fq2));
        out_s = c.take(n_sweep * sizeof(Affine<Fq2>));
        c.off = std::max(c.off, qap_end);
    }));
    hipEvent_t* ev = L->ev;
    if (prof) HK_HIP(hipEventRecord(ev[0], s));
    HK_HIP(hipMemcpyAsync(kc_d, kc.data(), sizeof(Fr) * kc.size(), hipMemcpyHostToDevice, s));
    HK_HIP(hipMemcpyAsync(begin_d, begin.data(), sizeof(u32) * n_st, hipMemcpyHostToDevice, s));
    HK_HIP(hipMemcpyAsync(s1_d, s1.data(), sizeof(Fr) * s1.size(), hipMemcpyHostToDevice, s));
    HK_HIP(hipMemcpyAsync(s2_d, s2.data(), sizeof(Fr) * s2.size(), hipMemcpyHostToDevice, s));
    HK_HIP(hipMemcpyAsync(g1_d, &G1, sizeof(G1), hipMemcpyHostToDevice, s));
    HK_HIP(hipMemcpyAsync(g2_d, &G2, sizeof(G2), hipMemcpyHostToDevice, s));
    // (a) + (b); every check of the matrices and of t happens here, before any sweep writes an output
    HK_TRY(q.run(L, kc_d, zt_zero, abc));
    if (prof) HK_HIP(hipEventRecord(ev[1], s));
    // (c)
    HK_LAUNCH((k_kg_scalars<Fr>), dim3((u32)((n_v + 63) / 64)), dim3(64), 0, s, (const Fr*)abc, (const Fr*)kc_d,
              (const Fr*)(kc_d + KC_N), (const u32*)begin_d, (u32)n_st, (u32)n_inst, (u32)n_v, sa, sb1, sb2, sgabc, sck);
    if (n_h)
        HK_LAUNCH((k_kg_hquery<Fr>), dim3((u32)((n_h / KG_CHUNK + 1 + 63) / 64)), dim3(64), 0, s, (const Fr*)kc_d,
                  (u32)n_h, sh);
    if (qap_abc.p)
        HK_HIP(hipMemcpyAsync(qap_abc.p, abc, 3 * n_v * sizeof(Fr), qap_abc.dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                              s));
    if (prof) HK_HIP(hipEventRecord(ev[2], s));
    // (d) one sweep per output
    Affine<Fq>* table1 = t1.table ? (Affine<Fq>*)t1.table : tab1;
    Affine<Fq2>* table2 = t2.table ? (Affine<Fq2>*)t2.table : tab2;
    bool build1 = t1.build, build2 = t2.build;
    auto sweep = [&](auto ftag, const Fr* sc, int mont, size_t n, const Out& dst) -> hk_status {
        typedef decltype(ftag) F;
        if (n == 0) return HK_OK;
        constexpr bool g1 = sizeof(F) == sizeof(Fq);
        Affine<F>* od = dst.dev ? (Affine<F>*)dst.p : (Affine<F>*)out_s;
        bool& build = g1 ? build1 : build2;
        HK_TRY(MsmRun<F>::fixed_base(s, g1 ? (const Affine<F>*)g1_d : (const Affine<F>*)g2_d, sc, mont, (u32)n,
                                     g1 ? (Affine<F>*)table1 : (Affine<F>*)table2, (XYZZ<F>*)xy, (F*)pref, od, build));
        build = false;
        if (!dst.dev) HK_HIP(hipMemcpyAsync(dst.p, od, n * sizeof(Affine<F>), hipMemcpyDeviceToHost, s));
        return HK_OK;
    };
    HK_TRY(sweep(Fq(), s1_d, 1, 1, alpha_g));
    HK_TRY(sweep(Fq(), s1_d + 1, 1, 1, beta_g));
    HK_TRY(sweep(Fq(), s1_d + 2, 1, n_st, deltas_g));
    HK_TRY(sweep(Fq(), sgabc, 0, n_inst, gamma_abc_g));
    HK_TRY(sweep(Fq(), sa, 0, n_v, a_g));
    HK_TRY(sweep(Fq(), sb1, 0, n_v, b_g));
    HK_TRY(sweep(Fq(), sh, 0, n_h, h_g));
    for (size_t k = 0; k < n_st; k++)
        HK_TRY(sweep(Fq(), sck + begin[k], 0, (size_t)(d->stage_ranges[2 * k + 1] - d->stage_ranges[2 * k]), ck[k]));
    HK_TRY(sweep(Fq2(), s2_d, 1, 1, beta_h));
    HK_TRY(sweep(Fq2(), s2_d + 1, 1, 1, gamma_h));
    HK_TRY(sweep(Fq2(), s2_d + 2, 1, n_st, deltas_h));
    HK_TRY(sweep(Fq2(), sb2, 0, n_v, b_h));
    if (prof) HK_HIP(hipEventRecord(ev[3], s));
    HK_TRY(L->settle());
    t1.publish();
    t2.publish();
    if (prof) {
        hk_timings& tm = L->timings;
        memset(&tm, 0, sizeof(tm));
        HK_HIP(hipEventElapsedTime(&tm.total_ms, ev[0], ev[3]));
        HK_HIP(hipEventElapsedTime(&tm.keygen_qap_ms, ev[0], ev[1]));
        HK_HIP(hipEventElapsedTime(&tm.keygen_scalars_ms, ev[1], ev[2]));
        HK_HIP(hipEventElapsedTime(&tm.keygen_sweeps_ms, ev[2], ev[3]));
    }
    return HK_OK;
}

}  // namespace hk
