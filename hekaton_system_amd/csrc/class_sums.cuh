// class_sums.cuh — the aggregate verifier's class sums on the device (hk_class_power_sums):
// sums[c] = sum of x^i over the i < n with class_of[i] == c, the exponents of prod_c e(alpha_c, beta_c)^(sums[c]), which is
// how a verifier forms prod_i e(alpha_i, beta_i)^(x^i) (aggregation.rs:265-273) from one pairing per key class.
//
//   chunks   one lane per chunk of AQ_CHUNK consecutive exponents, as hk_scalar_powers: x^(8 t) from the bits of t over the
//            host's table, then seven products by x.  Each power is added to one of CS_GROUP per-lane accumulators - eight
//            additions of the power or of zero (aq_select), never an accumulator indexed by the class: that one would live
//            in scratch.  Classes beyond eight are further passes on grid.y (class group g = classes 8 g .. 8 g + 7).  A
//            workgroup takes CS_WG chunks at a time and strides on by the grid (at most CS_MAX_WGS workgroups a class group),
//            then sums each accumulator over its lanes in LDS and writes its eight partials.  A class id >= n_classes sets
//            the call's error word.
//   reduce   one workgroup per class sums the class's partials over the workgroups of the first launch.
//
// No atomics on Fr (they would not be 256 bits wide), and none are needed: the sums are exact in the field, so every order of
// additions gives the same canonical bytes.  The chunk-level body is an HK_HD function of (table, class_of, n, chunk index,
// class group), so a host program runs it chunk by chunk with a serial reduction (tests/host_shim/class_sums_shim.cpp); only
// the LDS sums are device-only.
#pragma once
#include <stddef.h>
#include "agg_scalars.cuh"

namespace hk {

constexpr u32 CS_GROUP = 8;            // classes per pass: accumulators per lane
constexpr u32 CS_WG = 256;             // lanes per workgroup, one chunk each per stride
constexpr u32 CS_MAX_WGS = 1024;       // workgroups per class group: bounds the partials at any n
constexpr u32 CS_MAX_CLASSES = 1024;

template <class Fr>
struct CsAcc {
    Fr a[CS_GROUP];
};
template <class Fr>
HK_HD void cs_acc_zero(CsAcc<Fr>& acc) {
    HK_UNROLL for (u32 k = 0; k < CS_GROUP; k++) acc.a[k] = Fr::zero();
}

// acc.a[k] += x^i for the exponents i of chunk t below n whose class is 8 group + k; nbits: the bit length of the last chunk's
// index.  False when one of the chunk's class ids is >= n_classes.
template <class Fr>
HK_HD bool cs_chunk(const Fr* tab, const u32* class_of, u64 n, u32 n_classes, u32 t, u32 nbits, u32 group, CsAcc<Fr>& acc) {
    Fr pw = aq_bits_product<Fr>(tab + AQ_PW_SQ, t, nbits);
    const Fr x = aq_ld(&tab[AQ_PW_X]);
    bool ok = true;
    HK_NOUNROLL for (u32 j = 0; j < AQ_CHUNK; j++) {
        const u64 i = (u64)t * AQ_CHUNK + j;
        const bool in = i < n;
        const u32 c = in ? class_of[i] : 0u;
        ok = ok && c < n_classes;
        const u32 rel = c - group * CS_GROUP;                       // wraps for a class below the group: matches no k
        HK_UNROLL for (u32 k = 0; k < CS_GROUP; k++)
            acc.a[k] = Fr::add(acc.a[k], aq_select<Fr>(in && rel == k, pw, Fr::zero()));
        if (j + 1 < AQ_CHUNK) pw = Fr::mul(pw, x);
    }
    return ok;
}

// the workgroups of the first launch along x, and where workgroup b of class group g writes its CS_GROUP partials
static inline u32 cs_workgroups(u32 n_chunks) {
    const u32 w = (n_chunks + CS_WG - 1) / CS_WG;
    return w < CS_MAX_WGS ? w : CS_MAX_WGS;
}
HK_HD size_t cs_part_at(u32 group, u32 n_wgs, u32 b) { return ((size_t)group * n_wgs + b) * CS_GROUP; }

}  // namespace hk

#if defined(__HIPCC__)

namespace hk {

// the sum of v over the W lanes of a workgroup (W a power of two), on every lane; s: W Fr of LDS.  The first barrier lets a
// caller use s again right after an earlier sum.  Every lane meets every barrier.
template <class Fr, u32 W>
__device__ __forceinline__ Fr cs_wg_sum(Fr* s, u32 tid, const Fr& v) {
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    HK_NOUNROLL for (u32 off = W / 2; off; off >>= 1) {
        if (tid < off) s[tid] = Fr::add(s[tid], s[tid + off]);
        __syncthreads();
    }
    return s[0];
}

// grid (n_wgs, class groups).  part: class groups x n_wgs x CS_GROUP Fr.
template <class Fr>
__global__ void __launch_bounds__(CS_WG)
k_cs_chunks(const Fr* __restrict__ tab, const u32* __restrict__ class_of, u64 n, u32 n_classes, u32 n_chunks, u32 nbits,
            Fr* __restrict__ part, u32* __restrict__ flag) {
    __shared__ Fr s[CS_WG];
    const u32 tid = threadIdx.x, g = blockIdx.y;
    CsAcc<Fr> acc;
    cs_acc_zero<Fr>(acc);
    bool ok = true;
    HK_NOUNROLL for (u32 t = blockIdx.x * CS_WG + tid; t < n_chunks; t += gridDim.x * CS_WG)
        ok = cs_chunk<Fr>(tab, class_of, n, n_classes, t, nbits, g, acc) && ok;
    if (!ok) atomicOr(flag, 1u);
    Fr* out = part + cs_part_at(g, gridDim.x, blockIdx.x);
    HK_UNROLL for (u32 k = 0; k < CS_GROUP; k++) {
        const Fr v = cs_wg_sum<Fr, CS_WG>(s, tid, acc.a[k]);
        if (tid == 0) fr_store(&out[k], v);
    }
}

// one workgroup per class
template <class Fr>
__global__ void __launch_bounds__(CS_WG) k_cs_reduce(const Fr* __restrict__ part, u32 n_wgs, Fr* __restrict__ sums) {
    __shared__ Fr s[CS_WG];
    const u32 tid = threadIdx.x, c = blockIdx.x;
    Fr acc = Fr::zero();
    HK_NOUNROLL for (u32 b = tid; b < n_wgs; b += CS_WG) acc = Fr::add(acc, fr_load(&part[cs_part_at(c / CS_GROUP, n_wgs, b) + c % CS_GROUP]));
    acc = cs_wg_sum<Fr, CS_WG>(s, tid, acc);
    if (tid == 0) fr_store(&sums[c], acc);
}

template <class C>
hk_status Ops<C>::class_power_sums(hk_ctx* ctx, const void* x_mont, const uint32_t* class_of, size_t n, size_t n_classes,
                                   void* sums_out) {
    if (!x_mont || !class_of || !sums_out) return HK_ERR_ARG;
    if (n > ((size_t)1 << AQ_MAX_LOG) || n_classes == 0 || n_classes > CS_MAX_CLASSES) return HK_ERR_ARG;
    Fr x, tab[AQ_PW_LEN];
    memcpy(&x, x_mont, sizeof(Fr));
    aq_powers_table<Fr>(x, tab);
    const u32 n_chunks = (u32)((n + AQ_CHUNK - 1) / AQ_CHUNK), n_wgs = cs_workgroups(n_chunks);
    const u32 n_groups = (u32)((n_classes + CS_GROUP - 1) / CS_GROUP);
    u32 nbits = 0;
    while (((u64)1 << nbits) < n_chunks) nbits++;
    Staged in = staged(class_of, n * sizeof(u32)), to = staged(sums_out, n_classes * sizeof(Fr));
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    Fr *tab_d, *part;
    u32* flag;
    HK_TRY(L->carve([&](Carve& c) {
        tab_d = c.n<Fr>(AQ_PW_LEN);
        part = c.n<Fr>((size_t)n_groups * n_wgs * CS_GROUP);
        flag = c.n<u32>(1);
        stage_carve(c, &in, 1);
        stage_carve(c, &to, 1);
    }));
    hipStream_t s = L->stream;
    if (n == 0) {
        HK_HIP(hipMemsetAsync(to.p, 0, to.bytes, s));
        HK_TRY(stage_download(L, &to, 1));
        return L->settle();
    }
    HK_TRY(stage_upload(L, &in, 1));
    HK_HIP(hipMemcpyAsync(tab_d, tab, sizeof(tab), hipMemcpyHostToDevice, s));
    HK_HIP(hipMemsetAsync(flag, 0, 4, s));
    // the partials and the error word first: nothing touches sums_out before the host has read it (as hk_ram_stage1_witness)
    HK_LAUNCH((k_cs_chunks<Fr>), dim3(n_wgs, n_groups), dim3(CS_WG), 0, s, (const Fr*)tab_d, (const u32*)in.p, (u64)n,
              (u32)n_classes, n_chunks, nbits, part, flag);
    u32 fl = 0;
    HK_HIP(hipMemcpyAsync(&fl, flag, 4, hipMemcpyDeviceToHost, s));
    HK_HIP(hipStreamSynchronize(s));
    if (fl) { HK_TRY(L->settle()); return HK_ERR_ARG; }
    HK_LAUNCH((k_cs_reduce<Fr>), dim3((u32)n_classes), dim3(CS_WG), 0, s, (const Fr*)part, n_wgs, (Fr*)to.p);
    HK_TRY(stage_download(L, &to, 1));
    return L->settle();                                                     // `tab` is read until here
}

}  // namespace hk
#endif  // __HIPCC__
