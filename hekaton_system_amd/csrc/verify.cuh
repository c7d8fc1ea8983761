// verify.cuh — CP-Groth16 proof verification (cp-groth16/src/verifier.rs:7-71) for many proofs of one verifying key:
//
//     e(A, B) e(IC, -gamma) prod_j e(D_j, -delta_j) e(C, -delta_last) == e(alpha, beta),  IC = abc[0] + sum_k x_k abc[k+1]
//
// Kernels: k_points_check (on-curve + prime-order subgroup test of untrusted points, one lane per point),
// k_verify_ic (prepared inputs: one lane per proof, one interleaved double-and-add chain over its public inputs),
// k_verify_tree_lines (first tree level of N independent multi-pairings: the lines of the proofs' B points and the
// key's PREPARED lines of -gamma / -delta_j, evaluated at the matching G1 points), k_verify_coeffs (the combined inputs
// of the randomised batch check), k_verify_rand_zero (a zero r_i sends its chunk to the per-proof path) and
// k_verify_verdict.  The rest of the Miller pipeline (k_pair_lines, k_pair_tree, k_pair_horner) and the GT power are the
// multi-pairing's own (pairing_wave.cuh).  Host orchestration: VerifyRun<P>, explicitly instantiated in
// hk_<curve>_pair.hip.  DESIGN.md section 4f.
#pragma once
#include "pairing_driver_impl.cuh"

namespace hk {

constexpr u32 VERIFY_CHUNK = 1024;          // proofs per pass: bounds the lane's scratch and every grid dimension
constexpr unsigned char VERDICT_BAD_POINT = 2;

// subgroup tests by endomorphism (ark-ec 0.4 `is_in_correct_subgroup_assuming_on_curve`), canonical scalar limbs:
//   BN254 G1: cofactor 1.  BN254 G2: psi(Q) == [6 x^2] Q.  BLS12-381 G1: phi(P) == -[x^2] P.  BLS12-381 G2: psi(Q) == [x] Q
//   with x < 0, i.e. -[|x|] Q.  phi is EndoOf<Fp<P>>::apply (beta of eigenvalue -x^2 mod r), psi is g2_psi (eigenvalue
//   q mod r); tests/test_verify_gpu.py pins each test against [r] P == O.
template <class P> struct SubgroupTest;
template <> struct SubgroupTest<Bn254FqP> {
    static constexpr u32 G1_B = 3;
    static constexpr bool G1_COFACTOR_ONE = true, G1_NEG = false, G2_NEG = false;
    HK_HD static void g1_k(u32 (&k)[4]) { k[0] = 0; k[1] = 0; k[2] = 0; k[3] = 0; }
    HK_HD static void g2_k(u32 (&k)[4]) { k[0] = 0xe87cfd46u; k[1] = 0xf83e9682u; k[2] = 0xeeb859fbu; k[3] = 0x6f4d8248u; }
};
template <> struct SubgroupTest<Bls381FqP> {
    static constexpr u32 G1_B = 4;
    static constexpr bool G1_COFACTOR_ONE = false, G1_NEG = true, G2_NEG = true;
    HK_HD static void g1_k(u32 (&k)[4]) { k[0] = 0x00000000u; k[1] = 0x00000001u; k[2] = 0x0001a402u; k[3] = 0xac45a401u; }
    HK_HD static void g2_k(u32 (&k)[4]) { k[0] = 0x00010000u; k[1] = 0xd2010000u; k[2] = 0; k[3] = 0; }
};

// e == (+-) r for an affine e (not infinity) and an XYZZ r
template <class F>
HK_HD bool affine_eq_xyzz(const Affine<F>& e, const XYZZ<F>& r, bool neg) {
    if (r.is_inf()) return false;
    F y = neg ? F::neg(r.y) : r.y;
    return F::mul(e.x, r.zz) == r.x && F::mul(e.y, r.zzz) == y;
}

// ark's AffineRepr::check: on the curve (y^2 = x^3 + b) and in the prime-order subgroup; infinity is valid
template <class P>
HK_HD bool point_valid(const Affine<Fp<P>>& p) {
    typedef Fp<P> F;
    typedef SubgroupTest<P> T;
    if (p.is_inf()) return true;
    F b = F::one();
    for (u32 i = 1; i < T::G1_B; i++) b = F::add(b, F::one());
    if (!(F::sqr(p.y) == F::add(F::mul(F::sqr(p.x), p.x), b))) return false;
    if (T::G1_COFACTOR_ONE) return true;
    u32 k[4];
    T::g1_k(k);
    return affine_eq_xyzz(EndoOf<F>::apply(p), ec_mul_limbs(XYZZ<F>::from_affine(p), k), T::G1_NEG);
}
template <class P>
HK_HD bool point_valid(const Affine<Fp2<P>>& q) {
    typedef Fp2<P> F;
    typedef SubgroupTest<P> T;
    if (q.is_inf()) return true;
    F b = fp2_const<P>(TowerParams<P>::B_TWIST);
    if (!(F::sqr(q.y) == F::add(F::mul(F::sqr(q.x), q.x), b))) return false;
    u32 k[4];
    T::g2_k(k);
    return affine_eq_xyzz(g2_psi(q), ec_mul_limbs(XYZZ<F>::from_affine(q), k), T::G2_NEG);
}

#if defined(__HIPCC__)

// per == 0: out[i] = point i is valid (hk_points_check_*); else an invalid point i marks its proof: out[i / per] = 2
template <class F>
__global__ void __launch_bounds__(64)
k_points_check(const Affine<F>* __restrict__ pts, u32 n, u32 per, unsigned char* __restrict__ out) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool ok = point_valid(ld_vec(&pts[i]));
    if (per == 0) out[i] = ok ? 1 : 0;
    else if (!ok) out[i / per] = VERDICT_BAD_POINT;
}

// out[p * ostride] = base0 + sum_{k < nk} s[p][k] bases[k] (prepare_inputs, verifier.rs:45-62; base0 == nullptr: no
// constant term).  One lane per proof; the scalars go four at a time through ONE MSB-first double-and-add chain, so
// its 255 doublings serve every term (Straus).  Exact for any nk.
template <class P, class Fr>
__global__ void __launch_bounds__(64)
k_verify_ic(const Affine<Fp<P>>* __restrict__ bases, u32 nk, const Fr* __restrict__ scalars_mont,
            const Affine<Fp<P>>* __restrict__ base0, u32 n, Affine<Fp<P>>* __restrict__ out, u32 ostride) {
    typedef Fp<P> F;
    u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const Fr* sc = scalars_mont + (size_t)p * nk;
    XYZZ<F> total = base0 ? XYZZ<F>::from_affine(ld_vec(base0)) : XYZZ<F>::inf();
    HK_NOUNROLL for (u32 k0 = 0; k0 < nk; k0 += 4) {
        u32 c[4][Fr::N];
        HK_UNROLL for (int j = 0; j < 4; j++) {
            Fr s = k0 + j < nk ? Fr::from_mont(ld_vec(&sc[k0 + j])) : Fr::zero();
            HK_UNROLL for (int l = 0; l < Fr::N; l++) c[j][l] = s.v[l];
        }
        XYZZ<F> acc = XYZZ<F>::inf();
        HK_UNROLL for (int l = Fr::N - 1; l >= 0; l--) {
            HK_NOUNROLL for (int bit = 31; bit >= 0; bit--) {
                acc = ec_dbl_ni(acc);
                HK_UNROLL for (int j = 0; j < 4; j++)
                    if ((c[j][l] >> bit) & 1u) acc = ec_madd_ni(acc, ld_vec(&bases[k0 + j]));
            }
        }
        total = ec_add_ni(total, acc);
    }
    out[(size_t)p * ostride] = ec_to_affine(total);
}

// The members of N independent multi-pairings.  Product p multiplies M = dyn_per + n_st pairs:
//   member m < dyn_per: raw line dyn_lines[s * n_dyn + p * dyn_per + m] at dyn_g1[p * dyn_per + m] (the proofs' B lines);
//   member dyn_per + j: prepared line st_lines[s * n_st + j] at st_g1[p * n_st + j] (-gamma, -delta_j of the key).
template <class P>
struct VerifyMembers {
    const Line6<P>* dyn_lines;
    const Affine<Fp<P>>* dyn_g1;
    u32 n_dyn, dyn_per;
    const Line6<P>* st_lines;
    const Affine<Fp<P>>* st_g1;
    u32 n_st;
};

// k_pair_tree_lines over VerifyMembers: wave g of row y = row0 + blockIdx.y = p * S + s multiplies members
// [g c, min((g + 1) c, M)) of product p at step s into out[y * gridDim.x + g]
template <class P>
__global__ void __launch_bounds__(64)
k_verify_tree_lines(VerifyMembers<P> vm, u32 S, u32 c, u32 row0, Fp12<P>* __restrict__ out) {
    extern __shared__ unsigned char pair_lds[];
    typedef WaveF12<P> W;
    typedef Fp<P> Fq;
    typedef TowerParams<P> T;
    WaveArea<P>* w = reinterpret_cast<WaveArea<P>*>(pair_lds);
    Fq* s = reinterpret_cast<Fq*>(pair_lds + sizeof(WaveArea<P>));
    WaveF12<P>::init(w);
    Fq *acc = s, *cur = s + WV_SLOT;
    u32 M = vm.dyn_per + vm.n_st;
    u32 lo = blockIdx.x * c, hi = min(lo + c, M);
    u32 row = row0 + blockIdx.y;
    u32 p = row / S, st = row % S;
    u32 lane = threadIdx.x;
    int src_idx = -1, scale = 0;                    // as k_pair_tree_lines: 0 none, 1 by p.x, 2 by p.y
    if (lane < 2) { src_idx = lane; scale = T::TWIST_IS_D ? 2 : 0; }
    else if (T::TWIST_IS_D && lane >= 6 && lane < 8) { src_idx = 2 + (lane - 6); scale = 1; }
    else if (!T::TWIST_IS_D && lane >= 2 && lane < 4) { src_idx = 2 + (lane - 2); scale = 1; }
    else if (lane >= 8 && lane < 10) { src_idx = 4 + (lane - 8); scale = T::TWIST_IS_D ? 0 : 2; }
    auto load_line = [&](Fq* dst, u32 m) {
        const Line6<P>* ln;
        const Affine<Fq>* pt;
        if (m < vm.dyn_per) {
            size_t i = (size_t)p * vm.dyn_per + m;
            ln = vm.dyn_lines + (size_t)st * vm.n_dyn + i;
            pt = vm.dyn_g1 + i;
        } else {
            size_t j = m - vm.dyn_per;
            ln = vm.st_lines + (size_t)st * vm.n_st + j;
            pt = vm.st_g1 + (size_t)p * vm.n_st + j;
        }
        Fq v = Fq::zero();
        bool raw_nz = false, pt_nz = false;
        if (src_idx >= 0) {
            v = ld_vec(&reinterpret_cast<const Fq*>(ln)[src_idx]);
            raw_nz = !v.is_zero();
            if (scale) {
                Fq k = ld_vec(scale == 1 ? &pt->x : &pt->y);
                pt_nz = !k.is_zero();
                v = Fq::mul(v, k);
            }
        }
        bool one = __ballot(raw_nz) == 0 || __ballot(pt_nz) == 0;      // a member at infinity contributes 1
        if (lane < 13) dst[lane] = one ? (lane == 0 ? Fq::one() : Fq::zero()) : v;
        W::sync();
    };
    load_line(acc, lo);
    for (u32 m = lo + 1; m < hi; m++) {
        load_line(cur, m);
        W::mul(acc, acc, cur, w);
    }
    W::store(&out[(size_t)row * gridDim.x + blockIdx.x], acc);
}

// coef[0] = sum_i r_i, coef[k + 1] = sum_i r_i x[i][k] (Montgomery): the public input of the randomised batch check
template <class Fr>
__global__ void __launch_bounds__(64)
k_verify_coeffs(const Fr* __restrict__ r, const Fr* __restrict__ x, u32 n, u32 nk, Fr* __restrict__ coef) {
    u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nk) return;
    Fr acc = Fr::zero();
    HK_NOUNROLL for (u32 i = 0; i < n; i++) {
        Fr ri = ld_vec(&r[i]);
        acc = Fr::add(acc, k == 0 ? ri : Fr::mul(ri, ld_vec(&x[(size_t)i * nk + k - 1])));
    }
    coef[k] = Fr::canon(acc);
}

// zero[0] = 1 when some r_i == 0: its terms drop out of both sides of the batch equation, which would then hold whatever
// proof i is.  `zero` is the byte after the chunk's point flags, so the host reads both at once.
template <class Fr>
__global__ void __launch_bounds__(64)
k_verify_rand_zero(const Fr* __restrict__ r, u32 n, unsigned char* __restrict__ zero) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && ld_vec(&r[i]).is_zero()) *zero = 1;
}

// verdicts[p] = flags[p] when a point check marked the proof, else got[p] == want[p * want_stride]
template <class P>
__global__ void __launch_bounds__(64)
k_verify_verdict(const Fp12<P>* __restrict__ got, const Fp12<P>* __restrict__ want, u32 want_stride, u32 n,
                 const unsigned char* __restrict__ flags, unsigned char* __restrict__ verdicts) {
    u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (flags && flags[p]) { verdicts[p] = flags[p]; return; }
    const u32* a = reinterpret_cast<const u32*>(&got[p]);
    const u32* b = reinterpret_cast<const u32*>(&want[(size_t)p * want_stride]);
    u32 diff = 0;
    for (u32 i = 0; i < sizeof(Fp12<P>) / 4; i++) diff |= a[i] ^ b[i];
    verdicts[p] = diff == 0 ? 1 : 0;
}

#endif  // __HIPCC__

// ---- host side ----------------------------------------------------------------------------------------------------
template <class P>
struct VkImpl {
    u32 n_deltas = 0, n_abc = 0;
    Affine<Fp<P>>* abc = nullptr;        // [n_abc] gamma_abc_g
    Line6<P>* lines = nullptr;           // [S][n_deltas + 1] raw lines of -gamma, -delta_0, .., -delta_last (ark G2Prepared)
    Fp12<P>* alpha_beta = nullptr;       // e(alpha, beta), device
};

template <class P>
static hk_status verify_lines(hipStream_t s, const Affine<Fp2<P>>* g2, u32 n, Line6<P>* lines) {
    PairLoop loop = PairLoopOf<P>::get();
    u32 S = PairRun<P>::steps();
    if ((size_t)n * 4 <= SPLIT_MAX_LANES)
        HK_LAUNCH((k_pair_lines<Fp2Q<P>>), dim3((4 * n + 63) / 64, 1), dim3(64), 0, s, (const Affine<Fp2Q<P>>*)g2, n, 1u,
                  loop, S, lines);
    else
        HK_LAUNCH((k_pair_lines<Fp2<P>>), dim3((n + 63) / 64, 1), dim3(64), 0, s, g2, n, 1u, loop, S, lines);
    return HK_OK;
}

// count products of M members each -> their final-exponentiated values out[count].  pp: two buffers of
// count * S * ceil(M / 16) Fq12.  Grid rows (count * S) go in launches of at most 65535.
template <class P>
static hk_status verify_products(hipStream_t s, const VerifyMembers<P>& vm, u32 count, Fp12<P>* pp0, Fp12<P>* pp1, Fp12<P>* out) {
    PairSteps st = pair_steps(PairLoopOf<P>::get(), TowerParams<P>::TWIST_IS_D);
    u32 S = (u32)st.n, M = vm.dyn_per + vm.n_st;
    u32 rows = count * S;
    size_t lds_tree = sizeof(WaveArea<P>) + 2 * WV_SLOT * sizeof(Fp<P>);
    size_t lds_fin = sizeof(WaveArea<P>) + WV_FINISH_SLOTS * WV_SLOT * sizeof(Fp<P>);
    u32 g = (M + 15) / 16;
    for (u32 r0 = 0; r0 < rows; r0 += 65535u) {
        u32 nr = rows - r0 < 65535u ? rows - r0 : 65535u;
        HK_LAUNCH((k_verify_tree_lines<P>), dim3(g, nr), dim3(64), lds_tree, s, vm, S, 16u, r0, pp0);
    }
    Fp12<P>* pp[2] = {pp0, pp1};
    int cur = 0;
    while (g > 1) {
        u32 groups = (g + 15) / 16;
        for (u32 r0 = 0; r0 < rows; r0 += 65535u) {
            u32 nr = rows - r0 < 65535u ? rows - r0 : 65535u;
            HK_LAUNCH((k_pair_tree<P>), dim3(groups, nr), dim3(64), lds_tree, s, (const Fp12<P>*)pp[cur] + (size_t)r0 * g, g,
                      16u, pp[cur ^ 1] + (size_t)r0 * groups);
        }
        cur ^= 1;
        g = groups;
    }
    HK_LAUNCH((k_pair_horner<P>), dim3(count), dim3(64), lds_fin, s, (const Fp12<P>*)pp[cur], st, out);
    return HK_OK;
}

template <class P>
hk_status VerifyRun<P>::vk_prepare(hk_ctx* ctx, const hk_vk_desc* d, hk_vk** out) {
    typedef Fp<P> Fq;
    typedef Fp2<P> Fq2;
    typedef Fp12<P> GT;
    *out = nullptr;
    if (d->n_deltas == 0 || d->n_abc == 0 || d->n_deltas > 4096 || d->n_abc > ((size_t)1 << 24)) return HK_ERR_LEN;
    if (!d->alpha_g || !d->beta_h || !d->gamma_h || !d->deltas_h || !d->gamma_abc_g) return HK_ERR_ARG;
    u32 nst = (u32)d->n_deltas + 1, S = PairRun<P>::steps();
    // the static right-hand sides, negated on the host (verifier.rs:10-16)
    std::vector<Affine<Fq2>> neg(nst);
    HK_HIP(hipSetDevice(ctx->device));
    HK_HIP(hipMemcpy(&neg[0], d->gamma_h, sizeof(Affine<Fq2>), hipMemcpyDefault));
    HK_HIP(hipMemcpy(&neg[1], d->deltas_h, d->n_deltas * sizeof(Affine<Fq2>), hipMemcpyDefault));
    for (auto& q : neg) q.y = Fq2::neg(q.y);
    Staged in[2] = {staged(d->alpha_g, sizeof(Affine<Fq>)), staged(d->beta_h, sizeof(Affine<Fq2>))};
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    size_t mbytes = PairRun<P>::scratch_bytes(1, 1, 1);
    Affine<Fq2>* g2;
    GT *miller, *prod;
    HK_TRY(L->carve([&](Carve& c) {
        g2 = c.n<Affine<Fq2>>(nst);
        stage_carve(c, in, 2);
        miller = (GT*)c.take(mbytes);
        prod = c.n<GT>(1);
    }));
    hipStream_t s = L->stream;
    HK_TRY(stage_upload(L, in, 2));
    VkImpl<P>* v = new VkImpl<P>();
    v->n_deltas = (u32)d->n_deltas;
    v->n_abc = (u32)d->n_abc;
    auto fail = [&](hk_status st) { (void)hipStreamSynchronize(s); (void)hipFree(v->abc); (void)hipFree(v->lines); (void)hipFree(v->alpha_beta); delete v; return st; };
    if (hipMalloc(&v->abc, d->n_abc * sizeof(Affine<Fq>)) != hipSuccess ||
        hipMalloc(&v->lines, (size_t)S * nst * sizeof(Line6<P>)) != hipSuccess || hipMalloc(&v->alpha_beta, sizeof(GT)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(HK_ERR_NOMEM);
    }
    if (hipMemcpyAsync(v->abc, d->gamma_abc_g, d->n_abc * sizeof(Affine<Fq>), hipMemcpyDefault, s) != hipSuccess ||
        hipMemcpyAsync(g2, neg.data(), nst * sizeof(Affine<Fq2>), hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(HK_ERR_DEVICE);
    hk_status st = verify_lines<P>(s, g2, nst, v->lines);
    if (st == HK_OK)
        st = PairRun<P>::run(s, (const Affine<Fq>*)in[0].p, (const Affine<Fq2>*)in[1].p, 1, 1, 1, miller, prod, v->alpha_beta);
    if (st == HK_OK) st = L->settle();
    if (st != HK_OK) return fail(st);
    hk_vk* h = new hk_vk();
    h->ops = ctx->ops;
    h->ctx = ctx;
    h->impl = v;
    *out = h;
    return HK_OK;
}

template <class P>
void VerifyRun<P>::vk_free(hk_vk* h) {
    VkImpl<P>* v = (VkImpl<P>*)h->impl;
    (void)hipSetDevice(h->ctx->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(v->abc);
    (void)hipFree(v->lines);
    (void)hipFree(v->alpha_beta);
    delete v;
    delete h;
}

template <class P>
hk_status VerifyRun<P>::vk_alpha_beta(const hk_vk* h, void* gt_out) {
    const VkImpl<P>* v = (const VkImpl<P>*)h->impl;
    HK_HIP(hipSetDevice(h->ctx->device));
    HK_HIP(hipMemcpy(gt_out, v->alpha_beta, sizeof(Fp12<P>), hipMemcpyDefault));
    return HK_OK;
}

template <class P>
hk_status VerifyRun<P>::points_check(hk_ctx* ctx, int group, const void* pts, size_t n, unsigned char* ok) {
    if (n == 0) return HK_OK;
    if (n >= ((size_t)1 << 31)) return HK_ERR_ARG;
    Staged io[2] = {staged(pts, n * (group == 1 ? sizeof(Affine<Fp<P>>) : sizeof(Affine<Fp2<P>>))), staged(ok, n)};
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    auto run = [&](auto ftag) -> hk_status {
        typedef decltype(ftag) F;
        HK_TRY(L->carve([&](Carve& c) { stage_carve(c, io, 2); }));
        HK_TRY(stage_upload(L, io, 1));
        HK_LAUNCH((k_points_check<F>), dim3((u32)((n + 63) / 64)), dim3(64), 0, L->stream, (const Affine<F>*)io[0].p, (u32)n,
                  0u, (unsigned char*)io[1].p);
        HK_TRY(stage_download(L, io + 1, 1));
        return L->settle();
    };
    return group == 1 ? run(Fp<P>()) : run(Fp2<P>());
}

template <class P>
hk_status VerifyRun<P>::verify_batch(hk_ctx* ctx, const hk_vk* h, const void* a, const void* b, const void* c, const void* ds,
                                     const void* inputs, size_t n, unsigned flags, const void* rand, unsigned char* verdicts) {
    typedef Fp<P> Fq;
    typedef Fp2<P> Fq2;
    typedef Fp12<P> GT;
    typedef typename ScalarOfQ<P>::type Fr;
    const VkImpl<P>* v = (const VkImpl<P>*)h->impl;
    const bool check = (flags & HK_VERIFY_CHECK_POINTS) != 0;
    if (rand && !check) return HK_ERR_ARG;                 // the randomised check is sound on the prime-order groups only
    if (n == 0) return HK_OK;
    const u32 nd = v->n_deltas, nst = nd + 1, nk = v->n_abc - 1, S = PairRun<P>::steps();
    if (!a || !b || !c || !verdicts || (nd > 1 && !ds) || (nk && !inputs)) return HK_ERR_ARG;
    if (n >= ((size_t)1 << 31)) return HK_ERR_ARG;
    const size_t g1b = sizeof(Affine<Fq>), g2b = sizeof(Affine<Fq2>), frb = sizeof(Fr);
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    hipStream_t s = L->stream;
    const u32 gpp = (1 + nst + 15) / 16;                   // first-level groups of a per-proof product
    for (size_t o = 0; o < n; o += VERIFY_CHUNK) {
        const u32 m = (u32)(n - o < VERIFY_CHUNK ? n - o : VERIFY_CHUNK);
        const u32 gb = (m + nst + 15) / 16;                // ... of the batch product
        // this chunk of a, b, c, ds, inputs and rand, then of the verdicts
        Staged io[7] = {staged((const char*)a + o * g1b, m * g1b),
                        staged((const char*)b + o * g2b, m * g2b),
                        staged((const char*)c + o * g1b, m * g1b),
                        staged(nd > 1 ? (const char*)ds + o * (nd - 1) * g1b : nullptr, (size_t)m * (nd - 1) * g1b),
                        staged(nk ? (const char*)inputs + o * nk * frb : nullptr, (size_t)m * nk * frb),
                        staged(rand ? (const char*)rand + o * frb : nullptr, m * frb),
                        staged(verdicts + o, m)};
        unsigned char* flag;
        Affine<Fq>* gst;
        Line6<P>* lines;
        GT *pp0, *pp1, *res;
        // the randomised check's buffers (when `rand`)
        Affine<Fq>*ra = nullptr, *col = nullptr, *bst = nullptr;
        XYZZ<Fq>*xy = nullptr, *tab = nullptr, *sums = nullptr;
        Fq* pref = nullptr;
        Fr* coef = nullptr;
        GT *qa = nullptr, *qb = nullptr, *one = nullptr, *want = nullptr;
        unsigned char* eq = nullptr;
        HK_TRY(L->carve([&](Carve& k) {
            stage_carve(k, io, 7);
            flag = k.n<unsigned char>(m + 1);              // one per proof, then "some r_i is zero"
            gst = k.n<Affine<Fq>>((size_t)m * nst);
            lines = k.n<Line6<P>>((size_t)m * S);
            pp0 = k.n<GT>((size_t)m * S * gpp);
            pp1 = k.n<GT>((size_t)m * S * gpp);
            res = k.n<GT>(m);
            if (!rand) return;
            ra = k.n<Affine<Fq>>(m);
            xy = k.n<XYZZ<Fq>>(m);
            pref = k.n<Fq>(m);
            tab = (XYZZ<Fq>*)k.take(endo_tab_bytes<Fq>(m));
            col = k.n<Affine<Fq>>(m);
            sums = k.n<XYZZ<Fq>>(nst);
            bst = k.n<Affine<Fq>>(nst);
            coef = k.n<Fr>(nk + 1);
            qa = k.n<GT>((size_t)S * gb);
            qb = k.n<GT>((size_t)S * gb);
            one = k.n<GT>(1);
            want = k.n<GT>(1);
            eq = k.n<unsigned char>(1);
        }));
        const void *ad = io[0].p, *bd = io[1].p, *cd = io[2].p, *dd = io[3].p, *xd = io[4].p, *rd = io[5].p;
        unsigned char* vd = (unsigned char*)io[6].p;
        HK_TRY(stage_upload(L, io, 6));
        HK_HIP(hipMemsetAsync(flag, 0, m + 1, s));
        bool any_bad = false;
        if (check) {
            HK_LAUNCH((k_points_check<Fq>), dim3((m + 63) / 64), dim3(64), 0, s, (const Affine<Fq>*)ad, m, 1u, flag);
            HK_LAUNCH((k_points_check<Fq2>), dim3((m + 63) / 64), dim3(64), 0, s, (const Affine<Fq2>*)bd, m, 1u, flag);
            HK_LAUNCH((k_points_check<Fq>), dim3((m + 63) / 64), dim3(64), 0, s, (const Affine<Fq>*)cd, m, 1u, flag);
            if (nd > 1)
                HK_LAUNCH((k_points_check<Fq>), dim3((u32)(((size_t)m * (nd - 1) + 63) / 64)), dim3(64), 0, s,
                          (const Affine<Fq>*)dd, m * (nd - 1), nd - 1, flag);
        }
        HK_TRY(verify_lines<P>(s, (const Affine<Fq2>*)bd, m, lines));
        bool batch_ok = false;
        if (rand) {
            // one randomised equation for the chunk; a proof with a bad point, or a zero r_i, sends the chunk to the
            // per-proof path
            HK_LAUNCH((k_verify_rand_zero<Fr>), dim3((m + 63) / 64), dim3(64), 0, s, (const Fr*)rd, m, flag + m);
            std::vector<unsigned char> fh(m + 1);
            HK_HIP(hipMemcpyAsync(fh.data(), flag, m + 1, hipMemcpyDeviceToHost, s));
            HK_HIP(hipStreamSynchronize(s));
            for (u32 i = 0; i <= m; i++) any_bad = any_bad || fh[i];
        }
        if (rand && !any_bad) {
            // sum r_i, sum r_i x_i -> sum r_i IC_i = (sum r_i) abc[0] + sum_k (sum_i r_i x_ik) abc[k + 1]
            HK_LAUNCH((k_verify_coeffs<Fr>), dim3((nk + 1 + 63) / 64), dim3(64), 0, s, (const Fr*)rd, (const Fr*)xd, m, nk, coef);
            HK_LAUNCH((k_verify_ic<P, Fr>), dim3(1), dim3(64), 0, s, (const Affine<Fq>*)v->abc, nk + 1, (const Fr*)coef,
                      (const Affine<Fq>*)nullptr, 1u, bst, 1u);
            // sum r_i D_ij and sum r_i C_i: small MSMs over the proofs' columns
            for (u32 j = 0; j + 1 < nd; j++) {
                HK_HIP(hipMemcpy2DAsync(col, g1b, (const char*)dd + j * g1b, (nd - 1) * g1b, g1b, m, hipMemcpyDeviceToDevice, s));
                HK_TRY(MsmRun<Fq>::small_msm(s, col, rd, 1, m, tab, xy, sums + j));
            }
            HK_TRY(MsmRun<Fq>::small_msm(s, (const Affine<Fq>*)cd, rd, 1, m, tab, xy, sums + nd - 1));
            HK_TRY(MsmRun<Fq>::to_affine(s, sums, bst + 1, nd));
            // r_i A_i (the endomorphism-split sweep)
            HK_TRY(MsmRun<Fq>::scalar_mul_each(s, (const Affine<Fq>*)ad, rd, m, xy, pref, ra, tab));
            VerifyMembers<P> vm = {lines, ra, m, m, v->lines, bst, nst};
            HK_TRY(verify_products<P>(s, vm, 1, qa, qb, one));
            HK_TRY(PairRun<P>::gt_pow(s, v->alpha_beta, coef, 1, want, true));      // e(alpha, beta)^(sum r_i)
            HK_LAUNCH((k_verify_verdict<P>), dim3(1), dim3(64), 0, s, (const GT*)one, (const GT*)want, 0u, 1u,
                      (const unsigned char*)nullptr, eq);
            unsigned char eh = 0;
            HK_HIP(hipMemcpyAsync(&eh, eq, 1, hipMemcpyDeviceToHost, s));
            HK_HIP(hipStreamSynchronize(s));
            batch_ok = eh == 1;
            if (batch_ok) HK_HIP(hipMemsetAsync(vd, 1, m, s));
        }
        if (!batch_ok) {
            // per-proof: IC_p, then [IC_p, D_p0 .., C_p] side by side against the prepared lines
            HK_LAUNCH((k_verify_ic<P, Fr>), dim3((m + 63) / 64), dim3(64), 0, s, (const Affine<Fq>*)v->abc + 1, nk, (const Fr*)xd,
                      (const Affine<Fq>*)v->abc, m, gst, nst);
            if (nd > 1)
                HK_HIP(hipMemcpy2DAsync(gst + 1, nst * g1b, dd, (nd - 1) * g1b, (nd - 1) * g1b, m, hipMemcpyDeviceToDevice, s));
            HK_HIP(hipMemcpy2DAsync(gst + nd, nst * g1b, cd, g1b, g1b, m, hipMemcpyDeviceToDevice, s));
            VerifyMembers<P> vm = {lines, (const Affine<Fq>*)ad, m, 1, v->lines, gst, nst};
            HK_TRY(verify_products<P>(s, vm, m, pp0, pp1, res));
            HK_LAUNCH((k_verify_verdict<P>), dim3((m + 63) / 64), dim3(64), 0, s, (const GT*)res, (const GT*)v->alpha_beta, 0u, m,
                      check ? (const unsigned char*)flag : nullptr, vd);
        }
        HK_TRY(stage_download(L, io + 6, 1));
        HK_TRY(L->settle());
    }
    return HK_OK;
}

}  // namespace hk
