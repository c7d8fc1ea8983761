// point_codec.cuh — compressed curve points on the device (hk_field_sqrt, hk_points_decompress_*, hk_points_compress_*;
// DESIGN.md section 4q): what ark-ec's `get_point_from_x_unchecked` / `SWFlags::from_y_coordinate` do per point under
// `deserialize_compressed` / `serialize_compressed`, one lane per element.
//
//   square root in Fq   q = 3 mod 4 on both curves, q = 4 k + 3: t = a^k, s = a t = a^((q + 1) / 4), accepted iff s^2 == a.
//                       k = q >> 2 comes from P::MOD in constexpr code; the walk over its bits is uniform over the wave
//                       (plain square-and-multiply, no table).  s^2 = a a^((q - 1) / 2) = +-a: where a is no square, s is
//                       the root of -a, and t = +-1 / s - both are used below.
//   square root in Fq2  the complex method with two such powers and no inversion: alpha = sqrt(a0^2 + a1^2),
//                       d = (a0 + alpha) / 2 (d = a0 when a1 == 0), t = d^k, c0 = d t, w = a1 t / 2.  c0^2 == d: the root is
//                       (c0, w), since 1 / c0 = t.  Else c0^2 == -d and 1 / c0 = -t: the other d' = (a0 - alpha) / 2 =
//                       a1^2 / (4 (-d)) has the root -w, and the root of a is (-w, c0) - which for a1 == 0 is (0, s), s^2 =
//                       -a0.  Whatever came out is squared and compared with a, so a non-square norm needs no test of its own.
//   sign                ArkCodec._y_negative: on canonical values, y is the larger of (y, -y) iff y > (q - 1) / 2; in Fq2
//                       decided on c1 unless c1 == 0, then on c0.
//
// The arithmetic bodies are HK_HD and include nothing of HIP: tests/host_shim/point_codec_shim.cpp runs them on the host.
// The kernels, the subgroup test (point_valid, verify.cuh) and the host orchestration CodecRun<P> are hipcc-only;
// hk_<curve>_codec.hip instantiates them.
#pragma once
#include "tower.cuh"

namespace hk {

// the statuses of hk_points_decompress_*
constexpr unsigned char CODEC_BAD_X = 0, CODEC_OK = 1, CODEC_NOT_IN_SUBGROUP = 2;
// flag byte of a compressed point
constexpr unsigned char CODEC_FLAG_INF = 1, CODEC_FLAG_Y_LARGER = 2;

template <int N> struct CodecLimbs { u32 v[N]; };
template <class P>
constexpr CodecLimbs<P::N> codec_mod_shr(int s) {
    CodecLimbs<P::N> r = {};
    for (int i = 0; i < P::N; i++) r.v[i] = (P::MOD[i] >> s) | (i + 1 < P::N ? P::MOD[i + 1] << (32 - s) : 0u);
    return r;
}
template <class P>
struct CodecParams {
    static_assert((P::MOD[0] & 3u) == 3u, "the square root below needs q = 3 mod 4");
    static constexpr CodecLimbs<P::N> K = codec_mod_shr<P>(2);          // (q - 3) / 4
    static constexpr CodecLimbs<P::N> HALF = codec_mod_shr<P>(1);       // (q - 1) / 2
};
// b of y^2 = x^3 + b in G1 (the twist's is TowerParams<P>::B_TWIST)
template <class P> struct CodecG1B;
template <> struct CodecG1B<Bn254FqP> { static constexpr u32 B = 3; };
template <> struct CodecG1B<Bls381FqP> { static constexpr u32 B = 4; };

// a^((q - 3) / 4).  Out of line: the limb loop unrolls, so every limb of the exponent is an immediate and its bit tests are
// scalar; a 12-limb product is a call with register arguments (Fp::mul_call), as in Fp2.
template <class P>
HK_RARE Fp<P> pc_pow_k(const Fp<P>& a) {
    typedef Fp<P> F;
    F r = F::one();
    HK_UNROLL for (int i = P::N - 1; i >= 0; i--) {
        const u32 e = CodecParams<P>::K.v[i];
        HK_NOUNROLL for (int bit = 31; bit >= 0; bit--) {
            r = Fp2<P>::bmul(r, r);
            if ((e >> bit) & 1u) r = Fp2<P>::bmul(r, a);
        }
    }
    return r;
}

// canonical limbs: a > (q - 1) / 2, a < q
template <class P>
HK_HD bool pc_gt_half(const Fp<P>& a) {
    bool gt = false, eq = true;
    HK_UNROLL for (int i = P::N - 1; i >= 0; i--) {
        const u32 h = CodecParams<P>::HALF.v[i];
        gt = gt || (eq && a.v[i] > h);
        eq = eq && a.v[i] == h;
    }
    return gt;
}
template <class P>
HK_HD bool pc_below_q(const Fp<P>& a) {
    bool lt = false, eq = true;
    HK_UNROLL for (int i = P::N - 1; i >= 0; i--) {
        lt = lt || (eq && a.v[i] < P::MOD[i]);
        eq = eq && a.v[i] == P::MOD[i];
    }
    return lt;
}
template <class P>
HK_HD bool pc_below_q(const Fp2<P>& a) { return pc_below_q(a.c0) && pc_below_q(a.c1); }

// plain limb test: memory is canonical, and the ABI's infinity is all zeros
template <class P>
HK_HD bool pc_all_zero(const Fp<P>& a) {
    u32 acc = 0;
    HK_UNROLL for (int i = 0; i < P::N; i++) acc |= a.v[i];
    return acc == 0;
}
template <class P>
HK_HD bool pc_all_zero(const Fp2<P>& a) { return pc_all_zero(a.c0) && pc_all_zero(a.c1); }

template <class P>
HK_HD Fp<P> pc_to_mont(const Fp<P>& a) { return Fp<P>::to_mont(a); }
template <class P>
HK_HD Fp2<P> pc_to_mont(const Fp2<P>& a) { Fp2<P> r; r.c0 = Fp<P>::to_mont(a.c0); r.c1 = Fp<P>::to_mont(a.c1); return r; }
template <class P>
HK_HD Fp<P> pc_from_mont(const Fp<P>& a) { return Fp<P>::from_mont(a); }
template <class P>
HK_HD Fp2<P> pc_from_mont(const Fp2<P>& a) { Fp2<P> r; r.c0 = Fp<P>::from_mont(a.c0); r.c1 = Fp<P>::from_mont(a.c1); return r; }

// the sign rule, on a Montgomery value: y is the larger of (y, -y)
template <class P>
HK_HD bool pc_larger(const Fp<P>& y) { return pc_gt_half(pc_from_mont(y)); }
template <class P>
HK_HD bool pc_larger(const Fp2<P>& y) {
    const Fp2<P> c = pc_from_mont(y);
    return pc_all_zero(c.c1) ? pc_gt_half(c.c0) : pc_gt_half(c.c1);
}

template <class P>
HK_HD Fp<P> pc_select(bool take, const Fp<P>& a, const Fp<P>& b) {
    Fp<P> r;
    HK_UNROLL for (int i = 0; i < P::N; i++) r.v[i] = take ? a.v[i] : b.v[i];
    return r;
}

// *root = some square root of a (Montgomery; canonical limbs) and true, or false
template <class P>
HK_HD bool pc_sqrt(const Fp<P>& a, Fp<P>* root) {
    typedef Fp<P> F;
    const F s = F::canon(F::mul(a, pc_pow_k(a)));
    *root = s;
    return F::sqr(s) == a;
}
template <class P>
HK_HD bool pc_sqrt(const Fp2<P>& a, Fp2<P>* root) {
    typedef Fp<P> B;
    const B norm = B::add(B::sqr(a.c0), B::sqr(a.c1));
    const B alpha = B::mul(norm, pc_pow_k(norm));
    const B d = pc_select(a.c1.is_zero(), a.c0, B::halve(B::add(a.c0, alpha)));
    const B t = pc_pow_k(d);
    const B c0 = B::mul(d, t);
    const B w = B::halve(B::mul(a.c1, t));
    const bool pos = B::sqr(c0) == d;
    Fp2<P> r;
    r.c0 = B::canon(pc_select(pos, c0, B::neg(w)));
    r.c1 = B::canon(pc_select(pos, w, c0));
    *root = r;
    return Fp2<P>::sqr(r) == a;
}

// the root of a that is not larger than its negative (zero where a has none)
template <class F>
HK_HD bool pc_sqrt_smaller(const F& a, F* root) {
    F r;
    const bool ok = pc_sqrt(a, &r);
    if (pc_larger(r)) r = F::canon(F::neg(r));
    *root = ok ? r : F::zero();
    return ok;
}

template <class P>
HK_HD Fp<P> pc_curve_b(const Fp<P>*) {
    Fp<P> b = Fp<P>::one();
    for (u32 i = 1; i < CodecG1B<P>::B; i++) b = Fp<P>::add(b, Fp<P>::one());
    return b;
}
template <class P>
HK_HD Fp2<P> pc_curve_b(const Fp2<P>*) { return fp2_const<P>(TowerParams<P>::B_TWIST); }

// x canonical, flags as CODEC_FLAG_* -> the affine Montgomery point with the root of x^3 + b the flag names, canonical limbs.
// CODEC_BAD_X (x not below q, no root) leaves zeros.
template <class F>
HK_HD unsigned char pc_decompress(const F& x_canon, unsigned char flags, Affine<F>* out) {
    *out = Affine<F>::inf();
    if (flags & CODEC_FLAG_INF) return CODEC_OK;
    if (!pc_below_q(x_canon)) return CODEC_BAD_X;
    const F x = pc_to_mont(x_canon);
    const F rhs = F::add(F::mul(F::sqr(x), x), pc_curve_b((const F*)nullptr));
    F y;
    if (!pc_sqrt(rhs, &y)) return CODEC_BAD_X;
    if (pc_larger(y) != ((flags & CODEC_FLAG_Y_LARGER) != 0)) y = F::canon(F::neg(y));
    out->x = F::canon(x);
    out->y = y;
    return CODEC_OK;
}

// the inverse: canonical x and the flag byte of an affine Montgomery point.  No curve check.
template <class F>
HK_HD unsigned char pc_compress(const Affine<F>& p, F* x_canon) {
    if (pc_all_zero(p.x) && pc_all_zero(p.y)) {
        *x_canon = F::zero();
        return CODEC_FLAG_INF;
    }
    *x_canon = pc_from_mont(p.x);
    return pc_larger(p.y) ? CODEC_FLAG_Y_LARGER : 0;
}

}  // namespace hk

#if defined(__HIPCC__)
#include "verify.cuh"

namespace hk {

static_assert(CodecG1B<Bn254FqP>::B == SubgroupTest<Bn254FqP>::G1_B && CodecG1B<Bls381FqP>::B == SubgroupTest<Bls381FqP>::G1_B,
              "one b per curve");

constexpr size_t CODEC_CHUNK = (size_t)1 << 20;      // elements per pass: bounds the lane's scratch for host buffers

// out[i] = the smaller root of in[i] (Montgomery) or zero, ok[i] = 1 / 0
template <class F>
__global__ void __launch_bounds__(64)
k_field_sqrt(const F* __restrict__ in, u32 n, F* __restrict__ out, unsigned char* __restrict__ ok) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F r;
    const bool good = pc_sqrt_smaller(ld_vec(&in[i]), &r);
    st_vec(&out[i], r);
    ok[i] = good ? 1 : 0;
}

// status[i]: CODEC_OK, CODEC_BAD_X (zeros written) or - check != 0 only - CODEC_NOT_IN_SUBGROUP (the point is written)
template <class F>
__global__ void __launch_bounds__(64)
k_points_decompress(const F* __restrict__ x_canon, const unsigned char* __restrict__ flags, u32 n, int check,
                    Affine<F>* __restrict__ out, unsigned char* __restrict__ status) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> p;
    unsigned char st = pc_decompress(ld_vec(&x_canon[i]), flags[i], &p);
    if (check && st == CODEC_OK && !point_valid(p)) st = CODEC_NOT_IN_SUBGROUP;
    st_vec(&out[i], p);
    status[i] = st;
}

template <class F>
__global__ void __launch_bounds__(64)
k_points_compress(const Affine<F>* __restrict__ pts, u32 n, F* __restrict__ x_canon, unsigned char* __restrict__ flags) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F x;
    const unsigned char fl = pc_compress(ld_vec(&pts[i]), &x);
    st_vec(&x_canon[i], x);
    flags[i] = fl;
}

// One element-wise pass over n elements in chunks: buffer k holds elements of sz[k] bytes, the first n_in are inputs.
// launch(chunk's device pointers, elements) queues the kernel on the lane's stream.
template <class Launch>
static hk_status codec_pass(hk_ctx* ctx, void* const* bufs, const size_t* sz, int n_bufs, int n_in, size_t n, Launch&& launch) {
    LaneGuard g(ctx);
    Lane* L = g.lane;
    if (!L) return HK_ERR_DEVICE;
    for (size_t off = 0; off < n; off += CODEC_CHUNK) {
        const size_t k = n - off < CODEC_CHUNK ? n - off : CODEC_CHUNK;
        Staged io[4];
        for (int b = 0; b < n_bufs; b++) io[b] = staged((const char*)bufs[b] + off * sz[b], k * sz[b]);
        HK_TRY(L->carve([&](Carve& c) { stage_carve(c, io, (size_t)n_bufs); }));
        HK_TRY(stage_upload(L, io, (size_t)n_in));
        void* p[4];
        for (int b = 0; b < n_bufs; b++) p[b] = io[b].p;
        HK_TRY(launch(L->stream, p, (u32)k));
        HK_TRY(stage_download(L, io + n_in, (size_t)(n_bufs - n_in)));
        HK_TRY(L->settle());
    }
    return HK_OK;
}

template <class P>
hk_status CodecRun<P>::field_sqrt(hk_ctx* ctx, int which, const void* in, size_t n, void* out, unsigned char* ok) {
    auto run = [&](auto ftag) -> hk_status {
        typedef decltype(ftag) F;
        void* bufs[3] = {(void*)in, out, ok};
        const size_t sz[3] = {sizeof(F), sizeof(F), 1};
        return codec_pass(ctx, bufs, sz, 3, 1, n, [](hipStream_t s, void* const* p, u32 k) {
            HK_LAUNCH((k_field_sqrt<F>), dim3((k + 63) / 64), dim3(64), 0, s, (const F*)p[0], k, (F*)p[1], (unsigned char*)p[2]);
            return HK_OK;
        });
    };
    return which == 1 ? run(Fp<P>()) : run(Fp2<P>());
}

template <class P>
hk_status CodecRun<P>::points_decompress(hk_ctx* ctx, int group, const void* x_canon, const unsigned char* flags, size_t n,
                                         int check, void* points_out, unsigned char* status) {
    auto run = [&](auto ftag) -> hk_status {
        typedef decltype(ftag) F;
        void* bufs[4] = {(void*)x_canon, (void*)flags, points_out, status};
        const size_t sz[4] = {sizeof(F), 1, sizeof(Affine<F>), 1};
        return codec_pass(ctx, bufs, sz, 4, 2, n, [check](hipStream_t s, void* const* p, u32 k) {
            HK_LAUNCH((k_points_decompress<F>), dim3((k + 63) / 64), dim3(64), 0, s, (const F*)p[0], (const unsigned char*)p[1],
                      k, check, (Affine<F>*)p[2], (unsigned char*)p[3]);
            return HK_OK;
        });
    };
    return group == 1 ? run(Fp<P>()) : run(Fp2<P>());
}

template <class P>
hk_status CodecRun<P>::points_compress(hk_ctx* ctx, int group, const void* points, size_t n, void* x_canon_out,
                                       unsigned char* flags_out) {
    auto run = [&](auto ftag) -> hk_status {
        typedef decltype(ftag) F;
        void* bufs[3] = {(void*)points, x_canon_out, flags_out};
        const size_t sz[3] = {sizeof(Affine<F>), sizeof(F), 1};
        return codec_pass(ctx, bufs, sz, 3, 1, n, [](hipStream_t s, void* const* p, u32 k) {
            HK_LAUNCH((k_points_compress<F>), dim3((k + 63) / 64), dim3(64), 0, s, (const Affine<F>*)p[0], k, (F*)p[1],
                      (unsigned char*)p[2]);
            return HK_OK;
        });
    };
    return group == 1 ? run(Fp<P>()) : run(Fp2<P>());
}

}  // namespace hk
#endif  // __HIPCC__
