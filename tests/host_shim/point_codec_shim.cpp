// Host-compiled view of the PRODUCT's point_codec.cuh (g++): the HK_HD bodies the kernels k_field_sqrt,
// k_points_decompress and k_points_compress run per lane, here in a loop over the elements.  The subgroup test of
// hk_points_decompress_* (check != 0) is verify.cuh's and is not part of this view.  Test-only; never part of libhekaton.
//
// Built twice by tests/test_point_codec_cpu.py: as a shared object (the extern "C" entries, compared with the Python mirror)
// and, with -DPOINT_CODEC_MAIN, as a stand-alone program that prints one digest per case (run plain and under
// -fsanitize=address,undefined: same digests, clean exit).
#include "../../hekaton_system_amd/csrc/point_codec.cuh"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace hk;

template <class F>
static void field_sqrt(const void* in, size_t n, void* out, unsigned char* ok) {
    for (size_t i = 0; i < n; i++) {
        F a, r;
        memcpy(&a, (const char*)in + i * sizeof(F), sizeof(F));
        ok[i] = pc_sqrt_smaller(a, &r) ? 1 : 0;
        memcpy((char*)out + i * sizeof(F), &r, sizeof(F));
    }
}
template <class F>
static void decompress(const void* x_canon, const unsigned char* flags, size_t n, void* out, unsigned char* status) {
    for (size_t i = 0; i < n; i++) {
        F x;
        Affine<F> p;
        memcpy(&x, (const char*)x_canon + i * sizeof(F), sizeof(F));
        status[i] = pc_decompress(x, flags[i], &p);
        memcpy((char*)out + i * sizeof(p), &p, sizeof(p));
    }
}
template <class F>
static void compress(const void* pts, size_t n, void* x_canon, unsigned char* flags) {
    for (size_t i = 0; i < n; i++) {
        Affine<F> p;
        F x;
        memcpy(&p, (const char*)pts + i * sizeof(p), sizeof(p));
        flags[i] = pc_compress(p, &x);
        memcpy((char*)x_canon + i * sizeof(F), &x, sizeof(F));
    }
}

// f.template operator() is C++20: a tag argument picks the field instead
template <class Fn>
static void dispatch(int curve, int which, Fn&& f) {
    if (curve == 0) { if (which == 1) f(Fp<Bn254FqP>()); else f(Fp2<Bn254FqP>()); }
    else { if (which == 1) f(Fp<Bls381FqP>()); else f(Fp2<Bls381FqP>()); }
}

extern "C" {
// curve: 0 bn254, 1 bls12-381; which / group: 1 = Fq / G1, 2 = Fq2 / G2; the arguments of the hk_ entries, host buffers only
void shim_field_sqrt(int curve, int which, const void* in, size_t n, void* out, unsigned char* ok) {
    dispatch(curve, which, [&](auto t) { field_sqrt<decltype(t)>(in, n, out, ok); });
}
void shim_points_decompress(int curve, int group, const void* x_canon, const unsigned char* flags, size_t n, void* out,
                            unsigned char* status) {
    dispatch(curve, group, [&](auto t) { decompress<decltype(t)>(x_canon, flags, n, out, status); });
}
void shim_points_compress(int curve, int group, const void* pts, size_t n, void* x_canon, unsigned char* flags) {
    dispatch(curve, group, [&](auto t) { compress<decltype(t)>(pts, n, x_canon, flags); });
}
}

#ifdef POINT_CODEC_MAIN
static u64 fnv(const void* p, size_t n, u64 h = 1469598103934665603ull) {
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}
// field elements from a seed: Montgomery products and sums of what came before stay in [0, p)
template <class P>
static Fp<P> next_value(Fp<P>& state) {
    state = Fp<P>::add(Fp<P>::mul(state, state), Fp<P>::r2());
    return state;
}
template <class P>
static Fp2<P> next_value2(Fp<P>& state) {
    Fp2<P> r;
    r.c0 = next_value(state);
    r.c1 = next_value(state);
    return r;
}
template <class P>
static void next_of(Fp<P>& st, Fp<P>* out) { *out = next_value(st); }
template <class P>
static void next_of(Fp<P>& st, Fp2<P>* out) { *out = next_value2(st); }

// n elements: squares at even places; decompress what x they are as (mostly off-curve and on-curve mixed), compress the result
template <class P, class F>
static void run_cases(const char* name) {
    Fp<P> st = Fp<P>::r2();
    for (size_t n : {(size_t)1, (size_t)63, (size_t)65}) {
        std::vector<F> in(n), root(n), x(n), xc(n);
        std::vector<Affine<F>> pts(n);
        std::vector<unsigned char> ok(n), flags(n), status(n), fl2(n);
        for (size_t i = 0; i < n; i++) {
            F v;
            next_of(st, &v);
            in[i] = i % 2 ? v : F::sqr(v);
            x[i] = pc_from_mont(v);
            flags[i] = i % 7 == 3 ? CODEC_FLAG_INF : (i % 3 ? CODEC_FLAG_Y_LARGER : 0);
        }
        if (n > 2) { in[1] = F::zero(); x[2] = F::zero(); }
        field_sqrt<F>(in.data(), n, root.data(), ok.data());
        decompress<F>(x.data(), flags.data(), n, pts.data(), status.data());
        compress<F>(pts.data(), n, xc.data(), fl2.data());
        u64 h = fnv(root.data(), n * sizeof(F));
        h = fnv(ok.data(), n, h);
        h = fnv(pts.data(), n * sizeof(Affine<F>), h);
        h = fnv(status.data(), n, h);
        h = fnv(xc.data(), n * sizeof(F), h);
        h = fnv(fl2.data(), n, h);
        size_t n_ok = 0, n_on = 0;
        for (size_t i = 0; i < n; i++) { n_ok += ok[i]; n_on += status[i] == CODEC_OK; }
        printf("%s n=%zu roots=%zu points=%zu %016llx\n", name, n, n_ok, n_on, (unsigned long long)h);
    }
}
int main() {
    run_cases<Bn254FqP, Fp<Bn254FqP>>("bn254 fq");
    run_cases<Bn254FqP, Fp2<Bn254FqP>>("bn254 fq2");
    run_cases<Bls381FqP, Fp<Bls381FqP>>("bls12_381 fq");
    run_cases<Bls381FqP, Fp2<Bls381FqP>>("bls12_381 fq2");
    return 0;
}
#endif
