// What the test-only device shims (*_dev_shim.hip) share: the status convention, the device buffers with their 0xA5 fill, the
// end of a call, raw limb access, the build variant and the per-group translation-unit ladder.  Test-only; never part of
// libhekaton.
//
// Every host-side helper here has internal linkage.  Both variants of a shim and libhekaton get loaded into one process,
// and not every shim library is linked -Bsymbolic: an exported helper of one could be bound by another.
#pragma once
#include <vector>
#include "../../hekaton_system_amd/csrc/field.cuh"
using namespace hk;

// Part of the name of every kernel that exists in the shims only (k_field_op, k_wave_op, k_group_op, k_f2q_op,
// k_pow_from_tables_op): both variants get loaded into one test process, each must launch its own kernels, and a kernel trace
// tells them apart.  The exported dshim_*uses_asm functions return it: 1 when the arithmetic was compiled with the inline
// assembly of mont_asm.h, 0 for the -DHK_NO_ASM_MUL build.
#if defined(HK_NO_ASM_MUL)
constexpr int VARIANT = 0;
#else
constexpr int VARIANT = 1;
#endif

// registers <- limbs as they stand (that is how representatives in [p, 2p) get into registers), and back
template <class P> __device__ __forceinline__ void ld_raw(Fp<P>& f, const u32* p) {
    HK_UNROLL for (int i = 0; i < P::N; i++) f.v[i] = p[i];
}
template <class P> __device__ __forceinline__ void ld_raw(Fp2<P>& f, const u32* p) { ld_raw(f.c0, p); ld_raw(f.c1, p + P::N); }
template <class P> __device__ __forceinline__ void st_raw(u32* p, const Fp<P>& f) {
    HK_UNROLL for (int i = 0; i < P::N; i++) p[i] = f.v[i];
}
template <class P> __device__ __forceinline__ void st_raw(u32* p, const Fp2<P>& f) { st_raw(p, f.c0); st_raw(p + P::N, f.c1); }

// a failing HIP call ends the entry point with MINUS its hipError_t (the product's hk_status values are positive)
#define SHIM_TRY(e) do { hipError_t st_ = (e); if (st_ != hipSuccess) return -(int)st_; } while (0)

namespace {

// what ntt_dev_shim.hip and sublist_dev_shim.hip answer for arguments outside a kernel's contract (nothing is launched);
// above every hk_status
constexpr int SHIM_REFUSED = 1000;

// The device allocations of one call, freed when it returns.  Every byte that does not come from the caller starts as 0xA5:
// no stage may rely on cleared scratch, and an output the kernel does not write is no output.
struct DevBufs {
    std::vector<void*> p;
    ~DevBufs() { for (void* q : p) (void)hipFree(q); }
    // *out: `bytes` of device memory (at least one); its first src_bytes are a copy of `src` when there is one
    template <class T>
    int get(T** out, size_t bytes, const void* src, size_t src_bytes) {
        if (!src) src_bytes = 0;
        if (src_bytes > bytes) return -(int)hipErrorInvalidValue;
        const size_t cap = bytes ? bytes : 1;
        void* q = nullptr;
        SHIM_TRY(hipMalloc(&q, cap));
        p.push_back(q);
        if (src_bytes) SHIM_TRY(hipMemcpy(q, src, src_bytes, hipMemcpyHostToDevice));
        if (src_bytes < cap) SHIM_TRY(hipMemset((char*)q + src_bytes, 0xA5, cap - src_bytes));
        *out = (T*)q;
        return 0;
    }
    template <class T> int get(T** out, size_t bytes, const void* src) { return get(out, bytes, src, bytes); }
};
// SHIM_GET(&ptr, bytes, src[, src_bytes]) on the DevBufs d of the calling function
#define SHIM_GET(...) do { int st_ = d.get(__VA_ARGS__); if (st_) return st_; } while (0)

// the end of a call: the launch status, the kernels' status, then `bytes` from `dev` back to the caller
int finish(void* host, const void* dev, size_t bytes) {
    SHIM_TRY(hipGetLastError());
    SHIM_TRY(hipDeviceSynchronize());
    if (bytes) SHIM_TRY(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

// ---- one translation unit per group --------------------------------------------------------------------------------------
// A shim compiled with -DSHIM_GROUP=0..3 (bn254 G1, bn254 G2, bls12-381 G1, bls12-381 G2, as shim_group_op) sets SHIM_PREFIX
// before it includes this header.  Its per-group functions are SHIM_FN(name), i.e. <prefix>_g<group>_<name> with C++
// linkage inside the library; group 0's unit declares the other three and holds the extern "C" entry points, which reach a
// group's function with SHIM_DISPATCH(group, name(arguments)).
#if defined(SHIM_GROUP)
#include "../../hekaton_system_amd/csrc/hk_internal.h"
#ifndef SHIM_PREFIX
#error "define SHIM_PREFIX before including shim_common.cuh"
#endif
#if SHIM_GROUP == 0
typedef CurveBn254 ShimCurve;
typedef CurveBn254::Fq ShimF;
#elif SHIM_GROUP == 1
typedef CurveBn254 ShimCurve;
typedef CurveBn254::Fq2 ShimF;
#elif SHIM_GROUP == 2
typedef CurveBls381 ShimCurve;
typedef CurveBls381::Fq ShimF;
#elif SHIM_GROUP == 3
typedef CurveBls381 ShimCurve;
typedef CurveBls381::Fq2 ShimF;
#else
#error "compile with -DSHIM_GROUP=0..3"
#endif
typedef ShimCurve::Fr ShimFr;

#define SHIM_CAT_(prefix, g, name) prefix##_g##g##_##name
#define SHIM_CAT(prefix, g, name) SHIM_CAT_(prefix, g, name)
#define SHIM_FN(name) SHIM_CAT(SHIM_PREFIX, SHIM_GROUP, name)
#define SHIM_DISPATCH(group, call)                      \
    switch (group) {                                    \
        case 0: return SHIM_CAT(SHIM_PREFIX, 0, call);  \
        case 1: return SHIM_CAT(SHIM_PREFIX, 1, call);  \
        case 2: return SHIM_CAT(SHIM_PREFIX, 2, call);  \
        case 3: return SHIM_CAT(SHIM_PREFIX, 3, call);  \
    }                                                   \
    return -(int)hipErrorInvalidValue;
#endif
