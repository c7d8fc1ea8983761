// hk_internal.h — context, lanes and scratch arenas shared by the translation units of libhekaton.
#pragma once
#include <hip/hip_runtime.h>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hekaton.h"
#include "../../include/hekaton_gt.h"
#include "coalesce.h"
#include "msm.cuh"
#include "stream_plan.h"

#define HK_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            fprintf(stderr, "[hekaton] HIP error %s at %s:%d: %s\n", hipGetErrorName(_e),    \
                    __FILE__, __LINE__, #expr);                                              \
            return HK_ERR_DEVICE;                                                            \
        }                                                                                    \
    } while (0)

#define HK_TRY(expr)                       \
    do {                                   \
        hk_status _s = (expr);             \
        if (_s != HK_OK) return _s;        \
    } while (0)

#include "launch.h"

namespace hk {

// ---- curve traits -----------------------------------------------------------------------------
struct CurveBn254 {
    typedef Fp<Bn254FrP> Fr;
    typedef Fp<Bn254FqP> Fq;
    typedef Fp2<Bn254FqP> Fq2;
    static constexpr u32 FR_BITS = HK_BN254_FR_BITS;
    static constexpr u32 TWO_ADICITY = HK_BN254_TWO_ADICITY;
    static constexpr u32 ROOT[8] = HK_BN254_FR_ROOT;
    static constexpr u32 GEN[8] = HK_BN254_FR_GEN;
    static constexpr u32 GEN_INV[8] = HK_BN254_FR_GEN_INV;
};
struct CurveBls381 {
    typedef Fp<Bls381FrP> Fr;
    typedef Fp<Bls381FqP> Fq;
    typedef Fp2<Bls381FqP> Fq2;
    static constexpr u32 FR_BITS = HK_BLS12_381_FR_BITS;
    static constexpr u32 TWO_ADICITY = HK_BLS12_381_TWO_ADICITY;
    static constexpr u32 ROOT[8] = HK_BLS12_381_FR_ROOT;
    static constexpr u32 GEN[8] = HK_BLS12_381_FR_GEN;
    static constexpr u32 GEN_INV[8] = HK_BLS12_381_FR_GEN_INV;
};

// scalar field that goes with a coordinate field
template <class F> struct ScalarOf;
template <> struct ScalarOf<CurveBn254::Fq> { typedef CurveBn254::Fr type; };
template <> struct ScalarOf<CurveBn254::Fq2> { typedef CurveBn254::Fr type; };
template <> struct ScalarOf<CurveBls381::Fq> { typedef CurveBls381::Fr type; };
template <> struct ScalarOf<CurveBls381::Fq2> { typedef CurveBls381::Fr type; };

// ---- scratch carving -------------------------------------------------------------------------------------
// A call lists its scratch buffers once, as a function of a Carve, and Lane::carve walks that list twice: without a base the
// cursor only counts bytes, with one it hands out 256-B aligned slices of it.
struct Carve {
    char* base = nullptr;
    size_t off = 0;
    void* take(size_t bytes) {
        size_t o = (off + 255) & ~(size_t)255;
        off = o + bytes;
        return base ? base + o : nullptr;
    }
    template <class T> T* n(size_t count) { return (T*)take(count * sizeof(T)); }
};

// ---- per-call lane: one stream + one grow-only scratch arena ---------------------------------------
// A general lane has one stream.  A prove lane (hk_ctx::prove_lanes) has n_streams: `stream` and side[0 .. n_streams - 2],
// over which prove_batch spreads its five roles (stream_plan.h).
struct Lane {
    hipStream_t stream = nullptr;
    char* arena = nullptr;
    size_t arena_cap = 0;
    hipEvent_t ev[32];
    hipStream_t side[PROVE_MAX_STREAMS - 1] = {};
    unsigned n_streams = 1;
    bool prove = false;
    bool busy = false;
    bool settled = false;         // nothing queued since the last settle(): ~LaneGuard need not drain the streams
    hk_timings timings;
    std::vector<void*> retired;   // outgrown arenas: freed when no call is in flight (hipFree waits for the whole device)
    hk_ctx* owner = nullptr;      // the context the lane belongs to (reserve() may trade arenas with an idle lane of it)

    hk_status reserve(size_t bytes);                 // ensure capacity (may sync + realloc)
    // the call's scratch: fn(Carve&) runs once counting, then - after reserve(total) - once on the arena.  fn only carves
    // (no HIP call, no getenv / is_device_ptr: decide those before and capture the result), and both passes must agree.
    template <class Fn> hk_status carve(Fn&& fn) {
        Carve count;
        fn(count);
        HK_TRY(reserve(count.off));
        Carve real;
        real.base = arena;
        fn(real);
        if (real.off != count.off) {
            fprintf(stderr, "[hekaton] scratch carve is not deterministic (%zu bytes counted, %zu carved)\n", count.off, real.off);
            return HK_ERR_DEVICE;
        }
        settled = false;                             // work on the new slices follows
        return HK_OK;
    }
    hipStream_t stream_at(unsigned i) const { return i ? side[i - 1] : stream; }
    // the call's final synchronize, over every stream of the lane (kernels on any of them use the arena): the lane is idle
    // from here on
    hk_status settle() {
        for (unsigned i = 0; i < n_streams; i++) HK_HIP(hipStreamSynchronize(stream_at(i)));
        settled = true;
        return HK_OK;
    }
};

struct NttTables;   // ntt.hip

// one proof of a prove_batch call: its own assignment (host or device), blinders, kappas and host outputs
struct ProveRow {
    const void* z;                // n_v Fr, Montgomery [h|d]
    const void* r;                // 1 Fr [h]
    const void* s;                // 1 Fr [h]
    const void* kappas;           // n_kappas Fr [h]
    void *a, *b, *c;              // proof.a (G1), proof.b (G2), proof.c (G1) [h]
};

// what the coalescer hands each member of a batch: the batch's status and this proof's share of its timings
struct ProveResult {
    hk_status status;
    hk_timings timings;
    int64_t end_us;               // when the chunk ended (steady clock; HK_PROVE_GATHER_TRACE only, else 0)
};

// how long a leader of hk_prove's coalescer gathers the callers a finished chunk released before it runs a chunk below its
// balanced size (coalesce.h).  Measured in the default bench on MI355X; HK_PROVE_GATHER_US overrides.
enum { PROVE_GATHER_US = 1000 };

// a queued hk_prove call: its row and the lengths it was validated with (those of its key - a leader may run another
// key's calls than its own)
struct ProveCall {
    ProveRow row;
    size_t n_v, n_kappas;
};

// hk_prove's coalescer: at most PROVE_COALESCE_RUNNING coalesced batches of a context run at once
enum { PROVE_COALESCE_RUNNING = 2 };
typedef Coalescer<const hk_pk*, ProveCall, ProveResult> ProveCoalescer;

}  // namespace hk

namespace hk {
// per-curve entry points: each curve's translation unit (hk_<curve>_ops.hip) instantiates Ops<C> (curve_ops_impl.cuh), which
// overrides every one of them.  Grouped by the header that defines them, in the order of Ops<C>'s declarations.
struct CurveOps {
    const size_t fr_bytes, fq_bytes, g1_bytes, g2_bytes, gt_bytes;

    // curve_ops_impl.cuh
    virtual hk_status msm(hk_ctx*, int group, const void* bases, size_t n_bases, const void* scalars,
                          size_t n_scalars, int mont, int checked, void* out) = 0;
    // ntt_host.cuh
    virtual hk_status ntt(hk_ctx*, void* data, unsigned log_m, int inverse, int coset) = 0;
    virtual hk_status witness_map(hk_ctx*, const hk_csr* A, const hk_csr* B, const hk_csr* C, size_t n_inst,
                                  size_t n_c, const void* z, size_t n_v, void* h_out, size_t h_cap, size_t* m_out) = 0;
    virtual void ctx_release(hk_ctx*) = 0;
    // pk.cuh
    virtual hk_status pk_upload(hk_ctx*, const hk_pk_desc*, hk_pk**) = 0;
    virtual void pk_free(hk_pk*) = 0;
    // group_ops.cuh
    virtual hk_status bases_upload(hk_ctx*, int group, const void* bases, size_t n, hk_bases** out) = 0;
    virtual void bases_free(hk_bases*) = 0;
    virtual hk_status msm_bases(hk_ctx*, const hk_bases*, const void* scalars, size_t n_scalars, int mont, int checked,
                                void* out) = 0;
    virtual hk_status fixed_base(hk_ctx*, int group, const void* base, const void* scalars, size_t n, int mont,
                                 void* out) = 0;
    virtual hk_status scalar_pairing(hk_ctx*, int group, const void* points, const void* scalars, size_t n, void* out) = 0;
    virtual hk_status points_lincomb(hk_ctx*, int group, const void* const* vecs, const void* coeffs, size_t k, size_t n,
                                     void* out) = 0;
    virtual hk_status points_fold_many(hk_ctx*, int group, size_t k, const void* const* lo, const void* const* hi,
                                       const void* coeffs, unsigned neg_mask, size_t n, void* const* out) = 0;
    virtual hk_status field_convert(hk_ctx*, int which, const void* in, void* out, size_t n, int to_mont) = 0;
    // witness_host.cuh
    virtual hk_status assignment_from_bits(hk_ctx*, const void* bits, size_t n_v, const uint32_t* full_cols,
                                           const void* full_vals, size_t n_full, void* z_out) = 0;
    virtual hk_status wprog_upload(hk_ctx*, const uint32_t* ops, size_t n_ops, const uint32_t* refs, size_t n_refs,
                                   const uint32_t* map, size_t n_v, size_t n_values, size_t n_inputs, hk_wprog** out) = 0;
    virtual void wprog_free(hk_wprog*) = 0;
    virtual hk_status wprog_run(hk_ctx*, const hk_wprog*, const uint32_t* inputs, size_t batch, const uint32_t* full_cols,
                                const void* full_vals, size_t n_full, void* z_out) = 0;
    virtual hk_status assignment_scatter(hk_ctx*, const uint32_t* full_cols, const void* full_vals, size_t n_full, size_t batch,
                                         size_t n_v, void* z_out) = 0;
    virtual hk_status poseidon_path(hk_ctx*, const void* consts, size_t n_consts, const hk_poseidon_desc* leaf_hash,
                                    const hk_poseidon_desc* node_hash, const void* leaf, const void* siblings,
                                    const uint32_t* index, size_t depth, size_t batch, size_t n_v, size_t col0, void* z_out) = 0;
    // pairing_ops.cuh
    virtual hk_status pairing_products(hk_ctx*, const void* const* lhs, size_t n_lhs, const void* const* rhs, size_t n_rhs,
                                       size_t n, void* out) = 0;
    virtual hk_status pairing_pairs(hk_ctx*, const void* const* lhs, size_t n_lhs, const void* const* rhs, size_t n_rhs,
                                    const uint32_t* pair_lhs, const uint32_t* pair_rhs, size_t n_pairs, size_t n, void* out) = 0;
    virtual hk_status gt_pow(hk_ctx*, const void* gt_in, const void* scalars, size_t n, void* gt_out, int in_gt,
                             size_t group_len) = 0;
    virtual hk_status gt_check(hk_ctx*, const void* fq12_in, size_t n, unsigned char* ok) = 0;
    // prove_impl.cuh
    virtual hk_status commit(hk_ctx*, const hk_pk*, size_t stage, const void* w, size_t n, const void* kappa,
                             void* out) = 0;
    virtual hk_status commit_batch(hk_ctx*, const hk_pk*, size_t stage, const void* w, size_t n, const void* kappas, size_t batch,
                                   void* out) = 0;
    // `batch` proofs of one key, row b from rows[b]; batch == 0 only validates (key, n_v, n_kappas) and touches nothing
    virtual hk_status prove_batch(hk_ctx*, const hk_pk*, size_t n_v, size_t n_kappas, const ProveRow* rows, size_t batch) = 0;
    // verify.cuh
    virtual hk_status vk_prepare(hk_ctx*, const hk_vk_desc*, hk_vk**) = 0;
    virtual void vk_free(hk_vk*) = 0;
    virtual hk_status vk_alpha_beta(const hk_vk*, void*) = 0;
    virtual hk_status verify_batch(hk_ctx*, const hk_vk*, const void* a, const void* b, const void* c, const void* ds,
                                   const void* inputs, size_t n, unsigned flags, const void* rand, unsigned char* verdicts) = 0;
    virtual hk_status points_check(hk_ctx*, int group, const void* pts, size_t n, unsigned char* ok) = 0;
    // keygen.cuh
    virtual hk_status qap_eval(hk_ctx*, const hk_csr* A, const hk_csr* B, const hk_csr* C, size_t n_inst, size_t n_c, size_t n_v,
                               const void* t, void* a, void* b, void* c, void* zt, size_t* m_out) = 0;
    virtual hk_status keygen(hk_ctx*, const hk_keygen_desc*, const hk_keygen_out*, size_t* m_out) = 0;
    // exec_tree.cuh
    virtual hk_status exec_tree(hk_ctx*, const hk_exec_tree_desc*, const hk_exec_tree_out*) = 0;
    // stage1.cuh
    virtual hk_status stage1_witness(hk_ctx*, const hk_stage1_desc*, const uint32_t* sub_index, size_t batch, size_t n_v,
                                     void* z_out) = 0;
    // trace_sort.cuh
    virtual hk_status trace_sort(hk_ctx*, uint32_t entry_fields, const void* time_entries, size_t n_entries, void* addr_entries_out,
                                 uint32_t* perm_out) = 0;
    virtual hk_status stage0_witness(hk_ctx*, const uint32_t* offsets, uint32_t n_sub, uint32_t n_portals, const void* time_entries,
                                     const void* addr_entries, const uint32_t* sub_index, size_t batch, void* w_out) = 0;
    // r1cs_check.cuh
    virtual hk_status r1cs_check(hk_ctx*, const hk_csr* A, const hk_csr* B, const hk_csr* C, const void* z, size_t n_v, size_t batch,
                                 hk_r1cs_verdict* verdicts, uint32_t* bad_rows, void* bad_vals, size_t cap) = 0;
    virtual hk_status pk_r1cs_check(hk_ctx*, const hk_pk*, const void* z, size_t n_v, size_t batch, hk_r1cs_verdict* verdicts,
                                    uint32_t* bad_rows, void* bad_vals, size_t cap) = 0;
    // sha_tree.cuh
    virtual hk_status sha_tree(hk_ctx*, const void* leaves, uint32_t n_sub, uint32_t ns, uint32_t n_portals,
                               const hk_sha_tree_out* out) = 0;
    virtual hk_status sha_tree_inputs(hk_ctx*, const void* leaves, const void* digests, uint32_t n_sub, uint32_t n_inputs,
                                      const uint32_t* sub_index, size_t batch, uint32_t* inputs_out) = 0;

    // ram_witness.cuh
    virtual hk_status ram_stage0_witness(hk_ctx*, const uint32_t* offsets, uint32_t n_sub, uint32_t n_portals,
                                         const void* time_entries, const void* addr_entries, const uint32_t* sub_index,
                                         size_t batch, void* w_out) = 0;
    virtual hk_status ram_stage1_witness(hk_ctx*, const hk_ram_stage1_desc*, const uint32_t* sub_index, size_t batch, size_t n_v,
                                         void* z_out) = 0;
    // r1cs_job.cuh
    virtual hk_status r1cs_job_trace(hk_ctx*, const hk_r1cs_job_desc*, void* time_entries_out) = 0;
    virtual hk_status r1cs_job_witness(hk_ctx*, const hk_r1cs_job_desc*, const uint32_t* sub_index, size_t batch, size_t n_v,
                                       size_t body_col0, void* z_out) = 0;
    // vkd.cuh
    virtual hk_status vkd_trace(hk_ctx*, const hk_vkd_desc*, void* values_out, void* time_entries_out) = 0;
    virtual hk_status vkd_witness(hk_ctx*, const hk_vkd_desc*, const uint32_t* sub_index, size_t batch, size_t n_v,
                                  const hk_vkd_cols* cols, void* z_out) = 0;
    // vkd_tree.cuh
    virtual hk_status vkd_tree(hk_ctx*, const hk_vkd_tree_desc*, void* siblings_out, void* roots_out, uint8_t* status_out) = 0;
    // agg_scalars.cuh
    virtual hk_status scalar_powers(hk_ctx*, const void* x, size_t n, size_t reps, void* out) = 0;
    virtual hk_status ipa_quotient(hk_ctx*, const void* challenges, size_t l, const void* rho, const void* z, size_t shift,
                                   void* q_out) = 0;
    // class_sums.cuh
    virtual hk_status class_power_sums(hk_ctx*, const void* x, const uint32_t* class_of, size_t n, size_t n_classes,
                                       void* sums_out) = 0;
    // point_codec.cuh
    virtual hk_status field_sqrt(hk_ctx*, int which, const void* in, size_t n, void* out, unsigned char* ok) = 0;
    virtual hk_status points_decompress(hk_ctx*, int group, const void* x_canon, const unsigned char* flags, size_t n, int check,
                                        void* points_out, unsigned char* status) = 0;
    virtual hk_status points_compress(hk_ctx*, int group, const void* points, size_t n, void* x_canon_out,
                                      unsigned char* flags_out) = 0;

protected:
    CurveOps(size_t fr, size_t fq, size_t g1, size_t g2, size_t gt)
        : fr_bytes(fr), fq_bytes(fq), g1_bytes(g1), g2_bytes(g2), gt_bytes(gt) {}
    ~CurveOps() = default;
};
CurveOps* curve_ops_bn254();
CurveOps* curve_ops_bls381();
}  // namespace hk

struct hk_ctx {
    hk_curve curve;
    hk::CurveOps* ops = nullptr;
    int device;
    int profiling = 0;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<hk::Lane*> lanes;
    size_t max_lanes = 8;           // concurrent calls beyond this wait for a lane (HK_MAX_LANES)
    // every prove_batch runs on one of these PROVE_COALESCE_RUNNING lanes of prove_streams streams each, created with the
    // context before any general lane (hk_core.hip); their waiters wait on prove_cv
    std::vector<hk::Lane*> prove_lanes;
    unsigned prove_streams = 1;
    std::condition_variable prove_cv;
    hk::NttTables* ntt = nullptr;
    hk_timings last;
    uint32_t max_lanes0 = 262144;   // level-0 accumulate lanes: 4 waves/SIMD x 1024 SIMDs x 64
    void* presize_kernel = nullptr; // k_scratch_presize<W> with the process's deepest frame (hk_core.hip)
    // window tables of hk_fixed_base, kept per base: a trusted setup and the aggregator's SRS multiply the two generators
    // again and again, and a table is a 248-step doubling chain (2 ms in G1, 5 - 6 ms in G2) in front of a 0.6 ms sweep.
    // At most FB_CACHE_MAX entries, never evicted; freed with the context.
    struct FbTable { int group; std::string base; void* table; bool ready; };
    enum { FB_CACHE_MAX = 8 };
    std::vector<FbTable> fb_cache;
    // concurrent hk_prove calls of one key meet here and run as one lock-step batch (hk_core.hip); gather_us: how long a
    // leader waits for the callers a finished chunk released (HK_PROVE_GATHER_US, 0 = no waiting and no balancing)
    hk::ProveCoalescer prove_q;
    explicit hk_ctx(long gather_us)
        : prove_q(hk::PROVE_COALESCE_RUNNING, HK_PROVE_BATCH_CHUNK, hk::ProveResult{HK_ERR_NOMEM, {}, 0}, gather_us) {}
};

struct hk_pk {
    hk::CurveOps* ops;
    hk_ctx* ctx;
    void* impl;
};

struct hk_vk {                     // a prepared verifying key (verify.cuh VkImpl)
    hk::CurveOps* ops;
    hk_ctx* ctx;
    void* impl;
};

struct hk_bases {
    hk::CurveOps* ops;
    hk_ctx* ctx;
    void* impl;
};

namespace hk {
struct WprogImpl {                 // a class's word program on the device (witness.cuh)
    uint32_t *ops = nullptr, *refs = nullptr, *map = nullptr;
    uint32_t n_ops = 0, n_refs = 0, n_values = 0, n_inputs = 0;
    size_t n_v = 0;
};
}  // namespace hk
struct hk_wprog {
    hk::CurveOps* ops;
    hk_ctx* ctx;
    hk::WprogImpl* impl;
};

namespace hk {

struct ProveLaneTag {};
struct LaneGuard {
    hk_ctx* ctx;
    Lane* lane;
    LaneGuard(hk_ctx* c);                  // a general lane
    LaneGuard(hk_ctx* c, ProveLaneTag);    // a prove lane: waits for one of the context's prove lanes to be free
    ~LaneGuard();
};

bool is_device_ptr(const void* p);
static inline hipMemcpyKind h2d_kind(const void* src) {
    return is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
}
static inline float ev_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); return 0.f; }
    return ms;
}

// ---- a call's host-or-device buffers ----------------------------------------------------------
// One record per input or output.  staged(): where the buffer lives is asked ONCE, before the carve - a device-resident or
// absent (NULL) one takes no scratch.  stage_carve() inside the call's carve lambda: p = the buffer itself when it is
// resident, else its slice of scratch.  Kernels read and write p; stage_upload() queues the host inputs' copies in front of
// them, stage_download() the host outputs' copies behind them (before settle()).
struct Staged {
    const void* buf;              // the caller's pointer; NULL: absent
    size_t bytes;
    size_t scratch;               // bytes of lane scratch: `bytes` for a host buffer, 0 for a resident or absent one
    void* p;                      // what the kernels get (after stage_carve)
};
static inline Staged staged(const void* buf, size_t bytes) {
    return {buf, bytes, buf && !is_device_ptr(buf) ? bytes : 0, nullptr};
}
static inline void stage_carve(Carve& c, Staged* s, size_t n) {
    for (size_t k = 0; k < n; k++) {
        void* slice = c.take(s[k].scratch);
        s[k].p = s[k].scratch ? slice : (void*)s[k].buf;
    }
}
static inline hk_status stage_upload(Lane* L, const Staged* s, size_t n) {
    for (size_t k = 0; k < n; k++)
        if (s[k].scratch) HK_HIP(hipMemcpyAsync(s[k].p, s[k].buf, s[k].bytes, hipMemcpyHostToDevice, L->stream));
    return HK_OK;
}
static inline hk_status stage_download(Lane* L, const Staged* s, size_t n) {
    for (size_t k = 0; k < n; k++)
        if (s[k].scratch) HK_HIP(hipMemcpyAsync((void*)s[k].buf, s[k].p, s[k].bytes, hipMemcpyDeviceToHost, L->stream));
    return HK_OK;
}

}  // namespace hk
