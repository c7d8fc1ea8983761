#include <utility>
// hk_core.hip — context / lane management and the C ABI entry points (dispatch to per-curve code).
#include "hk_internal.h"
#include "job_args.h"
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <atomic>

namespace hk {

// ---- scratch budget ------------------------------------------------------------------------
// Measured on MI355X / ROCm 7.2 (tools/scratch_probe.hip, profiles/r03_scratch_probe.txt): a hardware queue that has
// run a kernel with B bytes of private memory per lane keeps a ring of B x 64 lanes x (CUs x 32 wave slots) bytes for
// as long as it lives - 1.49 GiB for the 3056-byte frame of k_msm_reduce_fused<Fp2<Bls381FqP>> - however few waves the
// kernel launches; the rings of all queues share HSA_AMD_AGENT_INFO_SCRATCH_LIMIT_MAX (32 GiB).  Streams map onto at
// most GPU_MAX_HW_QUEUES queues and any of them may end up running the curve's deepest kernel, so the bound that no
// setting of HK_MAX_LANES / HK_SERIAL_STREAMS can break is   queues x ring(deepest frame) + reserve <= limit.
static hsa_status_t scratch_limit_cb(hsa_agent_t a, void* data) {
    hsa_device_type_t type;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &type) != HSA_STATUS_SUCCESS || type != HSA_DEVICE_TYPE_GPU)
        return HSA_STATUS_SUCCESS;
    uint64_t mx = 0;
    if (hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_SCRATCH_LIMIT_MAX, &mx) == HSA_STATUS_SUCCESS && mx) {
        uint64_t* best = (uint64_t*)data;
        if (*best == 0 || mx < *best) *best = mx;
    }
    return HSA_STATUS_SUCCESS;
}
static uint64_t scratch_limit_bytes() {
    static const uint64_t v = [] {
        uint64_t best = 0;
        if (hsa_init() == HSA_STATUS_SUCCESS) {            // reference-counted; HIP holds its own reference
            (void)hsa_iterate_agents(scratch_limit_cb, &best);
            (void)hsa_shut_down();
        }
        return best ? best : (uint64_t)32 << 30;           // what this pool's MI355X report
    }();
    return v;
}
static std::atomic<size_t> g_deepest_frame{0};             // over every context created in this process (a switch may differ)

// Ring pre-sizing.  A queue's ring is re-allocated every time a kernel with a deeper frame than it has seen arrives; rings
// that grow one after another through several sizes fragment the agent's scratch range, and a request can then fail with
// most of the budget free.  Every stream a lane creates therefore first runs one wave of a kernel whose frame is the
// deepest of the process (rounded up to 256 B), in stream-creation = queue order: each ring is allocated once, at its
// final size.  k_scratch_presize<W> owns W * 4 bytes of private memory (runtime-indexed, so it cannot live in registers).
template <int WORDS>
__global__ void __launch_bounds__(64) k_scratch_presize(unsigned* sink, unsigned seed) {
    unsigned buf[WORDS];
    unsigned x = seed + threadIdx.x;
    for (int i = 0; i < WORDS; i += 16) buf[i] = x + i;
    unsigned j = (x * 2654435761u) % (unsigned)WORDS;
    buf[j & ~15u] += x;
    if (sink && buf[(j * 7u) % (unsigned)WORDS & ~15u] == 0x9e3779b9u) *sink = x;     // never true in practice; keeps buf alive
}
typedef void (*presize_fn)(unsigned*, unsigned);
template <int... I> struct PresizeTable { static const presize_fn fn[sizeof...(I)]; };
template <int... I> const presize_fn PresizeTable<I...>::fn[sizeof...(I)] = {k_scratch_presize<64 * (I + 1)>...};
typedef PresizeTable<0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
                     30, 31> Presize;                        // frames of 256 B ... 8 KiB
static presize_fn presize_kernel_for(size_t frame, size_t* actual) {
    size_t idx = frame ? (frame + 255) / 256 - 1 : 0;
    if (idx > 31) idx = 31;
    for (; idx < 32; idx++) {                               // the compiler may add a few bytes: take the first that is deep enough
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, (const void*)Presize::fn[idx]) != hipSuccess) { (void)hipGetLastError(); break; }
        if ((size_t)fa.localSizeBytes >= frame || idx == 31) { *actual = (size_t)fa.localSizeBytes; return Presize::fn[idx]; }
    }
    *actual = frame;
    return nullptr;
}

// the hardware queues the runtime gives the process: GPU_MAX_HW_QUEUES as the host set it, or the HIP runtime's default of 4
static unsigned hw_queues() {
    const char* q = getenv("GPU_MAX_HW_QUEUES");
    return q && atoi(q) > 0 ? (unsigned)atoi(q) : 4u;
}

// ---- the kernels the library launches (launch.h) -------------------------------------------------------------------
// kernel_registry() read once: one row per kernel (the registry holds one per instantiating translation unit), its name cut
// out of kernel_pretty()'s spelling.  A kernel launched both behind a switch and without one is ungated.
struct KernelInfo {
    const void* fn;
    std::string name;
    const char* only_with_env;
};
static const std::vector<KernelInfo>& kernels() {
    static const std::vector<KernelInfo> v = [] {
        std::vector<KernelInfo> out;
        std::map<const void*, size_t> at;
        for (const KernelEntry& e : kernel_registry()) {
            auto it = at.find(e.fn);
            if (it != at.end()) {
                if (!e.only_with_env) out[it->second].only_with_env = nullptr;
                continue;
            }
            // -> "hk::k_name(parameter types)".  This reads clang's spelling of __PRETTY_FUNCTION__; should a compiler spell
            // it otherwise the whole string stays, and tests/test_kernel_registry_cpu.py fails on the names
            std::string name = e.pretty;
            size_t a = name.find("[K = &"), t = name.find(", T = void (*)"), b = name.rfind(']');
            if (a != std::string::npos && t != std::string::npos && b != std::string::npos && a < t && t < b)
                name = name.substr(a + 6, t - a - 6) + name.substr(t + 14, b - t - 14);
            at[e.fn] = out.size();
            out.push_back({e.fn, name, e.only_with_env});
        }
        return out;
    }();
    return v;
}

// private-memory ("scratch") bytes per lane of kernels()[i], as the loaded code object declares them: asked once per process
// (several hundred handles), 0 where the runtime does not answer
static size_t private_bytes_of(size_t i) {
    static const std::vector<size_t> frames = [] {
        std::vector<size_t> f;
        for (const KernelInfo& k : kernels()) {
            hipFuncAttributes fa;
            if (hipFuncGetAttributes(&fa, k.fn) != hipSuccess) { (void)hipGetLastError(); fa.localSizeBytes = 0; }
            f.push_back((size_t)fa.localSizeBytes);
        }
        return f;
    }();
    return frames[i];
}

hk_status scratch_budget_check(const hipDeviceProp_t& prop, void** presize_out) {
    // the deepest frame of EVERY kernel the library launches, whatever the curve of this context: a process that opens a
    // context of the other curve later (the bench's BLS12-381 leg after its BN254 leg) then finds every queue's ring already
    // at its final size - no ring ever grows, and the moment the round-3 experiment aborted in (twenty rings wanted at once
    // while the previous context's were still held) does not arise
    size_t frame = 0;
    const std::vector<KernelInfo>& ks = kernels();
    for (size_t i = 0; i < ks.size(); i++)
        if (!ks[i].only_with_env || getenv(ks[i].only_with_env)) frame = std::max(frame, private_bytes_of(i));
    size_t prev = g_deepest_frame.load();
    while (frame > prev && !g_deepest_frame.compare_exchange_weak(prev, frame)) {}
    frame = g_deepest_frame.load();
    size_t presized = frame;
    *presize_out = (void*)presize_kernel_for(frame, &presized);
    if (presized > frame) frame = presized;                 // the ring every queue will actually hold
    uint64_t queues = hw_queues();
    uint64_t slots = (uint64_t)prop.multiProcessorCount * (uint64_t)(prop.maxThreadsPerMultiProcessor / 64);
    uint64_t ring = (uint64_t)frame * 64 * slots;
    uint64_t limit = scratch_limit_bytes();
    const uint64_t reserve = (uint64_t)1 << 30;                          // other users of the agent (RCCL, torch, rocprofv3)
    if (queues * ring + reserve > limit) {
        uint64_t fit = ring ? (limit - reserve) / ring : queues;
        fprintf(stderr, "[hekaton] scratch budget: %llu hardware queues x %.2f GiB (deepest kernel frame %zu B per lane x 64 x "
                        "%llu wave slots) + 1 GiB reserve exceeds the agent's scratch limit of %.1f GiB; export "
                        "GPU_MAX_HW_QUEUES=%llu or less before the first HIP call%s\n",
                (unsigned long long)queues, ring / 1073741824.0, frame, (unsigned long long)slots, limit / 1073741824.0,
                (unsigned long long)fit, getenv("HK_PAIR_SERIAL") ? " (or unset HK_PAIR_SERIAL: its kernels carry the deepest frames)" : "");
        return HK_ERR_DEVICE;
    }
    return HK_OK;
}

static thread_local hk_timings tl_last_timings = {};

// HK_PROVE_GATHER_TRACE=1 (read once, off by default): one stderr line per hk_prove arrival - how long after the end of the
// chunk that held this thread's previous call it re-entered - and one per chunk end, with the number of arena allocations of
// the process so far.  The figures behind PROVE_GATHER_US.
static bool gather_trace() { static const bool on = getenv("HK_PROVE_GATHER_TRACE") != nullptr; return on; }
static int64_t now_us() {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static std::atomic<unsigned> g_arena_allocs{0};
static thread_local int64_t tl_prev_chunk_end_us = 0;

hk_status Lane::reserve(size_t bytes) {
    if (bytes <= arena_cap) return HK_OK;
    HK_HIP(hipStreamSynchronize(stream));
    if (owner) {
        // an idle lane of the context may hold an arena that is large enough (an earlier call of this size ran there):
        // trade arenas with it - the smallest that fits - instead of allocating (a hipMalloc of tens of MB takes
        // milliseconds, and which lane a call lands on is arbitrary).  An idle lane's streams have nothing in flight:
        // ~LaneGuard drains them before it marks a lane free.
        // (within its own kind: a prove lane's arena stays with the prove lanes, which reuse it chunk after chunk)
        std::lock_guard<std::mutex> lk(owner->mu);
        Lane* best = nullptr;
        for (Lane* l : prove ? owner->prove_lanes : owner->lanes)
            if (l != this && !l->busy && l->arena_cap >= bytes && (!best || l->arena_cap < best->arena_cap)) best = l;
        if (best) {
            std::swap(arena, best->arena);
            std::swap(arena_cap, best->arena_cap);
            return HK_OK;
        }
    }
    if (arena) retired.push_back(arena);          // not hipFree here: it would wait for every other lane's kernels
    arena = nullptr;
    arena_cap = 0;
    size_t want = bytes + bytes / 8 + (1u << 20);
    g_arena_allocs++;
    hipError_t e = hipMalloc((void**)&arena, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fprintf(stderr, "[hekaton] scratch allocation of %zu bytes failed: %s\n", want, hipGetErrorName(e));
        return HK_ERR_NOMEM;
    }
    arena_cap = want;
    return HK_OK;
}

// A new lane with n streams (its events, its streams, each stream's scratch ring pre-sized); nullptr when the runtime
// refuses a stream or an event: a half-built lane would run on the legacy default stream / null events.
static Lane* new_lane(hk_ctx* ctx, unsigned n, bool prove) {
    Lane* l = new Lane();
    (void)hipSetDevice(ctx->device);
    for (auto& e : l->ev) e = nullptr;
    l->n_streams = n;
    l->prove = prove;
    bool ok = true;
    for (auto& e : l->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    for (unsigned i = 0; i < n; i++)
        ok = ok && hipStreamCreateWithFlags(i ? &l->side[i - 1] : &l->stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        fprintf(stderr, "[hekaton] could not create the streams / events of a lane\n");
        for (auto& e : l->ev) if (e) (void)hipEventDestroy(e);
        for (unsigned i = 0; i < n; i++) if (l->stream_at(i)) (void)hipStreamDestroy(l->stream_at(i));
        delete l;
        return nullptr;
    }
    if (ctx->presize_kernel && !getenv("HK_NO_SCRATCH_PRESIZE")) {
        // one wave of the deepest frame on each of the lane's streams, in creation order (see k_scratch_presize).  A raw
        // launch, the only one: this kernel IS the ring sizing, so it must not count towards the frame it is chosen from
        presize_fn k = (presize_fn)ctx->presize_kernel;
        for (unsigned i = 0; i < n; i++) hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, l->stream_at(i), (unsigned*)nullptr, 1u);
        bool okp = true;
        for (unsigned i = 0; i < n; i++) okp = okp && hipStreamSynchronize(l->stream_at(i)) == hipSuccess;
        if (!okp) { (void)hipGetLastError(); fprintf(stderr, "[hekaton] scratch pre-sizing of a lane failed\n"); }
    }
    memset(&l->timings, 0, sizeof(l->timings));
    l->owner = ctx;
    return l;
}

static void free_lane(Lane* l) {
    if (l->arena) (void)hipFree(l->arena);
    for (void* p : l->retired) (void)hipFree(p);
    for (auto& e : l->ev) (void)hipEventDestroy(e);
    for (unsigned i = 0; i < l->n_streams; i++) (void)hipStreamDestroy(l->stream_at(i));
    delete l;
}

LaneGuard::LaneGuard(hk_ctx* c) : ctx(c), lane(nullptr) {
    std::unique_lock<std::mutex> lk(ctx->mu);
    for (;;) {
        // among the free lanes the one with the largest scratch arena: a lane that has to grow its arena frees the old one,
        // and hipFree waits for the whole device - with calls of mixed sizes side by side (the aggregator: 6 ms pairing
        // calls beside 1 ms folds) a big call on a small lane stalled everything for milliseconds
        for (Lane* l : ctx->lanes)
            if (!l->busy && (!lane || l->arena_cap > lane->arena_cap)) lane = l;
        if (lane) break;
        if (ctx->lanes.size() < ctx->max_lanes) {
            // one stream: the runtime hands it the least-used hardware queue.  Lanes stay lazily created, one by one.
            lane = new_lane(ctx, 1, false);
            if (lane) ctx->lanes.push_back(lane);
            break;
        }
        ctx->cv.wait(lk);
    }
    if (lane) { lane->busy = true; lane->settled = false; lane->owner = ctx; }
    lk.unlock();
    (void)hipSetDevice(ctx->device);
}

LaneGuard::LaneGuard(hk_ctx* c, ProveLaneTag) : ctx(c), lane(nullptr) {
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (ctx->prove_lanes.empty()) return;              // hk_ctx_create made them; none means it could not
    for (;;) {
        for (Lane* l : ctx->prove_lanes)
            if (!l->busy && (!lane || l->arena_cap > lane->arena_cap)) lane = l;
        if (lane) break;
        ctx->prove_cv.wait(lk);
    }
    lane->busy = true;
    lane->settled = false;
    lk.unlock();
    (void)hipSetDevice(ctx->device);
}

LaneGuard::~LaneGuard() {
    if (!lane) return;
    if (!lane->settled) {
        // an error return (HK_TRY / HK_HIP) may leave kernels queued on the arena, on any of the lane's streams: another
        // call may take this lane, or trade arenas with it in reserve(), once it is free
        for (unsigned i = 0; i < lane->n_streams; i++) (void)hipStreamSynchronize(lane->stream_at(i));
    }
    std::unique_lock<std::mutex> lk(ctx->mu);
    lane->busy = false;
    ctx->last = lane->timings;
    tl_last_timings = lane->timings;
    bool idle = true;
    for (Lane* l : ctx->lanes) idle = idle && !l->busy;
    for (Lane* l : ctx->prove_lanes) idle = idle && !l->busy;
    if (idle)                                      // nothing of this context is on the GPU: outgrown arenas go now
        for (auto* v : {&ctx->lanes, &ctx->prove_lanes})
            for (Lane* l : *v) {
                if (l->retired.empty()) continue;
                (void)hipSetDevice(ctx->device);
                for (void* p : l->retired) (void)hipFree(p);
                l->retired.clear();
            }
    const bool prove = lane->prove;
    lk.unlock();
    if (prove) ctx->prove_cv.notify_one();
    else ctx->cv.notify_one();
}

bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

}  // namespace hk

using namespace hk;

extern "C" {

const char* hk_status_str(hk_status s) {
    switch (s) {
        case HK_OK: return "HK_OK";
        case HK_ERR_LEN: return "HK_ERR_LEN";
        case HK_ERR_DOMAIN_TOO_LARGE: return "HK_ERR_DOMAIN_TOO_LARGE";
        case HK_ERR_DEVICE: return "HK_ERR_DEVICE";
        case HK_ERR_ARG: return "HK_ERR_ARG";
        case HK_ERR_NOMEM: return "HK_ERR_NOMEM";
    }
    return "HK_ERR_UNKNOWN";
}

const char* hk_version(void) { return "hekaton-mi355x 0.1 (gfx950)"; }

hk_status hk_kernel_info(size_t i, const char** name, size_t* private_bytes, const char** only_with_env) {
    const std::vector<hk::KernelInfo>& ks = hk::kernels();
    if (i >= ks.size()) return HK_ERR_ARG;
    if (name) *name = ks[i].name.c_str();
    if (only_with_env) *only_with_env = ks[i].only_with_env;
    if (private_bytes) *private_bytes = hk::private_bytes_of(i);
    return HK_OK;
}

hk_status hk_ctx_create(hk_curve curve, int device_id, hk_ctx** out) {
    if (!out) return HK_ERR_ARG;
    *out = nullptr;
    if (curve != HK_BN254 && curve != HK_BLS12_381) return HK_ERR_ARG;
    // The library plans its streams within the hardware queues the process has (GPU_MAX_HW_QUEUES as the host set it
    // before its first HIP call, or the runtime's default of 4) and does NOT touch the process environment (setenv is
    // not safe against another thread's getenv in a multi-threaded host): DESIGN.md section 5, INTEGRATION.md section 3.
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        fprintf(stderr, "[hekaton] no HIP device: this library has no CPU path\n");
        return HK_ERR_DEVICE;
    }
    if (device_id < 0 || device_id >= n) return HK_ERR_DEVICE;
    HK_HIP(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HK_HIP(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "[hekaton] device %d is %s; kernels are built for gfx950 only\n", device_id,
                prop.gcnArchName);
        return HK_ERR_DEVICE;
    }
    hk::CurveOps* ops = curve == HK_BN254 ? curve_ops_bn254() : curve_ops_bls381();
    // no environment setting may be able to exhaust the runtime's scratch pool (the abort of round 2): refuse here
    void* presize = nullptr;
    HK_TRY(hk::scratch_budget_check(prop, &presize));
    // read once per context, before any thread can be inside hk_prove
    const char* gu = getenv("HK_PROVE_GATHER_US");
    hk_ctx* c = new hk_ctx(gu ? atol(gu) : (long)hk::PROVE_GATHER_US);
    c->presize_kernel = presize;
    c->curve = curve;
    c->device = device_id;
    c->ops = ops;
    memset(&c->last, 0, sizeof(c->last));
    const char* ml = getenv("HK_MAX_LANES");
    if (ml && atoi(ml) > 0) c->max_lanes = (size_t)atoi(ml);
    // the prove lanes, before any general lane of the context: PROVE_COALESCE_RUNNING lanes of s = Q / K streams (at most
    // five, the roles of a chunk), created in a row so that the runtime's least-used assignment gives each stream its own
    // hardware queue while the Q queues go round.  HK_SERIAL_STREAMS=1: one stream per prove lane.
    c->prove_streams = getenv("HK_SERIAL_STREAMS") ? 1u : hk::prove_lane_streams(hw_queues(), hk::PROVE_COALESCE_RUNNING);
    for (int i = 0; i < hk::PROVE_COALESCE_RUNNING; i++) {
        hk::Lane* l = new_lane(c, c->prove_streams, true);
        if (!l) {
            for (hk::Lane* p : c->prove_lanes) free_lane(p);
            delete c;
            return HK_ERR_DEVICE;
        }
        c->prove_lanes.push_back(l);
    }
    *out = c;
    return HK_OK;
}

void hk_ctx_destroy(hk_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    if (ctx->ops) ctx->ops->ctx_release(ctx);
    for (Lane* l : ctx->lanes) free_lane(l);
    for (Lane* l : ctx->prove_lanes) free_lane(l);
    delete ctx;
}

hk_status hk_ctx_sync(hk_ctx* ctx) {
    if (!ctx) return HK_ERR_ARG;
    HK_HIP(hipSetDevice(ctx->device));
    std::unique_lock<std::mutex> lk(ctx->mu);
    for (auto* v : {&ctx->lanes, &ctx->prove_lanes})
        for (Lane* l : *v)
            for (unsigned i = 0; i < l->n_streams; i++) HK_HIP(hipStreamSynchronize(l->stream_at(i)));
    return HK_OK;
}

hk_status hk_ctx_set_profiling(hk_ctx* ctx, int enable) {
    if (!ctx) return HK_ERR_ARG;
    ctx->profiling = enable;
    return HK_OK;
}

hk_status hk_ctx_last_timings(hk_ctx* ctx, hk_timings* out) {
    if (!ctx || !out) return HK_ERR_ARG;
    *out = hk::tl_last_timings;        // timings of the calling thread's most recent call
    return HK_OK;
}

hk_status hk_ctx_sizes(const hk_ctx* ctx, size_t* fr, size_t* fq, size_t* g1, size_t* g2) {
    if (!ctx) return HK_ERR_ARG;
    if (fr) *fr = ctx->ops->fr_bytes;
    if (fq) *fq = ctx->ops->fq_bytes;
    if (g1) *g1 = ctx->ops->g1_bytes;
    if (g2) *g2 = ctx->ops->g2_bytes;
    return HK_OK;
}

hk_status hk_dev_alloc(hk_ctx* ctx, size_t bytes, void** dptr) {
    if (!ctx || !dptr) return HK_ERR_ARG;
    HK_HIP(hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
    if (e != hipSuccess) { (void)hipGetLastError(); return HK_ERR_NOMEM; }
    return HK_OK;
}
hk_status hk_dev_free(hk_ctx* ctx, void* dptr) {
    if (!ctx) return HK_ERR_ARG;
    HK_HIP(hipSetDevice(ctx->device));
    HK_HIP(hipFree(dptr));
    return HK_OK;
}
hk_status hk_dev_upload(hk_ctx* ctx, void* dst_d, const void* src_h, size_t bytes) {
    if (!ctx) return HK_ERR_ARG;
    HK_HIP(hipSetDevice(ctx->device));
    HK_HIP(hipMemcpy(dst_d, src_h, bytes, hipMemcpyHostToDevice));
    return HK_OK;
}
hk_status hk_dev_download(hk_ctx* ctx, void* dst_h, const void* src_d, size_t bytes) {
    if (!ctx) return HK_ERR_ARG;
    HK_HIP(hipSetDevice(ctx->device));
    HK_HIP(hipMemcpy(dst_h, src_d, bytes, hipMemcpyDeviceToHost));
    return HK_OK;
}

hk_status hk_msm_g1(hk_ctx* ctx, const void* bases, size_t n_bases, const void* scalars, size_t n_scalars,
                    int mont, int checked, void* out) {
    if (!ctx || !out) return HK_ERR_ARG;
    return ctx->ops->msm(ctx, 1, bases, n_bases, scalars, n_scalars, mont, checked, out);
}
hk_status hk_msm_g2(hk_ctx* ctx, const void* bases, size_t n_bases, const void* scalars, size_t n_scalars,
                    int mont, int checked, void* out) {
    if (!ctx || !out) return HK_ERR_ARG;
    return ctx->ops->msm(ctx, 2, bases, n_bases, scalars, n_scalars, mont, checked, out);
}
hk_status hk_fixed_base_g1(hk_ctx* ctx, const void* base, const void* scalars, size_t n, int mont, void* out) {
    if (!ctx || !base || (n && (!scalars || !out))) return HK_ERR_ARG;
    return ctx->ops->fixed_base(ctx, 1, base, scalars, n, mont, out);
}
hk_status hk_fixed_base_g2(hk_ctx* ctx, const void* base, const void* scalars, size_t n, int mont, void* out) {
    if (!ctx || !base || (n && (!scalars || !out))) return HK_ERR_ARG;
    return ctx->ops->fixed_base(ctx, 2, base, scalars, n, mont, out);
}
hk_status hk_scalar_pairing_g1(hk_ctx* ctx, const void* points, const void* scalars, size_t n, void* out) {
    if (!ctx || (n && (!points || !scalars || !out))) return HK_ERR_ARG;
    return ctx->ops->scalar_pairing(ctx, 1, points, scalars, n, out);
}
hk_status hk_scalar_pairing_g2(hk_ctx* ctx, const void* points, const void* scalars, size_t n, void* out) {
    if (!ctx || (n && (!points || !scalars || !out))) return HK_ERR_ARG;
    return ctx->ops->scalar_pairing(ctx, 2, points, scalars, n, out);
}
hk_status hk_bases_upload(hk_ctx* ctx, int group, const void* bases, size_t n, hk_bases** out) {
    if (!ctx || !out || (group != 1 && group != 2) || (n && !bases)) return HK_ERR_ARG;
    return ctx->ops->bases_upload(ctx, group, bases, n, out);
}
void hk_bases_free(hk_bases* b) {
    if (b) b->ops->bases_free(b);
}
hk_status hk_msm_bases(hk_ctx* ctx, const hk_bases* b, const void* scalars, size_t n_scalars, int mont, int checked,
                       void* out) {
    if (!ctx || !b || !out || b->ctx != ctx) return HK_ERR_ARG;
    return ctx->ops->msm_bases(ctx, b, scalars, n_scalars, mont, checked, out);
}
hk_status hk_wprog_upload(hk_ctx* ctx, const uint32_t* ops, size_t n_ops, const uint32_t* refs, size_t n_refs,
                          const uint32_t* map, size_t n_v, size_t n_values, size_t n_inputs, hk_wprog** out) {
    if (!ctx || !ops || !map || !out || (n_refs && !refs)) return HK_ERR_ARG;
    return ctx->ops->wprog_upload(ctx, ops, n_ops, refs, n_refs, map, n_v, n_values, n_inputs, out);
}
void hk_wprog_free(hk_wprog* w) {
    if (w) w->ops->wprog_free(w);
}
hk_status hk_poseidon_path(hk_ctx* ctx, const void* consts_mont, size_t n_consts, const hk_poseidon_desc* leaf_hash,
                           const hk_poseidon_desc* node_hash, const void* leaf_mont, const void* siblings_mont,
                           const uint32_t* leaf_index, size_t depth, size_t batch, size_t n_v, size_t col0, void* z_out) {
    if (!ctx) return HK_ERR_ARG;
    return ctx->ops->poseidon_path(ctx, consts_mont, n_consts, leaf_hash, node_hash, leaf_mont, siblings_mont, leaf_index,
                                   depth, batch, n_v, col0, z_out);
}
hk_status hk_wprog_run(hk_ctx* ctx, const hk_wprog* w, const uint32_t* inputs, size_t batch, const uint32_t* full_cols,
                       const void* full_vals_mont, size_t n_full, void* z_out) {
    if (!ctx || !w || w->ctx != ctx || !z_out || (batch && !inputs) || (n_full && (!full_cols || !full_vals_mont))) return HK_ERR_ARG;
    return ctx->ops->wprog_run(ctx, w, inputs, batch, full_cols, full_vals_mont, n_full, z_out);
}
hk_status hk_assignment_scatter(hk_ctx* ctx, const uint32_t* full_cols, const void* full_vals_mont, size_t n_full, size_t batch,
                                size_t n_v, void* z_out) {
    if (!ctx || !z_out || (n_full && batch && (!full_cols || !full_vals_mont))) return HK_ERR_ARG;
    return ctx->ops->assignment_scatter(ctx, full_cols, full_vals_mont, n_full, batch, n_v, z_out);
}
hk_status hk_assignment_from_bits(hk_ctx* ctx, const void* bits, size_t n_v, const uint32_t* full_cols,
                                  const void* full_vals_mont, size_t n_full, void* z_out) {
    if (!ctx || !z_out || (n_v && !bits) || (n_full && (!full_cols || !full_vals_mont))) return HK_ERR_ARG;
    return ctx->ops->assignment_from_bits(ctx, bits, n_v, full_cols, full_vals_mont, n_full, z_out);
}
hk_status hk_gt_pow(hk_ctx* ctx, const void* gt_in, const void* scalars_mont, size_t n, void* gt_out) {
    if (!ctx || (n && (!gt_in || !scalars_mont || !gt_out))) return HK_ERR_ARG;
    return ctx->ops->gt_pow(ctx, gt_in, scalars_mont, n, gt_out, 1, 1);
}
hk_status hk_fq12_pow(hk_ctx* ctx, const void* gt_in, const void* scalars_mont, size_t n, void* gt_out) {
    if (!ctx || (n && (!gt_in || !scalars_mont || !gt_out))) return HK_ERR_ARG;
    return ctx->ops->gt_pow(ctx, gt_in, scalars_mont, n, gt_out, 0, 1);
}
hk_status hk_gt_pow_prod(hk_ctx* ctx, const void* gt_in, const void* scalars_mont, size_t n, size_t group_len, int in_gt,
                         void* gt_out) {
    if (!ctx || group_len == 0 || (n && (!gt_in || !scalars_mont || !gt_out))) return HK_ERR_ARG;
    return ctx->ops->gt_pow(ctx, gt_in, scalars_mont, n, gt_out, in_gt ? 1 : 0, group_len);
}
hk_status hk_points_lincomb_g1(hk_ctx* ctx, const void* const* vecs, const void* coeffs_mont, size_t k, size_t n, void* out) {
    if (!ctx || !vecs || !coeffs_mont || (n && !out)) return HK_ERR_ARG;
    return ctx->ops->points_lincomb(ctx, 1, vecs, coeffs_mont, k, n, out);
}
hk_status hk_points_lincomb_g2(hk_ctx* ctx, const void* const* vecs, const void* coeffs_mont, size_t k, size_t n, void* out) {
    if (!ctx || !vecs || !coeffs_mont || (n && !out)) return HK_ERR_ARG;
    return ctx->ops->points_lincomb(ctx, 2, vecs, coeffs_mont, k, n, out);
}
// out[i] = lo[i] + (+-) coeffs2[0] * hi[i] + (+-) coeffs2[1] * phi(hi[i]) in G1: the G1 fold lo + c * hi with c split along the
// GLV endomorphism phi(x, y) = (BETA x, y) into two ~128-bit parts on the host (128 doubling steps instead of 254)
hk_status hk_points_fold_g1(hk_ctx* ctx, const void* lo, const void* hi, const void* coeffs2_mont, unsigned neg_mask, size_t n,
                            void* out) {
    if (!ctx || !ctx->ops) return HK_ERR_ARG;
    return ctx->ops->points_fold_many(ctx, 1, 1, &lo, &hi, coeffs2_mont, neg_mask, n, &out);
}
// out[i] = lo[i] + sum_{j<4} (+-) coeffs4[j] * psi^j(hi[i]) in G2: the fold lo + c * hi of a TIPA round with c split into
// four ~64-bit parts on the host (c = sum +-coeffs4[j] lambda^j mod r, lambda = psi's eigenvalue), so the shared doubling
// chain of the element-wise combination is ~66 steps instead of 254; one table add per step (endo.cuh)
hk_status hk_points_fold_g2(hk_ctx* ctx, const void* lo, const void* hi, const void* coeffs4_mont, unsigned neg_mask, size_t n,
                            void* out) {
    if (!ctx || !ctx->ops) return HK_ERR_ARG;
    return ctx->ops->points_fold_many(ctx, 2, 1, &lo, &hi, coeffs4_mont, neg_mask, n, &out);
}
hk_status hk_points_fold_many_g1(hk_ctx* ctx, size_t k, const void* const* lo, const void* const* hi, const void* coeffs2_mont,
                                 unsigned neg_mask, size_t n, void* const* out) {
    if (!ctx || !ctx->ops) return HK_ERR_ARG;
    return ctx->ops->points_fold_many(ctx, 1, k, lo, hi, coeffs2_mont, neg_mask, n, out);
}
hk_status hk_points_fold_many_g2(hk_ctx* ctx, size_t k, const void* const* lo, const void* const* hi, const void* coeffs4_mont,
                                 unsigned neg_mask, size_t n, void* const* out) {
    if (!ctx || !ctx->ops) return HK_ERR_ARG;
    return ctx->ops->points_fold_many(ctx, 2, k, lo, hi, coeffs4_mont, neg_mask, n, out);
}
hk_status hk_pairing_pairs(hk_ctx* ctx, const void* const* lhs_g1, size_t n_lhs, const void* const* rhs_g2, size_t n_rhs,
                           const uint32_t* pair_lhs, const uint32_t* pair_rhs, size_t n_pairs, size_t n, void* gt_out) {
    if (!ctx || !lhs_g1 || !rhs_g2 || !pair_lhs || !pair_rhs || !gt_out) return HK_ERR_ARG;
    return ctx->ops->pairing_pairs(ctx, lhs_g1, n_lhs, rhs_g2, n_rhs, pair_lhs, pair_rhs, n_pairs, n, gt_out);
}
hk_status hk_pairing_products(hk_ctx* ctx, const void* const* lhs_g1, size_t n_lhs, const void* const* rhs_g2,
                              size_t n_rhs, size_t n, void* gt_out) {
    if (!ctx || !lhs_g1 || !rhs_g2 || !gt_out) return HK_ERR_ARG;
    return ctx->ops->pairing_products(ctx, lhs_g1, n_lhs, rhs_g2, n_rhs, n, gt_out);
}
hk_status hk_multi_pairing(hk_ctx* ctx, const void* g1, const void* g2, size_t n, void* gt_out) {
    if (!ctx || !gt_out || (n && (!g1 || !g2))) return HK_ERR_ARG;
    const void* l[1] = {n ? g1 : (const void*)gt_out};
    const void* r[1] = {n ? g2 : (const void*)gt_out};
    return ctx->ops->pairing_products(ctx, l, 1, r, 1, n, gt_out);
}
hk_status hk_vk_prepare(hk_ctx* ctx, const hk_vk_desc* desc, hk_vk** out) {
    if (!ctx || !desc || !out) return HK_ERR_ARG;
    return ctx->ops->vk_prepare(ctx, desc, out);
}
void hk_vk_free(hk_vk* vk) {
    if (vk) vk->ops->vk_free(vk);
}
hk_status hk_vk_alpha_beta(const hk_vk* vk, void* gt_out) {
    if (!vk || !gt_out) return HK_ERR_ARG;
    return vk->ops->vk_alpha_beta(vk, gt_out);
}
hk_status hk_verify_batch(hk_ctx* ctx, const hk_vk* vk, const void* a_g1, const void* b_g2, const void* c_g1, const void* ds_g1,
                          const void* inputs_mont, size_t n, unsigned flags, const void* rand_mont, uint8_t* verdicts) {
    if (!ctx || !vk || vk->ctx != ctx) return HK_ERR_ARG;
    return ctx->ops->verify_batch(ctx, vk, a_g1, b_g2, c_g1, ds_g1, inputs_mont, n, flags, rand_mont, verdicts);
}
hk_status hk_points_check_g1(hk_ctx* ctx, const void* points, size_t n, uint8_t* ok) {
    if (!ctx || (n && (!points || !ok))) return HK_ERR_ARG;
    return ctx->ops->points_check(ctx, 1, points, n, ok);
}
hk_status hk_points_check_g2(hk_ctx* ctx, const void* points, size_t n, uint8_t* ok) {
    if (!ctx || (n && (!points || !ok))) return HK_ERR_ARG;
    return ctx->ops->points_check(ctx, 2, points, n, ok);
}
hk_status hk_gt_check(hk_ctx* ctx, const void* fq12_in, size_t n, uint8_t* ok) {          // include/hekaton_gt.h
    if (!ctx || (n && (!fq12_in || !ok))) return HK_ERR_ARG;
    return ctx->ops->gt_check(ctx, fq12_in, n, ok);
}
hk_status hk_ctx_gt_bytes(const hk_ctx* ctx, size_t* gt) {
    if (!ctx || !gt) return HK_ERR_ARG;
    *gt = ctx->ops->gt_bytes;
    return HK_OK;
}
hk_status hk_field_convert(hk_ctx* ctx, int which, const void* in, void* out, size_t n, int to_mont) {
    if (!ctx || (which != 0 && which != 1) || (n && (!in || !out))) return HK_ERR_ARG;
    return ctx->ops->field_convert(ctx, which, in, out, n, to_mont);
}
hk_status hk_ntt(hk_ctx* ctx, void* data, unsigned log_m, int inverse, int coset) {
    if (!ctx || !data) return HK_ERR_ARG;
    return ctx->ops->ntt(ctx, data, log_m, inverse, coset);
}
hk_status hk_witness_map(hk_ctx* ctx, const hk_csr* A, const hk_csr* B, const hk_csr* C, size_t n_inst,
                         size_t n_constraints, const void* z_mont, size_t n_v, void* h_out,
                         size_t h_capacity, size_t* m_out) {
    if (!ctx || !A || !B || !C || !z_mont || !h_out) return HK_ERR_ARG;
    return ctx->ops->witness_map(ctx, A, B, C, n_inst, n_constraints, z_mont, n_v, h_out, h_capacity, m_out);
}
hk_status hk_pk_upload(hk_ctx* ctx, const hk_pk_desc* desc, hk_pk** out) {
    if (!ctx || !desc || !out) return HK_ERR_ARG;
    return ctx->ops->pk_upload(ctx, desc, out);
}
void hk_pk_free(hk_pk* pk) {
    if (!pk) return;
    pk->ops->pk_free(pk);
}
hk_status hk_commit(hk_ctx* ctx, const hk_pk* pk, size_t stage, const void* w, size_t n, const void* kappa,
                    void* out) {
    if (!ctx || !pk || !kappa || !out) return HK_ERR_ARG;
    return ctx->ops->commit(ctx, pk, stage, w, n, kappa, out);
}
hk_status hk_commit_batch(hk_ctx* ctx, const hk_pk* pk, size_t stage, const void* w, size_t n, const void* kappas, size_t batch,
                          void* out) {
    if (!ctx || !pk || (batch && (!kappas || !out))) return HK_ERR_ARG;
    return ctx->ops->commit_batch(ctx, pk, stage, w, n, kappas, batch, out);
}
hk_status hk_prove(hk_ctx* ctx, const hk_pk* pk, const void* z, size_t n_v, const void* r, const void* s,
                   const void* kappas, size_t n_kappas, void* a, void* b, void* c) {
    if (!ctx || !pk || !z || !r || !s || !a || !b || !c) return HK_ERR_ARG;
    // a bad call fails on its own thread and never joins a batch: key and lengths (a batch of none only validates), kappas
    HK_TRY(ctx->ops->prove_batch(ctx, pk, n_v, n_kappas, nullptr, 0));
    if (n_kappas && !kappas) return HK_ERR_ARG;
    // concurrent calls of this key meet in the context's coalescer and run as one lock-step batch;
    // a lone call leads at once, a batch of one
    const hk::ProveCall call = {{z, r, s, kappas, a, b, c}, n_v, n_kappas};
    if (hk::gather_trace() && hk::tl_prev_chunk_end_us)
        fprintf(stderr, "[hekaton] gather arrive gap_us=%lld\n", (long long)(hk::now_us() - hk::tl_prev_chunk_end_us));
    hk::ProveResult res = ctx->prove_q.submit(pk, call, [&](const hk_pk* key, hk::ProveCoalescer::Member* const* ms, size_t n) {
        std::vector<hk::ProveRow> rows(n);
        for (size_t i = 0; i < n; i++) rows[i] = ms[i]->item->row;
        // the key's lengths, from its own calls: the leader's n_v / n_kappas belong to the leader's key
        hk_status st = ctx->ops->prove_batch(ctx, key, ms[0]->item->n_v, ms[0]->item->n_kappas, rows.data(), n);
        // every member's share of the chunk: each *_ms figure over the chunk's proofs, four accumulate launches as for
        // one proof (bench.py and the roofline divide per-proof bytes by accum_kernel_ms / accum_kernel_launches)
        hk_timings t = tl_last_timings;      // the lane's timings, published by prove_batch's LaneGuard on this thread
        const float f = 1.0f / (float)n;
        for (float* x : {&t.total_ms, &t.digits_ms, &t.msm_a_ms, &t.msm_b_g1_ms, &t.msm_b_g2_ms, &t.msm_l_ms, &t.witness_map_ms,
                         &t.msm_h_ms, &t.finish_ms, &t.accum_kernel_ms, &t.accum_h_ms, &t.keygen_qap_ms, &t.keygen_scalars_ms,
                         &t.keygen_sweeps_ms})
            *x *= f;
        if (t.accum_kernel_launches) t.accum_kernel_launches = 4;
        t.batch_proofs = (uint32_t)n;
        int64_t end_us = 0;
        if (hk::gather_trace()) {
            end_us = hk::now_us();
            fprintf(stderr, "[hekaton] gather chunk n=%zu arena_allocs=%u\n", n, hk::g_arena_allocs.load());
        }
        for (size_t i = 0; i < n; i++) ms[i]->result = hk::ProveResult{st, t, end_us};
    });
    hk::tl_prev_chunk_end_us = res.end_us;
    tl_last_timings = res.timings;
    return res.status;
}
hk_status hk_prove_batch(hk_ctx* ctx, const hk_pk* pk, const void* z, size_t n_v, const void* r, const void* s,
                         const void* kappas, size_t n_kappas, size_t batch, void* a, void* b, void* c) {
    if (!ctx || !pk) return HK_ERR_ARG;
    HK_TRY(ctx->ops->prove_batch(ctx, pk, n_v, n_kappas, nullptr, 0));      // key and lengths first, as documented
    if (batch == 0) return HK_OK;
    if (!z || !r || !s || !a || !b || !c || (n_kappas && !kappas)) return HK_ERR_ARG;
    // row b of the arrays, row after row
    const size_t fr = ctx->ops->fr_bytes, g1 = ctx->ops->g1_bytes, g2 = ctx->ops->g2_bytes;
    std::vector<hk::ProveRow> rows(batch);
    for (size_t i = 0; i < batch; i++)
        rows[i] = {(const char*)z + i * n_v * fr, (const char*)r + i * fr, (const char*)s + i * fr,
                   n_kappas ? (const char*)kappas + i * n_kappas * fr : nullptr, (char*)a + i * g1, (char*)b + i * g2,
                   (char*)c + i * g1};
    return ctx->ops->prove_batch(ctx, pk, n_v, n_kappas, rows.data(), batch);
}

hk_status hk_qap_eval(hk_ctx* ctx, const hk_csr* A, const hk_csr* B, const hk_csr* C, size_t n_inst, size_t n_constraints,
                      size_t n_v, const void* t, void* a, void* b, void* c, void* zt, size_t* m_out) {
    if (!ctx) return HK_ERR_ARG;
    return ctx->ops->qap_eval(ctx, A, B, C, n_inst, n_constraints, n_v, t, a, b, c, zt, m_out);
}
hk_status hk_keygen(hk_ctx* ctx, const hk_keygen_desc* desc, const hk_keygen_out* out, size_t* m_out) {
    if (!ctx || !desc || !out) return HK_ERR_ARG;
    return ctx->ops->keygen(ctx, desc, out, m_out);
}
hk_status hk_exec_tree(hk_ctx* ctx, const hk_exec_tree_desc* desc, const hk_exec_tree_out* out) {
    if (!ctx || !desc || !out) return HK_ERR_ARG;
    return ctx->ops->exec_tree(ctx, desc, out);
}
hk_status hk_stage1_witness(hk_ctx* ctx, const hk_stage1_desc* desc, const uint32_t* sub_index, size_t batch, size_t n_v,
                            void* z_out) {
    if (!ctx || !desc) return HK_ERR_ARG;
    return ctx->ops->stage1_witness(ctx, desc, sub_index, batch, n_v, z_out);
}
hk_status hk_trace_sort(hk_ctx* ctx, uint32_t entry_fields, const void* time_entries_mont, size_t n_entries,
                        void* addr_entries_mont_out, uint32_t* perm_out) {
    if (!ctx) return HK_ERR_ARG;
    return ctx->ops->trace_sort(ctx, entry_fields, time_entries_mont, n_entries, addr_entries_mont_out, perm_out);
}
hk_status hk_stage0_witness(hk_ctx* ctx, const uint32_t* offsets, uint32_t n_sub, uint32_t n_portals, const void* time_entries_mont,
                            const void* addr_entries_mont, const uint32_t* sub_index, size_t batch, void* w_out) {
    if (!ctx) return HK_ERR_ARG;
    return ctx->ops->stage0_witness(ctx, offsets, n_sub, n_portals, time_entries_mont, addr_entries_mont, sub_index, batch, w_out);
}
hk_status hk_r1cs_check(hk_ctx* ctx, const hk_csr* A, const hk_csr* B, const hk_csr* C, const void* z_mont, size_t n_v, size_t batch,
                        hk_r1cs_verdict* verdicts, uint32_t* bad_rows, void* bad_vals, size_t cap) {
    if (!ctx || !A || !B || !C) return HK_ERR_ARG;
    return ctx->ops->r1cs_check(ctx, A, B, C, z_mont, n_v, batch, verdicts, bad_rows, bad_vals, cap);
}
hk_status hk_pk_r1cs_check(hk_ctx* ctx, const hk_pk* pk, const void* z_mont, size_t n_v, size_t batch, hk_r1cs_verdict* verdicts,
                           uint32_t* bad_rows, void* bad_vals, size_t cap) {
    if (!ctx || !pk) return HK_ERR_ARG;
    return ctx->ops->pk_r1cs_check(ctx, pk, z_mont, n_v, batch, verdicts, bad_rows, bad_vals, cap);
}
hk_status hk_sha_tree(hk_ctx* ctx, const void* leaves, uint32_t n_sub, uint32_t ns, uint32_t n_portals, const hk_sha_tree_out* out) {
    if (!ctx || !leaves || !out) return HK_ERR_ARG;
    return ctx->ops->sha_tree(ctx, leaves, n_sub, ns, n_portals, out);
}
hk_status hk_sha_tree_inputs(hk_ctx* ctx, const void* leaves, const void* digests, uint32_t n_sub, uint32_t n_inputs,
                             const uint32_t* sub_index, size_t batch, uint32_t* inputs_out) {
    if (!ctx) return HK_ERR_ARG;
    return ctx->ops->sha_tree_inputs(ctx, leaves, digests, n_sub, n_inputs, sub_index, batch, inputs_out);
}
hk_status hk_ram_stage0_witness(hk_ctx* ctx, const uint32_t* offsets, uint32_t n_sub, uint32_t n_portals,
                                const void* time_entries_mont, const void* addr_entries_mont, const uint32_t* sub_index, size_t batch,
                                void* w_out) {
    if (!ctx) return HK_ERR_ARG;
    return ctx->ops->ram_stage0_witness(ctx, offsets, n_sub, n_portals, time_entries_mont, addr_entries_mont, sub_index, batch, w_out);
}
hk_status hk_ram_stage1_witness(hk_ctx* ctx, const hk_ram_stage1_desc* desc, const uint32_t* sub_index, size_t batch, size_t n_v,
                                void* z_out) {
    if (!ctx || !desc) return HK_ERR_ARG;
    return ctx->ops->ram_stage1_witness(ctx, desc, sub_index, batch, n_v, z_out);
}
hk_status hk_r1cs_job_trace(hk_ctx* ctx, const hk_r1cs_job_desc* desc, void* time_entries_mont_out) {
    if (!ctx || !desc) return HK_ERR_ARG;
    return ctx->ops->r1cs_job_trace(ctx, desc, time_entries_mont_out);
}
hk_status hk_r1cs_job_witness(hk_ctx* ctx, const hk_r1cs_job_desc* desc, const uint32_t* sub_index, size_t batch, size_t n_v,
                              size_t body_col0, void* z_out) {
    if (!ctx || !desc) return HK_ERR_ARG;
    return ctx->ops->r1cs_job_witness(ctx, desc, sub_index, batch, n_v, body_col0, z_out);
}
hk_status hk_vkd_trace(hk_ctx* ctx, const hk_vkd_desc* desc, void* values_mont_out, void* time_entries_mont_out) {
    if (!ctx || !desc) return HK_ERR_ARG;
    return ctx->ops->vkd_trace(ctx, desc, values_mont_out, time_entries_mont_out);
}
hk_status hk_vkd_witness(hk_ctx* ctx, const hk_vkd_desc* desc, const uint32_t* sub_index, size_t batch, size_t n_v,
                         const hk_vkd_cols* cols, void* z_out) {
    if (!ctx || !desc) return HK_ERR_ARG;
    return ctx->ops->vkd_witness(ctx, desc, sub_index, batch, n_v, cols, z_out);
}
hk_status hk_vkd_tree(hk_ctx* ctx, const hk_vkd_tree_desc* desc, void* siblings_mont_out, void* roots_mont_out, uint8_t* status_out) {
    if (!ctx || !desc) return HK_ERR_ARG;
    return ctx->ops->vkd_tree(ctx, desc, siblings_mont_out, roots_mont_out, status_out);
}
hk_status hk_scalar_powers(hk_ctx* ctx, const void* x_mont, size_t n, size_t reps, void* out) {
    if (!ctx) return HK_ERR_ARG;
    return ctx->ops->scalar_powers(ctx, x_mont, n, reps, out);
}
hk_status hk_ipa_quotient(hk_ctx* ctx, const void* challenges_mont, size_t l, const void* rho_mont, const void* z_mont,
                          size_t shift, void* q_out) {
    if (!ctx) return HK_ERR_ARG;
    return ctx->ops->ipa_quotient(ctx, challenges_mont, l, rho_mont, z_mont, shift, q_out);
}
hk_status hk_class_power_sums(hk_ctx* ctx, const void* x_mont, const uint32_t* class_of, size_t n, size_t n_classes,
                              void* sums_out) {
    if (!ctx) return HK_ERR_ARG;
    return ctx->ops->class_power_sums(ctx, x_mont, class_of, n, n_classes, sums_out);
}

// ---- compressed points (point_codec.cuh).  A rule refuses with HK_ERR_ARG before anything is written: a missing buffer, an
// input that shares a byte with an output, two outputs that share one, n >= 2^31.
static bool codec_bufs_bad(const void* const* in, const size_t* in_len, int n_in, const void* const* out, const size_t* out_len,
                           int n_out) {
    for (int a = 0; a < n_in; a++)
        if (!in[a]) return true;
    for (int b = 0; b < n_out; b++) {
        if (!out[b]) return true;
        for (int a = 0; a < n_in; a++)
            if (hk::bufs_overlap(in[a], in_len[a], out[b], out_len[b])) return true;
        for (int c = 0; c < b; c++)
            if (hk::bufs_overlap(out[c], out_len[c], out[b], out_len[b])) return true;
    }
    return false;
}
hk_status hk_field_sqrt(hk_ctx* ctx, int which, const void* in_mont, size_t n, void* out_mont, uint8_t* ok) {
    if (!ctx || (which != 1 && which != 2) || n >= ((size_t)1 << 31)) return HK_ERR_ARG;
    if (n == 0) return HK_OK;
    const size_t eb = ctx->ops->fq_bytes * (size_t)which;
    const void* in[1] = {in_mont};
    const void* out[2] = {out_mont, ok};
    const size_t il[1] = {n * eb}, ol[2] = {n * eb, n};
    if (codec_bufs_bad(in, il, 1, out, ol, 2)) return HK_ERR_ARG;
    return ctx->ops->field_sqrt(ctx, which, in_mont, n, out_mont, ok);
}
static hk_status points_decompress(hk_ctx* ctx, int group, const void* x_canon, const uint8_t* flags, size_t n, int check,
                                   void* points_out, uint8_t* status) {
    if (!ctx || n >= ((size_t)1 << 31)) return HK_ERR_ARG;
    if (n == 0) return HK_OK;
    const size_t xb = ctx->ops->fq_bytes * (size_t)group;
    const void* in[2] = {x_canon, flags};
    const void* out[2] = {points_out, status};
    const size_t il[2] = {n * xb, n}, ol[2] = {2 * n * xb, n};
    if (codec_bufs_bad(in, il, 2, out, ol, 2)) return HK_ERR_ARG;
    return ctx->ops->points_decompress(ctx, group, x_canon, flags, n, check, points_out, status);
}
static hk_status points_compress(hk_ctx* ctx, int group, const void* points, size_t n, void* x_canon_out, uint8_t* flags_out) {
    if (!ctx || n >= ((size_t)1 << 31)) return HK_ERR_ARG;
    if (n == 0) return HK_OK;
    const size_t xb = ctx->ops->fq_bytes * (size_t)group;
    const void* in[1] = {points};
    const void* out[2] = {x_canon_out, flags_out};
    const size_t il[1] = {2 * n * xb}, ol[2] = {n * xb, n};
    if (codec_bufs_bad(in, il, 1, out, ol, 2)) return HK_ERR_ARG;
    return ctx->ops->points_compress(ctx, group, points, n, x_canon_out, flags_out);
}
hk_status hk_points_decompress_g1(hk_ctx* ctx, const void* x_canon, const uint8_t* flags, size_t n, int check, void* points_out,
                                  uint8_t* status) {
    return points_decompress(ctx, 1, x_canon, flags, n, check, points_out, status);
}
hk_status hk_points_decompress_g2(hk_ctx* ctx, const void* x_canon, const uint8_t* flags, size_t n, int check, void* points_out,
                                  uint8_t* status) {
    return points_decompress(ctx, 2, x_canon, flags, n, check, points_out, status);
}
hk_status hk_points_compress_g1(hk_ctx* ctx, const void* points, size_t n, void* x_canon_out, uint8_t* flags_out) {
    return points_compress(ctx, 1, points, n, x_canon_out, flags_out);
}
hk_status hk_points_compress_g2(hk_ctx* ctx, const void* points, size_t n, void* x_canon_out, uint8_t* flags_out) {
    return points_compress(ctx, 2, points, n, x_canon_out, flags_out);
}

}  // extern "C"

// ---- host utility: Keccak-f[1600], the permutation under the merlin transcripts of the aggregator (STROBE-128;
// distributed-prover/src/util.rs:22, aggregation.rs:219-222,276-278).  Plain C on the host: a pure-Python permutation costs
// 0.35 ms a call, 30 ms per aggregation.  state: 25 little-endian 64-bit lanes, lane (x, y) at x + 5 y.
extern "C" void hk_keccak_f1600(uint64_t* st) {
    static const uint64_t RC[24] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
        0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
        0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
        0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
        0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    static const int ROT[5][5] = {{0, 36, 3, 41, 18}, {1, 44, 10, 45, 2}, {62, 6, 43, 15, 61}, {28, 55, 25, 21, 56}, {27, 20, 39, 8, 14}};
    auto rol = [](uint64_t x, int n) { return n ? (x << n) | (x >> (64 - n)) : x; };
    for (int rnd = 0; rnd < 24; rnd++) {
        uint64_t c[5], d[5], b[25];
        for (int x = 0; x < 5; x++) c[x] = st[x] ^ st[x + 5] ^ st[x + 10] ^ st[x + 15] ^ st[x + 20];
        for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ rol(c[(x + 1) % 5], 1);
        for (int i = 0; i < 25; i++) st[i] ^= d[i % 5];
        for (int x = 0; x < 5; x++)
            for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = rol(st[x + 5 * y], ROT[x][y]);
        for (int y = 0; y < 5; y++)
            for (int x = 0; x < 5; x++) st[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        st[0] ^= RC[rnd];
    }
}
