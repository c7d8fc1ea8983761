// launch.h — the one way the library launches a kernel: named, checked, and counted for the scratch-ring budget.
// HK_LAUNCH((kernel<...>), grid, block, lds, stream, args...) launches, checks hipGetLastError() for that launch and
// returns HK_ERR_DEVICE from the enclosing function when it failed (HK_TRY of hk_internal.h, which includes this header);
// HK_LAUNCH_STATUS is the same as an expression, for a site with an error idiom of its own.  With HK_DEBUG_SYNC=1 every
// launch is named on stderr, synchronised and named again with its outcome, so a faulting kernel is the last one "launched"
// and not "finished".
// Every kernel for which the helper is instantiated is in kernel_registry() from the moment the library is loaded, whether
// or not that launch ever executes: the deepest private-memory frame over the registry is what hk_ctx_create sizes every
// hardware queue's scratch ring to.  A kernel is counted because it is launched through here.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/hekaton.h"

#if defined(__HIPCC__)
#include <hip/hip_ext.h>

namespace hk {

struct KernelEntry {
    const void* fn;              // the kernel's host handle (what hipFuncGetAttributes takes)
    const char* pretty;          // kernel_pretty<K>(): "... [K = &hk::k_name, T = void (*)(parameter types)]"
    const char* only_with_env;   // the environment switch without which nothing launches it, or nullptr
};
// in registration order, one entry per instantiation of Kernel<K, Gate> per translation unit: read it deduplicated by fn
inline std::vector<KernelEntry>& kernel_registry() {
    static std::vector<KernelEntry> r;
    return r;
}
// (a function template: __PRETTY_FUNCTION__ is valid inside a function only; T spells the instantiation, which K's own
// spelling leaves out)
template <auto K, class T = decltype(K)> const char* kernel_pretty() { return __PRETTY_FUNCTION__; }

// where a kernel's launches sit behind an environment switch, the Gate names it; such a kernel's frame counts towards the
// scratch budget only when the switch is set
struct Ungated { static const char* env() { return nullptr; } };

template <auto K, class Gate> struct KernelReg { static const bool registered; };
template <auto K, class Gate>
const bool KernelReg<K, Gate>::registered = (kernel_registry().push_back({(const void*)K, kernel_pretty<K>(), Gate::env()}), true);

static inline bool debug_sync() { static const bool on = getenv("HK_DEBUG_SYNC") != nullptr; return on; }

template <auto K, class Gate = Ungated> struct Kernel;
template <class... P, void (*K)(P...), class Gate>
struct Kernel<K, Gate> {
    // name: the kernel as the launch site spells it (HK_LAUNCH's parentheses are stripped).  ev0 and ev1, both or neither:
    // they take the kernel's own start / stop timestamps (hipExtLaunchKernelGGL)
    static hk_status launch(const char* name, dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1,
                            P... args) {
        (void)&KernelReg<K, Gate>::registered;
        if (ev0 && ev1) hipExtLaunchKernelGGL(K, grid, block, (unsigned)lds, s, ev0, ev1, 0, args...);
        else hipLaunchKernelGGL(K, grid, block, lds, s, args...);
        hipError_t e = hipGetLastError();
        int len = (int)strlen(name);
        if (len >= 2 && name[0] == '(' && name[len - 1] == ')') { name++; len -= 2; }
        if (e != hipSuccess) {
            fprintf(stderr, "[hekaton] HIP error %s at the launch of %.*s\n", hipGetErrorName(e), len, name);
            return HK_ERR_DEVICE;
        }
        if (debug_sync()) {
            fprintf(stderr, "[hk] launched %.*s\n", len, name); fflush(stderr);
            e = hipStreamSynchronize(s);
            fprintf(stderr, "[hk] finished %.*s: %s\n", len, name, hipGetErrorName(e)); fflush(stderr);
            if (e != hipSuccess) return HK_ERR_DEVICE;
        }
        return HK_OK;
    }
};

}  // namespace hk

#define HK_LAUNCH_TIMED_STATUS(kernel, grid, block, lds, stream, ev0, ev1, ...) \
    (::hk::Kernel<kernel>::launch(#kernel, grid, block, lds, stream, ev0, ev1, ##__VA_ARGS__))
#define HK_LAUNCH_STATUS(kernel, grid, block, lds, stream, ...) \
    HK_LAUNCH_TIMED_STATUS(kernel, grid, block, lds, stream, nullptr, nullptr, ##__VA_ARGS__)
#define HK_LAUNCH(...) HK_TRY(HK_LAUNCH_STATUS(__VA_ARGS__))
#define HK_LAUNCH_TIMED(...) HK_TRY(HK_LAUNCH_TIMED_STATUS(__VA_ARGS__))
// a kernel behind an environment switch: gate is a struct like hk::Ungated whose env() names the switch
#define HK_LAUNCH_GATED(gate, kernel, grid, block, lds, stream, ...) \
    HK_TRY((::hk::Kernel<kernel, gate>::launch(#kernel, grid, block, lds, stream, nullptr, nullptr, ##__VA_ARGS__)))

#endif  // __HIPCC__
