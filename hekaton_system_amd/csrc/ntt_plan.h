// ntt_plan.h — which butterfly stages each launch of k_ntt_pass4 (ntt.cuh) takes: the pass list of a 2^logn transform and
// the normalisation of the two knobs that shape it.  Plain C++, no HIP: tests/test_ntt_plan_cpu.py compiles it into a small
// host program.
//
// The bottom pass runs the low min(logn, tile_log) stages on contiguous tiles of 2^tile_log elements; the stages above it
// are split evenly over ceil(rest / upper_max) upper passes, the larger shares first, whose tiles are 2^nst rows of
// 2^(tile_log - nst) contiguous elements.  With the defaults (tile_log 11, upper_max 6), as stage counts from stage 0 up:
//   2^11: 11        2^12: 11+1      2^16: 11+5      2^17: 11+6      2^21: 11+5+5    2^22: 11+6+5
// What every pass satisfies is k_ntt_pass4's contract: nst >= 1, cols_bits <= lo, nst + cols_bits <= tile_log.
#pragma once
#include <cstdint>

namespace hk {

typedef uint32_t u32;

constexpr u32 NTT_PLAN_TILE_LOG = 11;        // elements per LDS tile (ntt.cuh: NTT_TILE_LOG)
constexpr u32 NTT_PLAN_UPPER_MAX = 6;        // 2^21: 11+5+5, 2^22: 11+6+5 (a single 10-stage upper pass with 64-B rows
                                             // measured the same alone and less steady under load)
constexpr int NTT_PLAN_MAX_PASSES = 34;

struct NttPass { u32 lo, nst, cols_bits; };

// HK_NTT_TILE_LOG as given -> the tile size used: [8, 11]
inline u32 ntt_plan_tile_log(u32 raw) { return raw < 8 ? 8u : (raw > NTT_PLAN_TILE_LOG ? NTT_PLAN_TILE_LOG : raw); }

// HK_NTT_UPPER_MAX as given -> the stages an upper pass may take: [1, min(10, tile_log)].  A pass of more stages than the
// tile has address bits has no tile shape (cols_bits = tile_log - nst would wrap).
inline u32 ntt_plan_upper_max(u32 raw, u32 tile_log) {
    u32 v = raw < 1 ? 1u : (raw > 10 ? 10u : raw);
    return v > tile_log ? tile_log : v;
}

// The passes of a 2^logn transform (logn <= 32) in DIT order (stage 0 first; a DIF chain runs them backwards), from
// NORMALISED knobs.  Returns their number, 0 for logn == 0.
inline int ntt_pass_plan(u32 logn, u32 tile_log, u32 upper_max, NttPass out[NTT_PLAN_MAX_PASSES]) {
    if (logn == 0) return 0;
    u32 bottom = logn < tile_log ? logn : tile_log;
    u32 rest = logn - bottom;
    u32 npass = (rest + upper_max - 1) / upper_max;
    int np = 0;
    out[np++] = {0, bottom, 0};
    u32 lo = bottom;
    for (u32 i = 0; i < npass; i++) {
        u32 nst = (rest - (lo - bottom) + (npass - i) - 1) / (npass - i);
        out[np++] = {lo, nst, tile_log - nst};
        lo += nst;
    }
    return np;
}

}  // namespace hk
