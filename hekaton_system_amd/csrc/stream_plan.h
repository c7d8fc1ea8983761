// stream_plan.h — how prove_batch's five query roles share the streams of a prove lane.
// Plain C++, no HIP: tests/test_stream_plan_cpu.py compiles it into a small host program.
//
// Packets on one hardware queue run in order, so two streams that share a queue serialise.  A context therefore owns
// PROVE_COALESCE_RUNNING prove lanes of s = clamp(Q / K, 1, 5) streams each, created before anything else of the context,
// so that the runtime gives each of those streams its own queue, and a chunk's five roles fold onto its lane's s streams.
#pragma once

namespace hk {

// the five roles of a proof chunk: main (z sort, A, the finish kernels), B1, B2 (G2), L, H (witness map, H sort, H)
enum ProveRole { ROLE_MAIN = 0, ROLE_B1, ROLE_B2, ROLE_L, ROLE_H, PROVE_ROLES };
enum { PROVE_MAX_STREAMS = 5 };

// streams of each of `lanes` prove lanes when the process has `queues` hardware queues
inline unsigned prove_lane_streams(unsigned queues, unsigned lanes) {
    unsigned s = lanes ? queues / lanes : queues;
    if (s < 1) s = 1;
    if (s > PROVE_MAX_STREAMS) s = PROVE_MAX_STREAMS;
    return s;
}

// the stream (0 .. s - 1) each role runs on, for s streams.  Stream 0 always carries main.  From the per-proof kernel
// times the query roles together are shorter than H, so H keeps a stream of its own from s = 2 on, and B1 / B2, the
// longest queries, get theirs before L does.
//   s = 1: everything on one stream          s = 2: {main, B1, B2, L} {H}        s = 3: {main, L} {B1, B2} {H}
//   s = 4: {main, L} {B1} {B2} {H}           s = 5: one stream per role
inline unsigned prove_role_stream(unsigned s, ProveRole role) {
    static const unsigned char map[PROVE_MAX_STREAMS][PROVE_ROLES] = {
        //  main B1 B2 L  H
        {0, 0, 0, 0, 0},
        {0, 0, 0, 0, 1},
        {0, 1, 1, 0, 2},
        {0, 1, 2, 0, 3},
        {0, 1, 2, 3, 4},
    };
    if (s < 1) s = 1;
    if (s > PROVE_MAX_STREAMS) s = PROVE_MAX_STREAMS;
    return map[s - 1][role];
}

}  // namespace hk
