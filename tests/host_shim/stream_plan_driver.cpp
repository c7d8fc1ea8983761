// Prints the prove-lane stream plan of hekaton_system_amd/csrc/stream_plan.h for tests/test_stream_plan_cpu.py:
//   "s Q K <streams>" for Q = 0 .. 40, K = 1 .. 4, then "map s <stream of main> <B1> <B2> <L> <H>" for s = 1 .. 5.
#include <cstdio>

#include "../../hekaton_system_amd/csrc/stream_plan.h"

int main() {
    for (unsigned q = 0; q <= 40; q++)
        for (unsigned k = 1; k <= 4; k++) printf("s %u %u %u\n", q, k, hk::prove_lane_streams(q, k));
    for (unsigned s = 1; s <= hk::PROVE_MAX_STREAMS; s++) {
        printf("map %u", s);
        for (int r = 0; r < hk::PROVE_ROLES; r++) printf(" %u", hk::prove_role_stream(s, (hk::ProveRole)r));
        printf("\n");
    }
    return 0;
}
