// Prints the NTT pass plans of hekaton_system_amd/csrc/ntt_plan.h for tests/test_ntt_plan_cpu.py and the tests that chain
// passes by the plan:
//   "knob <raw tile_log> <raw upper_max> <tile_log> <upper_max>" for raw tile_log = 0 .. 13, raw upper_max = 0 .. 13, then
//   "plan <logn> <tile_log> <raw upper_max> <upper_max> <np> <lo> <nst> <cols_bits> ..." for logn = 0 .. 32,
//   tile_log = 8 .. 11, raw upper_max = 0 .. 12.
#include <cstdio>

#include "../../hekaton_system_amd/csrc/ntt_plan.h"

int main() {
    for (unsigned t = 0; t <= 13; t++)
        for (unsigned u = 0; u <= 13; u++) {
            unsigned tl = hk::ntt_plan_tile_log(t);
            printf("knob %u %u %u %u\n", t, u, tl, hk::ntt_plan_upper_max(u, tl));
        }
    for (unsigned logn = 0; logn <= 32; logn++)
        for (unsigned t = 8; t <= 11; t++)
            for (unsigned u = 0; u <= 12; u++) {
                hk::NttPass ps[hk::NTT_PLAN_MAX_PASSES];
                unsigned um = hk::ntt_plan_upper_max(u, t);
                int np = hk::ntt_pass_plan(logn, t, um, ps);
                printf("plan %u %u %u %u %d", logn, t, u, um, np);
                for (int k = 0; k < np; k++) printf(" %u %u %u", ps[k].lo, ps[k].nst, ps[k].cols_bits);
                printf("\n");
            }
    return 0;
}
