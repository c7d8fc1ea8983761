/*
 * hekaton_gt.h — companion to hekaton.h: membership in GT, the twin of hk_points_check_g1 / _g2 for the third group.
 *
 * A separate header only for now: tests/test_capi_signatures_cpu.py pins hekaton.h at its present list of declarations
 * (and capi.py's first signature table at exactly those names), and existing test files do not change with a feature.
 * Folding this header into hekaton.h - and capi.py's second table into the first - waits for a change that may touch
 * that test.  Conventions ([h|d] pointers, Montgomery limbs, thread safety) are hekaton.h's.
 */
#ifndef HEKATON_GT_H
#define HEKATON_GT_H

#include "hekaton.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ok[i] = 1 when fq12_in[i] lies in GT - it is not zero and fq12_in[i]^r = 1, r the order of G1 and G2 - else 0.  ark's
 * `PairingOutput` deserialises WITHOUT this check, and hk_gt_pow's Frobenius split is a power only for such elements: a
 * verifier that reads Fq12 values from untrusted bytes asks here before it uses them as GT members (the wire readers of
 * hekaton_system_amd/agg_verify.py do).  One wavefront per element on the wave Fq12 multiplier; with q the base prime, t
 * the trace of Frobenius, u the curve parameter and Phi_12(q) = q^4 - q^2 + 1, for x = fq12_in[i]:
 *   1. x != 0, and each of its 12 coefficients is a canonical Fq (below q; anything else is refused, not reduced);
 *   2. x^(q^4) * x == x^(q^2): x lies in the cyclotomic subgroup, of order Phi_12(q) - two Frobenius maps, one product,
 *      no inversion;
 *   3. x^q == x^(t - 1), the right side by the final exponentiation's chains: t - 1 = 6 u^2 on BN254 (x^u twice, then
 *      y -> (y^2 y)^2), t - 1 = u on BLS12-381.
 * 2 and 3 together say ord(x) divides gcd(Phi_12(q), q - (t - 1)), which is r on both curves (BN254: q + 1 - t = r itself;
 * BLS12-381: q - u = r (u - 1)^2 / 3, and (u - 1)^2 / 3 is coprime to Phi_12(q)).  3's chain squares with the cyclotomic
 * formula and inverts by conjugation, which are a square and an inverse only on the cyclotomic subgroup: an element that
 * fails 1 or 2 is refused before the chain runs.  Zero satisfies 2 and 3 as 0 == 0, hence 1.  126 cyclotomic
 * squarings and 56 products on BN254, 63 and 6 on BLS12-381, against the 254 squarings and ~127 products of
 * hk_fq12_pow with exponent r - the only test there was.
 * fq12_in [h|d]: n Fq12 in the GT layout of hk_multi_pairing (12 Fq, Montgomery); ok [h|d]: n bytes.  HK_ERR_ARG for a
 * NULL pointer with n > 0 or n >= 2^31; n == 0 is HK_OK and writes nothing. */
hk_status hk_gt_check(hk_ctx* ctx, const void* fq12_in, size_t n, uint8_t* ok);

#ifdef __cplusplus
}
#endif

#endif  /* HEKATON_GT_H */
