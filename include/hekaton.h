/*
 * hekaton.h — C ABI of the MI355X-native Hekaton subcircuit prover (libhekaton.so).
 *
 * This is the drop-in boundary for ONE hot path of zhaowenlan1779/hekaton-system:
 * the per-subcircuit CP-Groth16 commit + prove step.  The reference has no FFI
 * (SURVEY.md F5); the entry points below are what a Rust shim binds to replace
 * the arkworks call sites of that path (the binding is shown in INTEGRATION.md).
 * Every entry point cites the reference interface it replaces (paths relative to
 * the reference repository root).
 *
 * Conventions
 *   - Field elements are little-endian limb arrays in MONTGOMERY form with
 *     R = 2^(64*N), exactly the in-memory form of ark-ff `Fp<MontBackend<_,N>>`
 *     (N = 4 for BN254 Fr/Fq and BLS12-381 Fr; N = 6 for BLS12-381 Fq), unless a
 *     parameter says "canonical" (ark `BigInt<N>`: plain integer, LE limbs).
 *   - G1 affine = x || y ; G2 affine = x.c0 || x.c1 || y.c0 || y.c1 ; the point at
 *     infinity is encoded as all-zero coordinates ((0,0) is on neither curve).
 *     Rust `Affine<P>{x,y,infinity}` is not repr(C): the shim repacks once at
 *     key-load time.
 *   - Pointers marked [h|d] may be host or device memory (detected with
 *     hipPointerGetAttributes); [h] must be host, [d] must be device.
 *   - All calls are thread-safe on a shared hk_ctx: each call runs on a private
 *     lane (HIP stream + scratch arena), mirroring `compute_responses`
 *     (mpi-snark/src/bin/node.rs:745-795) which proves from several OS threads.
 *   - There is NO CPU backend: hk_ctx_create fails with HK_ERR_DEVICE when no
 *     gfx950 device is usable.  Randomness (r, s, kappa) always comes from the
 *     caller (prover.rs:28-29, committer.rs:85); the library is deterministic.
 */
#ifndef HEKATON_H
#define HEKATON_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hk_ctx hk_ctx;   /* one per (process, device): lanes, twiddles, scratch */
typedef struct hk_pk hk_pk;
typedef struct hk_vk hk_vk;     /* prepared verifying key (hk_vk_prepare) */     /* device-resident proving-key class (+ its R1CS matrices) */

typedef enum { HK_BN254 = 0, HK_BLS12_381 = 1 } hk_curve;

typedef enum {
    HK_OK = 0,
    HK_ERR_LEN = 1,               /* ark `msm` Err(min_len) on length mismatch   */
    HK_ERR_DOMAIN_TOO_LARGE = 2,  /* SynthesisError::PolynomialDegreeTooLarge                 */
    HK_ERR_DEVICE = 3,            /* no device / HIP runtime error                            */
    HK_ERR_ARG = 4,
    HK_ERR_NOMEM = 5
} hk_status;

/* One R1CS matrix in CSR form; mirrors one of ark_relations `ConstraintMatrices::{a,b,c}`
 * (Vec<Vec<(F, usize)>>): row i holds (val, col) pairs, col indexes instance||witness. */
typedef struct {
    const uint64_t* row_ptr;   /* [n_rows + 1]                 [h|d] */
    const uint32_t* col;       /* [nnz]                        [h|d] */
    const void*     val_mont;  /* [nnz] Fr, Montgomery         [h|d] */
    size_t n_rows;
    size_t nnz;
} hk_csr;

/* Everything `ProvingKey<E>` (cp-groth16/src/data_structures.rs:66-83) holds that the
 * prover touches, plus the circuit class's constraint matrices (identical for every
 * subcircuit of a class, so uploaded once with the key). All arrays [h|d], packed affine. */
typedef struct {
    const void* a_g;  size_t a_len;        /* pk.a_g   : n_v G1  (data_structures.rs:72) */
    const void* b_g;  size_t b_g_len;      /* pk.b_g   : n_v G1  (:74)                   */
    const void* b_h;  size_t b_h_len;      /* pk.b_h   : n_v G2  (:76)                   */
    const void* h_g;  size_t h_len;        /* pk.h_g   : m-1 G1  (:78)                   */
    const void* const* ck_stage;           /* pk.ck.deltas_abc_g[stage] (:113)           */
    const size_t* ck_len;
    size_t n_stages;
    const void* deltas_g;                  /* pk.deltas_g : n_stages G1 (:82)            */
    const void* last_delta_h;              /* pk.vk.deltas_h.last() : 1 G2 (:95-97)      */
    const void* alpha_g;                   /* pk.vk.alpha_g : 1 G1 (:36)                 */
    const void* beta_g;                    /* pk.beta_g : 1 G1 (:70)                     */
    const void* beta_h;                    /* pk.vk.beta_h : 1 G2 (:38)                  */
    const hk_csr* A; const hk_csr* B; const hk_csr* C;   /* may be NULL: then hk_prove is unavailable */
    size_t n_inst;                         /* cs.num_instance_variables()                */
    size_t n_constraints;                  /* cs.num_constraints()                       */
} hk_pk_desc;

/* Per-phase device timings of the last hk_prove / hk_commit on the calling thread's lane,
 * measured with HIP events on the lane's stream (milliseconds). Replaces the reference's
 * start_timer!/end_timer! brackets (cp-groth16/src/prover.rs:65-150).
 * After an hk_prove that ran in a coalesced chunk of batch_proofs proofs, every *_ms field is this proof's share of the
 * chunk (the chunk's figure / batch_proofs) and accum_kernel_launches is 4, as for a proof that ran alone.
 * The struct grew: batch_proofs was appended after keygen_sweeps_ms; a host that mirrors it must add the field. */
typedef struct {
    float total_ms;
    float digits_ms;       /* scalar from-Montgomery + signed-digit split + bucket sort   */
    float msm_a_ms;        /* "Compute A"        prover.rs:85-90   */
    float msm_b_g1_ms;     /* "Compute B in G1"  prover.rs:95-100  */
    float msm_b_g2_ms;     /* "Compute B in G2"  prover.rs:105-108 */
    float msm_l_ms;        /* "Compute L"        prover.rs:113-118 */
    float witness_map_ms;  /* "R1CS to QAP witness map" prover.rs:122-125 */
    float msm_h_ms;        /* "Compute H"        prover.rs:127-130 */
    float finish_ms;       /* "Finish C" + into_affine prover.rs:135-155, committer.rs:112-114 */
    float accum_kernel_ms; /* sum over this call's k_msm_accum0<Fq> launches (dominant kernel),  */
    uint32_t accum_kernel_launches;  /* timed on the kernel itself; and how many launches that was */
    float accum_h_ms;      /* the H-query launch alone (the dense one)                             */
    float keygen_qap_ms;      /* hk_keygen only (total_ms spans the call): the QAP at t (Lagrange coefficients +   */
    float keygen_scalars_ms;  /* column sums), the scalar assembly, and every fixed-base sweep with its copy-out    */
    float keygen_sweeps_ms;
    uint32_t batch_proofs;    /* hk_prove / hk_prove_batch: proofs in the chunk the call ran in (1: it ran alone)       */
} hk_timings;

const char* hk_status_str(hk_status s);
const char* hk_version(void);
/* Diagnostics: entry i of the kernels the library launches - every one of them, since each is launched through one helper
 * that registers it when the library is loaded.  name: the kernel and its parameter types; only_with_env: NULL, or the
 * environment switch without which nothing launches it; private_bytes: its private-memory frame per lane, from the loaded
 * code object - the deepest of them (over the entries whose switch, if any, is set) sizes every hardware queue's scratch
 * ring.  private_bytes may be NULL: no HIP call is made then, so the list can be read on a machine without a GPU.  The
 * strings live as long as the library.  HK_ERR_ARG once i is past the end. */
hk_status hk_kernel_info(size_t i, const char** name, size_t* private_bytes, const char** only_with_env);

/* ---- context ------------------------------------------------------------------------ */
hk_status hk_ctx_create(hk_curve curve, int device_id, hk_ctx** out);
void      hk_ctx_destroy(hk_ctx* ctx);
hk_status hk_ctx_sync(hk_ctx* ctx);                      /* drain every lane */
hk_status hk_ctx_set_profiling(hk_ctx* ctx, int enable); /* record hk_timings per call */
hk_status hk_ctx_last_timings(hk_ctx* ctx, hk_timings* out);
/* element sizes for this curve: Fr, Fq, G1 affine, G2 affine bytes */
hk_status hk_ctx_sizes(const hk_ctx* ctx, size_t* fr, size_t* fq, size_t* g1, size_t* g2);

/* device-memory plumbing so a host (Rust shim, ctypes) can keep inputs resident */
hk_status hk_dev_alloc(hk_ctx* ctx, size_t bytes, void** dptr);
hk_status hk_dev_free(hk_ctx* ctx, void* dptr);
hk_status hk_dev_upload(hk_ctx* ctx, void* dst_d, const void* src_h, size_t bytes);
hk_status hk_dev_download(hk_ctx* ctx, void* dst_h, const void* src_d, size_t bytes);

/* ---- primitives: one per arkworks call the hot path makes ----------------------------- */

/* VariableBaseMSM for G1 — replaces `G::Group::msm_bigint(&query[1..], assignment)`
 * (cp-groth16/src/prover.rs:167, scalars canonical BigInt) and `E::G1::msm(bases, scalars)`
 * (prover.rs:117,129; committer.rs:89, scalars Montgomery Fr) and `msm_unchecked`
 * (committer.rs:113).  checked != 0: HK_ERR_LEN when n_bases != n_scalars (ark `msm`);
 * checked == 0: zip to min(n_bases, n_scalars) (ark `msm_unchecked` / `msm_bigint`).
 * out_affine [h]: packed affine sum (infinity = zeros). */
hk_status hk_msm_g1(hk_ctx* ctx, const void* bases, size_t n_bases,
                    const void* scalars, size_t n_scalars,
                    int scalars_are_montgomery, int checked, void* out_affine);
/* Same for G2 — replaces prover.rs:107 (`calculate_coeff` over pk.b_h). */
hk_status hk_msm_g2(hk_ctx* ctx, const void* bases, size_t n_bases,
                    const void* scalars, size_t n_scalars,
                    int scalars_are_montgomery, int checked, void* out_affine);

/* ark-poly Radix2EvaluationDomain {fft,ifft}_in_place and the coset forms with shift
 * F::GENERATOR.  data [h|d]: 2^log_m Fr (Montgomery), natural order in
 * and out.  HK_ERR_DOMAIN_TOO_LARGE when log_m > TWO_ADICITY. */
hk_status hk_ntt(hk_ctx* ctx, void* data, unsigned log_m, int inverse, int coset);

/* R1CSToQAP::witness_map (LibsnarkReduction) — replaces `cs.map(QAP::witness_map::<_, D<_>>)`
 * at cp-groth16/src/prover.rs:123.  z_mont: full assignment instance||witness (n_v Fr).
 * h_out [h|d]: m Fr (Montgomery), natural order; *m_out = domain size. */
hk_status hk_witness_map(hk_ctx* ctx, const hk_csr* A, const hk_csr* B, const hk_csr* C,
                         size_t n_inst, size_t n_constraints,
                         const void* z_mont, size_t n_v,
                         void* h_out, size_t h_capacity, size_t* m_out);

/* Fixed-base batch scalar multiplication: out[i] = scalars[i] * base, normalised to affine.
 * Replaces `FixedBase::msm` + `normalize_batch` of the trusted setup (cp-groth16/src/generator.rs:
 * 134-224).  base [h|d]: one affine point; scalars [h|d]: n Fr;
 * out [h|d]: n packed affine points.  The base's window table (`FixedBase::get_window_table`: a 248-step doubling chain,
 * 2 ms in G1 and 5 - 6 ms in G2) is kept per context for the first 8 distinct HOST bases and reused by later calls
 * (HK_FB_NO_CACHE=1: rebuilt every call); results do not depend on it. */
hk_status hk_fixed_base_g1(hk_ctx* ctx, const void* base, const void* scalars, size_t n,
                           int scalars_are_montgomery, void* out);
hk_status hk_fixed_base_g2(hk_ctx* ctx, const void* base, const void* scalars, size_t n,
                           int scalars_are_montgomery, void* out);

/* N independent scalar multiplications out[i] = scalars[i] * points[i], batch-normalised to affine —
 * replaces `scalar_pairing` (distributed-prover/src/pairing_ops.rs:32-39: `*si * *ri` + `normalize_batch`),
 * called 8x per aggregation with N = #subcircuits (aggregation.rs:236-242,289-310).
 * points [h|d]: n packed affine; scalars [h|d]: n Fr (Montgomery); out [h|d]: n packed affine. */
hk_status hk_scalar_pairing_g1(hk_ctx* ctx, const void* points, const void* scalars, size_t n, void* out);
hk_status hk_scalar_pairing_g2(hk_ctx* ctx, const void* points, const void* scalars, size_t n, void* out);

/* ---- pairings of the aggregation path -------------------------------------------------------
 * GT elements cross the ABI as ark's `Fp12`: c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1 - 12 Fq, Montgomery
 * (hk_ctx_gt_bytes: 384 B on BN254, 576 B on BLS12-381).
 * hk_multi_pairing: prod_i e(g1[i], g2[i]) = `E::final_exponentiation(E::multi_miller_loop(left, right))` - replaces
 * `pairing(left, right)` (distributed-prover/src/pairing_ops.rs:9-29; pairs with an infinity member contribute 1,
 * n = 0 gives 1).  g1 [h|d]: n packed G1 affine; g2 [h|d]: n packed G2 affine; gt_out [h|d].
 * hk_pairing_products: every lhs vector against every rhs vector in ONE batched launch,
 * gt_out[a * n_rhs + b] = pairing(lhs_g1[a], rhs_g2[b]) - replaces the 4 x 4 `cross_terms` of
 * distributed-prover/src/aggregation.rs:255-263 and, with n_lhs = n_rhs = 1, the IPP commitments'
 * inner products (aggregation.rs:97-103,167-168).  All vectors have n elements. */
hk_status hk_multi_pairing(hk_ctx* ctx, const void* g1, const void* g2, size_t n, void* gt_out);
hk_status hk_pairing_products(hk_ctx* ctx, const void* const* lhs_g1, size_t n_lhs, const void* const* rhs_g2,
                              size_t n_rhs, size_t n, void* gt_out);
/* hk_pairing_pairs: the same batched launch for a LIST of (lhs vector, rhs vector) pairs instead of the full grid:
 * gt_out[p] = pairing(lhs_g1[pair_lhs[p]], rhs_g2[pair_rhs[p]]), p < n_pairs <= 64.  One GIPA round of the TIPA prover
 * (ark-ip-proofs `gipa` under distributed-prover/src/aggregation.rs:340) needs ten inner products between six G1 and six
 * G2 half-vectors - e(A_R, v1_L), e(w1_R, B_L), ... - each rhs vector's Miller lines are computed once and shared by the
 * pairs that use it.  pair_lhs, pair_rhs [h]: n_pairs indices into lhs_g1 / rhs_g2 (at most 64 pairs).  TWO rounds fit one
 * call: round k + 1's messages are inner products of the folded vectors, by bilinearity products of quarter-by-quarter
 * inner products of the current vectors raised to 1, c, 1 / c - sixty pairs out of twelve G1 and twelve G2 quarter
 * vectors, then hk_gt_pow_prod (hekaton_system_amd/tipa.py `_round_pair`). */
hk_status hk_pairing_pairs(hk_ctx* ctx, const void* const* lhs_g1, size_t n_lhs, const void* const* rhs_g2, size_t n_rhs,
                           const uint32_t* pair_lhs, const uint32_t* pair_rhs, size_t n_pairs, size_t n, void* gt_out);
hk_status hk_ctx_gt_bytes(const hk_ctx* ctx, size_t* gt);
/* gt_out[i] = gt_in[i]^scalars[i] in GT - `Commitment * scalar` (distributed-prover/src/aggregation.rs:171-174,328-332) and
 * the six GT powers per round of the TIPA verifier; one wavefront per element.  gt_in, gt_out [h|d]: n GT elements;
 * scalars_mont [h|d]: n Fr.  The inputs must lie IN GT (order r: pairing values and their products - what `PairingOutput`
 * holds): the exponent is split along the Frobenius, z^c = prod_j pi^j(z)^(k_j) with four parts of <= 67 bits, which is
 * z^c only there (hk_fq12_pow below takes any element; HK_GT_POW_PLAIN in the environment routes hk_gt_pow to it). */
hk_status hk_gt_pow(hk_ctx* ctx, const void* gt_in, const void* scalars_mont, size_t n, void* gt_out);
/* The same power for ANY Fq12 elements (the plain 254-step square-and-multiply chain): what a verifier uses on values it
 * has not produced itself - the GT members of a TIPA proof (ark's `PairingOutput` deserialises without a subgroup check). */
hk_status hk_fq12_pow(hk_ctx* ctx, const void* fq12_in, const void* scalars_mont, size_t n, void* fq12_out);
/* Grouped multi-exponentiation: gt_out[g] = prod_{j < group_len} gt_in[g * group_len + j]^scalars[g * group_len + j], n a
 * multiple of group_len, n / group_len <= 65535 groups.  The fold check of the TIPA verifier (ark-ip-proofs `gipa` verify
 * under distributed-prover/src/aggregation.rs:340): T' = T * prod_k TL_k^(c_k) TR_k^(1/c_k), likewise U and Z - three groups
 * of 2 log2(N) powers; the powers run one wavefront per element as in hk_gt_pow / hk_fq12_pow (in_gt != 0: the Frobenius
 * split, elements of GT only; 0: the plain chain, any Fq12 element), then one wavefront per group multiplies them up.
 * gt_in [h|d]: n elements; scalars_mont [h|d]: n Fr; gt_out [h|d]: n / group_len elements. */
hk_status hk_gt_pow_prod(hk_ctx* ctx, const void* gt_in, const void* scalars_mont, size_t n, size_t group_len, int in_gt,
                         void* gt_out);

/* Element-wise linear combination of k <= 8 point vectors: out[i] = sum_j coeffs[j] * vecs[j][i], batch-normalised to
 * affine.  Replaces the aggregator's `prepared_input = s0 + s1*x0 + s2*x1 + s3*x2` (distributed-prover/src/
 * aggregation.rs:192-203) and the `left` / `right` combinations of :293-326 (three constant-scalar `scalar_pairing`
 * sweeps + element-wise additions each) with ONE launch sharing one doubling chain.
 * vecs [h]: k pointers, each [h|d] to n packed affine points; coeffs_mont [h|d]: k Fr; out [h|d]: n packed affine. */
hk_status hk_points_lincomb_g1(hk_ctx* ctx, const void* const* vecs, const void* coeffs_mont, size_t k, size_t n, void* out);
hk_status hk_points_lincomb_g2(hk_ctx* ctx, const void* const* vecs, const void* coeffs_mont, size_t k, size_t n, void* out);
/* out[i] = lo[i] + sum_{j<4} s_j * coeffs4[j] * psi^j(hi[i]) in G2, s_j = -1 where bit j of neg_mask is set: the G2 fold
 * `lo + c * hi` of a TIPA / GIPA round (ark-ip-proofs `gipa`, called from distributed-prover/src/aggregation.rs:340) with the
 * challenge split by the caller into four ~64-bit parts along psi, the untwist-Frobenius-twist endomorphism of G2
 * (psi(Q) = [q mod r] Q: c = sum s_j coeffs4[j] lambda^j mod r with lambda = 6 x^2 on BN254, x on BLS12-381) - the shared
 * doubling chain is ~66 steps instead of 254.  lo, hi [h|d]: n G2 points; coeffs4_mont [h|d]: 4 Fr; out [h|d]: n G2.
 * Magnitudes: host-resident coeffs may be any values below r - parts longer than the short-vector kernel reads (above
 * 0x77..7 over 18 hex digits, 71 bits; G1: over 34 hex digits, 135 bits) take a slower kernel that is right for every
 * magnitude.  Device-resident coeffs are not inspected and MUST stay within that bound (a nearest-plane split does: its
 * parts are below 2^66 in G2 and 2^130 in G1); beyond it the result of a call with 4 n <= 65536 (G1: 2 n) is undefined. */
hk_status hk_points_fold_g2(hk_ctx* ctx, const void* lo, const void* hi, const void* coeffs4_mont, unsigned neg_mask, size_t n,
                            void* out);
/* Host utility (no device work): Keccak-f[1600] on 25 little-endian 64-bit lanes - the permutation under the merlin
 * transcripts (STROBE-128) the aggregator draws its challenges from (distributed-prover/src/util.rs:22,41-75). */
void hk_keccak_f1600(uint64_t* state25);

/* The same for G1 along the GLV endomorphism phi(x, y) = (beta x, y) (phi(P) = [lambda] P, lambda^2 + lambda + 1 = 0 mod r):
 * out[i] = lo[i] + s_0 coeffs2[0] hi[i] + s_1 coeffs2[1] phi(hi[i]), c = s_0 coeffs2[0] + s_1 coeffs2[1] lambda mod r with two
 * ~128-bit parts - the folds `A' = A_L + c A_R`, `w' = w_L + c w_R` of a round.  128 doubling steps instead of 254.
 * The magnitude rule of hk_points_fold_g2 applies (here: 0x77..7 over 34 hex digits). */
hk_status hk_points_fold_g1(hk_ctx* ctx, const void* lo, const void* hi, const void* coeffs2_mont, unsigned neg_mask, size_t n,
                            void* out);
/* k <= 4 folds that share ONE scalar, as the folds of one GIPA round do (`A' = A_L + c A_R`, `w1' = ..`, `w2' = ..` with c;
 * `B'`, `v1'`, `v2'` with c^-1: ark-ip-proofs `gipa`, reached from distributed-prover/src/aggregation.rs:340 - there one rayon
 * sweep per vector): out[y][i] = lo[y][i] + c * hi[y][i], one launch and one normalisation for all k vectors.
 * lo, hi, out [h]: k pointers, each [h|d] to n packed affine points; coeffs / neg_mask (and the magnitude rule) as in
 * hk_points_fold_g1 / _g2. */
hk_status hk_points_fold_many_g1(hk_ctx* ctx, size_t k, const void* const* lo, const void* const* hi, const void* coeffs2_mont,
                                 unsigned neg_mask, size_t n, void* const* out);
hk_status hk_points_fold_many_g2(hk_ctx* ctx, size_t k, const void* const* lo, const void* const* hi, const void* coeffs4_mont,
                                 unsigned neg_mask, size_t n, void* const* out);

/* ---- MSM over a RESIDENT base set ----------------------------------------------------------------------
 * Bases that are key material (the KZG / commitment-key powers of the aggregator's SRS, any static query) are
 * uploaded once; long sets together with their 2^(16 g) multiples, exactly like the proving-key queries, so that every later
 * MSM over them has no Horner tail (the 254 sequential doublings that bound a one-off MSM's latency).  Short sets (G1 up to
 * 8 192 bases, G2 up to 2 048) stay as they are - hk_msm_bases runs n element-wise endomorphism products and one sum over
 * them, 1.4 - 2.4 ms - because building the multiples costs 6 - 10 ms per set and the aggregator multiplies each of its sets
 * once per aggregation (HK_BASES_TABLES=1 in the environment builds them for G1 sets of any length).
 * replaces `G::Group::msm(&srs_powers_alpha, &witness_poly.coeffs)` / `..beta..` of the KZG openings
 * (distributed-prover/src/kzg.rs:151-152) and the static-key MSMs of TIPA (distributed-prover/src/aggregation.rs:337,
 * third-party ripp) once the SRS of `TIPA::setup` (aggregation.rs:60-135) is resident.
 * group: 1 = G1, 2 = G2.  hk_msm_bases: same scalar conventions and length semantics as hk_msm_g1/g2
 * (checked != 0: n_scalars must equal the number of bases, else HK_ERR_LEN; unchecked: zip to the shorter). */
typedef struct hk_bases hk_bases;
hk_status hk_bases_upload(hk_ctx* ctx, int group, const void* bases, size_t n, hk_bases** out);
void      hk_bases_free(hk_bases* b);
hk_status hk_msm_bases(hk_ctx* ctx, const hk_bases* b, const void* scalars, size_t n_scalars, int mont,
                       int checked, void* out);

/* Montgomery <-> canonical conversion of n field elements (which: 0 = Fr, 1 = Fq; to_mont != 0: out = in*R mod p,
 * else out = in/R mod p; canonical input must be < p).  in/out are host or device pointers and may alias.
 * replaces ark-ff `into_bigint()` / `from_bigint()` as ark-serialize calls them for every field element of a key
 * file or response (mpi-snark/src/bin/node.rs:231-237 `ProvingKeys::deserialize_uncompressed_unchecked`;
 * mpi-snark/src/lib.rs:68-71 `serialize_to_vec`): the wire format is canonical little-endian, the ABI Montgomery. */
hk_status hk_field_convert(hk_ctx* ctx, int which, const void* in, void* out, size_t n, int to_mont);

/* ---- witness materialisation ------------------------------------------------------------------
 * A gadget circuit's assignment is almost entirely bits (SHA-256: > 99.99 %).  The witness generator hands over ONE
 * BYTE per variable plus the few full-width values, and the assignment `cs.full_assignment()` would hold
 * (cp-groth16/src/constraint_synthesizer.rs:102-106: instance || witness, 32 B Montgomery each) is materialised in
 * HBM: z[i] = bits[i] ? 1 : 0, then z[full_cols[k]] = full_vals[k].  PCIe carries n_v bytes instead of 32 n_v.
 * bits [h|d]: n_v bytes (0 / 1; bits[0] = 1 for the constant); full_cols [h|d]: n_full column indices;
 * full_vals_mont [h|d]: n_full Fr; z_out [d]: n_v Fr, ready for hk_commit / hk_prove. */
hk_status hk_assignment_from_bits(hk_ctx* ctx, const void* bits, size_t n_v, const uint32_t* full_cols,
                                  const void* full_vals_mont, size_t n_full, void* z_out);

/* Witness generation ON the device for gadget circuits: a class's WORD PROGRAM (the dataflow of its bit gadgets at
 * 32-bit word granularity, recorded when its R1CS is built) + column map are uploaded once; hk_wprog_run then turns the
 * inputs of `batch` subcircuits (a leaf's 16 words, the 54 bytes of two child hashes) into their full Montgomery
 * assignments in HBM - replaces the witness side of `circuit.generate_constraints` (cp-groth16/src/prover.rs:70-75;
 * distributed-prover/src/tree_hash_circuit.rs:313-398) for a re-implemented gadget set (csrc/witness.cuh).
 *   ops [h]: n_ops x 8 u32 (opcode, a, b, c, imm, 0, 0, 0): 0 INPUT imm | 1 CONST imm | 2 XOR a b | 3 CH a b c | 4 AND a b |
 *            5 MAJ a b c | 6 ADD refs[a .. a+b) + imm -> TWO values (low word, carry) | 7 PACK4 refs[a .. a+4) | imm;
 *            8 SHA_ROUND refs[a .. a+9) = (a b c d e f g h w), imm = K_t -> ELEVEN values, those of the round's gadget
 *            entries in their order (rotr6^rotr11 of e, Sigma1, Ch, rotr2^rotr13 of a, Sigma0, a & b, Maj, low / carry of
 *            d + h + Sigma1 + Ch + w + K, low / carry of h + Sigma1 + Ch + w + Sigma0 + Maj + K) | 9 SHA_SCHED
 *            refs[a .. a+4) = (w[t-15] w[t-2] w[t-7] w[t-16]) -> SIX values (rotr7^rotr18, sigma0, rotr17^rotr19, sigma1,
 *            low / carry of sigma1 + w[t-7] + sigma0 + w[t-16]);
 *            an operand = value id | rotate-right << 20 | shift-right << 25; every entry defines the next value id(s)
 *   map [h]: n_v u32, value id << 5 | bit position, or 0xffffffff for instance / full-width columns
 *   hk_wprog_run: inputs [h|d] batch x n_inputs u32; full_cols [h|d] n_full columns; full_vals_mont [h|d] batch x n_full Fr;
 *            z_out [d]: batch x n_v Fr.  HK_ERR_ARG for a program that would index out of range. */
typedef struct hk_wprog hk_wprog;
hk_status hk_wprog_upload(hk_ctx* ctx, const uint32_t* ops, size_t n_ops, const uint32_t* refs, size_t n_refs,
                          const uint32_t* map, size_t n_v, size_t n_values, size_t n_inputs, hk_wprog** out);
void      hk_wprog_free(hk_wprog* w);
hk_status hk_wprog_run(hk_ctx* ctx, const hk_wprog* w, const uint32_t* inputs, size_t batch, const uint32_t* full_cols,
                       const void* full_vals_mont, size_t n_full, void* z_out);
/* The full-width values alone: z_out[b][full_cols[j]] = full_vals[b][j] for b < batch.  A subcircuit's bit columns do not
 * depend on the round's challenges, its running evaluations do (distributed-prover/src/subcircuit_circuit.rs:206-231): a
 * worker may run hk_wprog_run with n_full = 0 while the first round is still in flight and hand these in afterwards. */
hk_status hk_assignment_scatter(hk_ctx* ctx, const uint32_t* full_cols, const void* full_vals_mont, size_t n_full, size_t batch,
                                size_t n_v, void* z_out);

/* The Poseidon membership block of a subcircuit's assignment (the witness side of `verify_membership`,
 * distributed-prover/src/subcircuit_circuit.rs:233-252, with the hashes of poseidon_util.rs:26-107): for `batch`
 * subcircuits at once, the S-box chains and round states of the leaf hash (rate 3 over the 4 leaf fields) and of the
 * `depth` two-to-one hashes along the path, plus per level (bit, sibling, left input), written to columns
 * [col0, col0 + block) of each subcircuit's assignment in HBM - the order of hekaton_system_amd/sha_circuit.py
 * `poseidon_path_trace`.  hk_poseidon_desc: width t = rate + 1 (<= 4), S-box exponent (5 or 17), full / partial rounds,
 * offset (in Fr elements) of its constants inside `consts_mont` = ark[(rf + rp)][t] then mds[t][t].
 *   consts_mont [h|d]; leaf_mont [h|d] batch x 4 Fr; siblings_mont [h|d] batch x depth Fr (bottom-up: the leaf's sibling
 *   first); leaf_index [h|d] batch u32; z_out [d] batch x n_v Fr.  HK_ERR_ARG for a block that would not fit n_v. */
typedef struct { uint32_t t, alpha, full_rounds, partial_rounds, consts_offset; } hk_poseidon_desc;
hk_status hk_poseidon_path(hk_ctx* ctx, const void* consts_mont, size_t n_consts, const hk_poseidon_desc* leaf_hash,
                           const hk_poseidon_desc* node_hash, const void* leaf_mont, const void* siblings_mont,
                           const uint32_t* leaf_index, size_t depth, size_t batch, size_t n_v, size_t col0, void* z_out);

/* ---- proving-key residency --------------------------------------------------------------
 * A key with matrices holds its H query in the coset's evaluation basis (hk_prove then runs four
 * transforms and no C pass; the upload transforms h_g once, seconds at m = 2^21); HK_H_BASIS=coeff in the environment of the
 * upload keeps the coefficient basis.  The proofs of the two forms are the same bytes. */
hk_status hk_pk_upload(hk_ctx* ctx, const hk_pk_desc* desc, hk_pk** out);
void      hk_pk_free(hk_pk* pk);

/* ---- fused per-subcircuit calls (the unit of work the metric counts) --------------------- */

/* CommitmentBuilder::commit arithmetic (cp-groth16/src/committer.rs:87-91):
 * com = msm(ck[stage], w_stage) + kappa * last_delta_g.  w_stage_mont [h|d]: n Fr; HK_ERR_LEN
 * unless n == ck_len[stage] (committer.rs:83 assert). com_affine_out [h]. */
hk_status hk_commit(hk_ctx* ctx, const hk_pk* pk, size_t stage,
                    const void* w_stage_mont, size_t n, const void* kappa_mont,
                    void* com_affine_out);
/* The same for `batch` subcircuits of one proving-key class in ONE call - what a worker does for the stage-0 requests of the
 * subcircuits it holds (distributed-prover/src/worker.rs:91-146 under mpi-snark/src/bin/node.rs:500-506: one rayon task per
 * subcircuit there): com[b] = msm(ck[stage], w[b]) + kappa[b] * last_delta_g.  w_mont [h|d]: batch x n Fr, row after row;
 * kappas_mont [h]: batch Fr; coms_affine_out [h]: batch G1.  Short stages (the 16 stage-0 witnesses of a big-merkle subcircuit)
 * run as one set of launches; long ones as `batch` hk_commit calls. */
hk_status hk_commit_batch(hk_ctx* ctx, const hk_pk* pk, size_t stage, const void* w_mont, size_t n, const void* kappas_mont,
                          size_t batch, void* coms_affine_out);

/* CPGroth16::prove_last_stage (prover.rs:78-155) followed by CommitmentBuilder::prove's
 * kappa correction (committer.rs:112-114), everything after constraint synthesis:
 *   z_mont [h|d]  full assignment instance||witness, n_v Fr Montgomery, z[0] = 1
 *   r_mont,s_mont [h] the two blinders (prover.rs:28-29)
 *   kappas_mont [h]   n_kappas = n_stages-1 commitment randomizers (committer.rs:110-113)
 * Outputs [h]: proof.a (G1), proof.b (G2), proof.c (G1), packed affine.
 * Concurrent calls coalesce: a call that passes the checks (HK_ERR_ARG for a NULL pointer, a key of another context or
 * one without QAP matrices; HK_ERR_LEN for n_v / n_kappas) queues behind the other calls of its context.  While fewer
 * than two coalesced chunks of the context run, a caller at once leads the oldest queued key's calls - up to
 * HK_PROVE_BATCH_CHUNK of them, its own among the candidates - through hk_prove_batch's lock-step pipeline; the others
 * wait without holding a lane and get their own outputs, the chunk's status and their share of its hk_timings
 * (batch_proofs tells how many proofs the chunk held).  A lone caller runs at once as a batch of one.  Every output is
 * byte-identical to the proof the call would get alone. */
hk_status hk_prove(hk_ctx* ctx, const hk_pk* pk, const void* z_mont, size_t n_v,
                   const void* r_mont, const void* s_mont,
                   const void* kappas_mont, size_t n_kappas,
                   void* proof_a_g1, void* proof_b_g2, void* proof_c_g1);

/* hk_prove for `batch` subcircuits of one proving-key class in ONE call - the stage-1 half of a worker's
 * compute_responses (mpi-snark/src/bin/node.rs:760-795: one task per subcircuit there).  Row b of every output is
 * byte-identical to
 *   hk_prove(ctx, pk, z + b*n_v, n_v, r + b, s + b, kappas + b*n_kappas, n_kappas, proofs_a + b, proofs_b + b, proofs_c + b)
 * (pointer arithmetic in elements):
 *   z_mont         [h|d] batch x n_v Fr, row after row (the layout hk_wprog_run / hk_assignment_scatter write)
 *   r_mont, s_mont [h]   batch Fr each
 *   kappas_mont    [h]   batch x n_kappas Fr, row after row
 *   proofs_a_g1 [h] batch G1, proofs_b_g2 [h] batch G2, proofs_c_g1 [h] batch G1 (packed affine)
 * Errors, for the batch as a whole and checked in this order: HK_ERR_ARG for a key of another context or one without
 * QAP matrices; HK_ERR_LEN when n_v or n_kappas does not match the key; batch == 0 then returns HK_OK and touches
 * nothing; HK_ERR_ARG for a NULL pointer (kappas only when n_kappas > 0).  A failed call leaves the lane usable.
 * The proofs run in lock-step: every stage of hk_prove (digit sorts, the bucket accumulation of each of the five
 * queries, the level / reduction tail, k_finish) is ONE launch for a whole chunk of proofs, each proof on its own
 * slice of the buffers, over the key's shared shift tables; the witness map runs one chain per proof.
 * Chunks: a batch is proven in consecutive chunks of at most HK_PROVE_BATCH_CHUNK proofs, and of fewer when a chunk's
 * scratch (hk_prove's per-proof device buffers times the chunk, DESIGN.md "Batched proving") would not fit in the
 * device's free memory plus the lane's own arena; a chunk is never smaller than one proof.
 * hk_timings after the call: total_ms spans the whole call, every phase figure is summed over the chunks (within a
 * chunk the queries overlap as in hk_prove); accum_kernel_launches counts the real k_msm_accum0<Fq> launches - four per
 * chunk (A, B1, L, H; the G2 query is not counted, as for hk_prove) - and accum_kernel_ms their summed kernel time;
 * batch_proofs is the chunk size.  hk_prove_batch does not pass through hk_prove's coalescer. */
#define HK_PROVE_BATCH_CHUNK 8
hk_status hk_prove_batch(hk_ctx* ctx, const hk_pk* pk, const void* z_mont, size_t n_v,
                         const void* r_mont, const void* s_mont, const void* kappas_mont, size_t n_kappas,
                         size_t batch, void* proofs_a_g1, void* proofs_b_g2, void* proofs_c_g1);

/* ---- CP-Groth16 proof verification (cp-groth16/src/verifier.rs) ------------------------------------------------- */

/* A verifying key (data_structures.rs:33-46), every point [h|d] packed affine: deltas_h[n_deltas] are the stage deltas
 * followed by delta_last; gamma_abc_g[n_abc] the input bases.  A proof of this key carries n_deltas - 1 commitments D
 * and n_abc - 1 public inputs. */
typedef struct {
    const void* alpha_g;
    const void* beta_h;
    const void* gamma_h;
    const void* deltas_h;
    size_t n_deltas;
    const void* gamma_abc_g;
    size_t n_abc;
} hk_vk_desc;

/* prepare_verifying_key (verifier.rs:7-18): uploads the key, computes e(alpha, beta) on the device and keeps the Miller
 * lines of -gamma and of every -delta_j (ark's G2Prepared), so that verification never runs them again.  HK_ERR_LEN for
 * n_deltas == 0 or n_abc == 0. */
hk_status hk_vk_prepare(hk_ctx* ctx, const hk_vk_desc* desc, hk_vk** out);
void      hk_vk_free(hk_vk* vk);
/* PreparedVerifyingKey.alpha_beta_gt in the GT layout of hk_multi_pairing (gt_out [h|d], hk_ctx_gt_bytes bytes) */
hk_status hk_vk_alpha_beta(const hk_vk* vk, void* gt_out);

#define HK_VERIFY_CHECK_POINTS 1u   /* validate A, B, C and every D first (ark AffineRepr::check) */
#define HK_VERDICT_REJECT    0      /* the verifier's equation fails */
#define HK_VERDICT_ACCEPT    1
#define HK_VERDICT_BAD_POINT 2      /* a proof point is off its curve or outside the prime-order subgroup */

/* verify_proof (verifier.rs:64-71) for n proofs of one key, one verdict byte each (HK_VERDICT_*):
 *   a, c [h|d] n G1; b [h|d] n G2; ds [h|d] n x (n_deltas - 1) G1, row after row; inputs_mont [h|d] n x (n_abc - 1) Fr
 *   (Montgomery), row after row; verdicts [h|d] n bytes.
 * rand_mont == NULL: per-proof mode, the exact equation of every proof.  rand_mont [h|d]: n nonzero Fr (Montgomery),
 * batch mode: one randomised equation
 *   prod e(r_i A_i, B_i) e(sum r_i IC_i, -gamma) prod_j e(sum r_i D_ij, -delta_j) e(sum r_i C_i, -delta_last)
 *     == e(alpha, beta)^(sum r_i)
 * per chunk of proofs; all verdicts are 1 when it holds, else that chunk is verified per proof.  An r_i == 0 would drop
 * proof i from both sides, so a chunk that holds one is verified per proof as well (the entry looks; no verdict becomes 2).
 * The r_i must be drawn after the proofs are fixed: a prover who knows them can make wrong proofs cancel.  Batch mode requires
 * HK_VERIFY_CHECK_POINTS (HK_ERR_ARG otherwise).  A pair with a member at infinity contributes 1; infinity passes the
 * point check.  Returns HK_OK whatever the verdicts; n == 0 does nothing. */
hk_status hk_verify_batch(hk_ctx* ctx, const hk_vk* vk, const void* a_g1, const void* b_g2, const void* c_g1,
                          const void* ds_g1, const void* inputs_mont, size_t n, unsigned flags, const void* rand_mont,
                          uint8_t* verdicts);
/* ok[i] = 1 when points[i] is on its curve and in the prime-order subgroup (or infinity), else 0 (ark's AffineRepr::check,
 * what deserialize_* with Validate::Yes runs).  points [h|d] n packed affine, ok [h|d] n bytes. */
hk_status hk_points_check_g1(hk_ctx* ctx, const void* points, size_t n, uint8_t* ok);
hk_status hk_points_check_g2(hk_ctx* ctx, const void* points, size_t n, uint8_t* ok);

/* ---- compressed points (ark-serialize's second wire form: x and a sign flag, half the bytes) ---------------------------
 * Every array is [h|d]; calls are thread-safe on a shared context.  HK_ERR_ARG, with nothing written, for: a NULL pointer
 * with n > 0, `which` outside {1, 2}, n >= 2^31, an input range that shares a byte with an output range (or two outputs that
 * do).  n == 0 is HK_OK and writes nothing.
 *
 * hk_field_sqrt: square roots in the coordinate fields (which: 1 = Fq, 2 = Fq2; both curves have q = 3 mod 4).  in_mont n
 * elements (Montgomery); out_mont[i] = the root r of in[i] that is not larger than -r, or zero where in[i] is no square;
 * ok[i] = 1 / 0.  "Larger" is ark's order, on canonical values: r > (q - 1) / 2 in Fq; in Fq2 decided on c1 unless c1 == 0,
 * then on c0.  Fr is out of scope: its two-adicity is 28, so its roots need Tonelli-Shanks, and nothing on the wire needs them.
 *
 * hk_points_decompress_g1 / _g2 replace ark-ec's `get_point_from_x_unchecked` + `SWFlags` under `deserialize_compressed`
 * (and, with check != 0, the `check()` of its Validate::Yes form):
 *   x_canon n coordinates, canonical little-endian (G2: c0 || c1); flags n bytes, bit 0 = infinity, bit 1 = y is the larger of
 *   (y, -y); points_out n packed affine Montgomery points - y the root of x^3 + b the flag names, infinity all zeros;
 *   status n bytes: 1 ok | 0 x is not below q or x^3 + b is no square (the point is zeros) | 2 - only when check != 0 - on the
 *   curve but outside the prime-order subgroup (the point is still written).
 * hk_points_compress_g1 / _g2 are the inverse and replace `SWFlags::from_y_coordinate` + the x of `serialize_compressed`:
 *   points n packed affine -> x_canon_out, flags_out as above.  No curve check: y only decides the flag. */
hk_status hk_field_sqrt(hk_ctx* ctx, int which, const void* in_mont, size_t n, void* out_mont, uint8_t* ok);
hk_status hk_points_decompress_g1(hk_ctx* ctx, const void* x_canon, const uint8_t* flags, size_t n, int check,
                                  void* points_out, uint8_t* status);
hk_status hk_points_decompress_g2(hk_ctx* ctx, const void* x_canon, const uint8_t* flags, size_t n, int check,
                                  void* points_out, uint8_t* status);
hk_status hk_points_compress_g1(hk_ctx* ctx, const void* points, size_t n, void* x_canon_out, uint8_t* flags_out);
hk_status hk_points_compress_g2(hk_ctx* ctx, const void* points, size_t n, void* x_canon_out, uint8_t* flags_out);

/* ---- trusted setup past synthesis (cp-groth16/src/generator.rs:66-224) ---------------------------------------------
 * Both entries take the class's matrices in the hk_csr form of hk_witness_map / hk_pk_upload ([h|d]).  Errors, checked in
 * this order: HK_ERR_DOMAIN_TOO_LARGE when log2(m) exceeds the curve's two-adicity (from the sizes alone, before any array
 * is read); HK_ERR_ARG for a NULL required pointer, a matrix with n_rows != n_constraints, n_v, an nnz or m >= 2^32,
 * n_inst == 0 or > n_v (hk_keygen also: stage ranges that do not tile [0, n_v - n_inst) in order, a zero gamma or delta);
 * then, found on the device: HK_ERR_ARG for a column index >= n_v or a row_ptr that decreases or does not end at nnz, and
 * HK_ERR_ARG for t in the domain (zt = 0; generator.rs:68 never draws one).  hk_keygen writes no point output unless all
 * of these pass; the contents of hk_qap_eval's outputs after a failed call are undefined.  A failed call leaves the lane
 * usable. */

/* LibsnarkReduction::instance_map_with_evaluation (cp-groth16/src/generator.rs:75-76): a_j = sum_i A_ij u_i(t) + u_(n_c+j)(t)
 * for j < n_inst, b_j and c_j likewise without the instance rows, u_i the Lagrange coefficients of the domain of size m
 * (the next power of two >= n_constraints + n_inst) at t.  t_mont [h]: 1 Fr; a/b/c_out [h|d]: n_v Fr (Montgomery);
 * zt_out [h]: t^m - 1 (1 Fr, Montgomery); *m_out = m (m_out may be NULL). */
hk_status hk_qap_eval(hk_ctx* ctx, const hk_csr* A, const hk_csr* B, const hk_csr* C, size_t n_inst,
                      size_t n_constraints, size_t n_v, const void* t_mont,
                      void* a_out, void* b_out, void* c_out, void* zt_out, size_t* m_out);

/* The toxic waste and the class: every Fr [h], 1 element each, Montgomery. */
typedef struct {
    const hk_csr *A, *B, *C;
    size_t n_inst, n_constraints, n_v;
    const uint64_t* stage_ranges; size_t n_stages;   /* [h] [begin, end) per stage over witness indices, in order */
    const void *alpha, *beta, *gamma, *t, *g1_scalar, *g2_scalar;
    const void* deltas;                               /* n_stages Fr */
} hk_keygen_desc;

/* Where the key goes: every pointer [h|d], packed affine; layouts = ProvingKey (cp-groth16/src/data_structures.rs:66-83). */
typedef struct {
    void *a_g, *b_g, *b_h, *h_g;      /* n_v G1, n_v G1, n_v G2, m - 1 G1 (h_g may be NULL when m == 1) */
    void* const* ck_stage;            /* [h] n_stages pointers; stage k: (end - begin) G1 (NULL allowed for an empty stage) */
    void *deltas_g, *alpha_g, *beta_g, *gamma_abc_g;   /* n_stages, 1, 1, n_inst G1 */
    void *beta_h, *gamma_h, *deltas_h;                 /* 1, 1, n_stages G2 */
    void* qap_abc;                    /* optional (NULL: not written): 3 n_v Fr, a | b | c at t, Montgomery */
} hk_keygen_out;

/* generate_parameters past synthesis (generator.rs:66-224): the QAP at t (as hk_qap_eval), every scalar of the key -
 * (beta a_i + alpha b_i + c_i) / delta_k over stage k's witness range, / gamma over the instance, zt t^i / delta_last for
 * i < m - 1 - and every fixed-base sweep over the standard generators times g1_scalar / g2_scalar, without a host round
 * trip: a_g = a_i g1s G1, b_g = b_i g1s G1, b_h = b_i g2s G2, h_g, ck, gamma_abc_g, alpha_g = alpha g1s G1, beta_g,
 * deltas_g = delta_k g1s G1, beta_h = beta g2s G2, gamma_h, deltas_h.  *m_out = m (may be NULL).  The sweeps share the
 * context's window-table cache with hk_fixed_base_g1 / _g2.  Errors: see above. */
hk_status hk_keygen(hk_ctx* ctx, const hk_keygen_desc* desc, const hk_keygen_out* out, size_t* m_out);

/* ---- the coordinator between the two rounds (distributed-prover/src/coordinator.rs:125-174, 425-466) ---------------
 * Once the stage-0 commitments are hashed to the challenges, `generate_exec_tree` threads the running evaluations through
 * every subtrace (transcript/mod.rs:85-132: eval *= tr_chal - repr(entry)), forms one leaf per subcircuit
 * (eval_tree.rs:53-101) and builds the Poseidon Merkle tree over them; `CoordinatorStage1State::new` then takes one
 * `generate_proof` path per subcircuit.  hk_exec_tree does all of it in one call from the two flattened traces:
 *   factor of an entry f     tr_chal - (f[1] + c0 f[0] [+ c1 f[2] + c2 f[3]])   (rom_transcript.rs:84-86, ram :109-112)
 *   evaluation i             product of the factors of entries [0, offsets[i + 1]), from 1, per order
 *   leaf i                   (time eval, addr eval, last entry): the last entry is entry offsets[i + 1] - 1 of the address
 *                            order, all zero when offsets[i + 1] == 0 (`padding()`); an empty subtrace carries the previous
 *                            one over (coordinator.rs:137-160)
 *   leaf digest              the rate-3 sponge over the 2 + entry_fields leaf fields (two permutations), inner node = the
 *                            two-to-one hash of its children (poseidon_util.rs:26-107)
 * The address sort (coordinator.rs:92-123) does not depend on the challenges: hk_trace_sort (below) makes the address-ordered
 * trace on the device from the time-ordered one, before or without this call.  siblings_mont and
 * leaves_mont are what hk_poseidon_path takes as they are (ROM).  HK_ERR_ARG, before any device work and with the outputs
 * untouched: n_sub not a power of two or 1, entry_fields not 2 / 4, offsets[0] != 0 or decreasing offsets, a descriptor
 * other than the compiled (t 4, alpha 5) leaf / (t 3, alpha 17) node pair, constants that end before its tables do. */
typedef struct {
    uint32_t n_sub;                 /* leaves = subcircuits; a power of two >= 2 (ark MerkleTree::new) */
    uint32_t entry_fields;          /* 2 = ROM (addr, val); 4 = RAM (addr, val, timestamp, is_read): to_field_elements() order */
    const uint32_t* offsets;        /* [h] n_sub + 1; offsets[0] = 0, non-decreasing: subtrace i = entries [offsets[i], offsets[i+1]) of BOTH orders */
    const void* time_entries_mont;  /* [h|d] offsets[n_sub] x entry_fields Fr */
    const void* addr_entries_mont;  /* [h|d] same shape, address-ordered */
    const void* challenges_mont;    /* [h] entry_fields Fr in the reference's challenges() order: entry challenge(s), then tr_chal */
    const void* consts_mont; size_t n_consts;             /* as hk_poseidon_path */
    const hk_poseidon_desc* leaf_hash; const hk_poseidon_desc* node_hash;
} hk_exec_tree_desc;
typedef struct {                    /* every pointer [h|d]; evals / nodes may be NULL */
    void* evals_mont;               /* n_sub x 2 Fr: (time, addr) evaluation AFTER subcircuit i */
    void* leaves_mont;              /* n_sub x (2 + entry_fields) Fr: ExecTreeLeaf::to_field_elements (eval_tree.rs:81-94) */
    void* nodes_mont;               /* 2 n_sub - 1 Fr: leaf digests, then each level, root last */
    void* siblings_mont;            /* n_sub x depth Fr, bottom-up: hk_poseidon_path's `siblings_mont` as is */
    void* root_mont;                /* 1 Fr */
} hk_exec_tree_out;
hk_status hk_exec_tree(hk_ctx* ctx, const hk_exec_tree_desc* desc, const hk_exec_tree_out* out);

/* ---- a subcircuit's challenge-dependent witness (distributed-prover/src/subcircuit_circuit.rs:206-252) -------------
 * A stage-1 assignment has the bit columns of its gadgets (hk_wprog_run; no challenge in them) and the columns that wait for
 * the round's challenges: what `generate_constraints` witnesses from its Stage1Request (coordinator.rs:569-604: the
 * challenges, the previous leaf's evaluations and last entry, the membership path of its own leaf, the root).  hk_exec_tree
 * computes every one of those values; hk_stage1_witness writes them into the assignments of any subset of the job's
 * subcircuits, from hk_exec_tree's inputs and outputs where they lie (ROM entries; hk_ram_stage1_witness below is the RAM form).  Row b of z_out is the assignment of
 * subcircuit i = sub_index[b]; indices may come in any order and may repeat.  With k = n_portals:
 *   inst_col0 + 0 .. 2     entry_chal, tr_chal, root
 *   col0 ..                (addr, val) of the k time-ordered entries, then of the k address-ordered ones        4 k
 *                          time chain: evals[i - 1][0] (1 for i = 0), then per entry e = val + entry_chal addr
 *                          and cur <- cur (tr_chal - e)                                                         1 + 2 k
 *                          address chain, the same from evals[i - 1][1]                                         1 + 2 k
 *                          the previous leaf's last address-ordered entry: entry offsets[i] - 1, (0, 0) when
 *                          offsets[i] == 0                                                                      2
 *                          per consecutive pair of [previous] + address entries, d = addr' - addr: inv = 1 / d
 *                          (0 when d = 0), same = [d == 0]                                                      2 k
 *   pos_col0 ..            the membership block of leaf leaves[i], path siblings[i], index i: the values and order of
 *                          hk_poseidon_path
 * - the columns hekaton_system_amd/sha_circuit.py `ShaMerkleSubcircuit._program` allocates.  Every other column of z_out keeps
 * its bytes, column 0 included.  The call runs on the caller's lane; host-resident inputs are staged in lane scratch, device-
 * resident ones are read in place.  batch == 0: HK_OK, nothing done.  HK_ERR_ARG, before any device work and with z_out
 * untouched: a NULL pointer; n_sub not a power of two >= 2 or depth != log2(n_sub); n_portals == 0; offsets[0] != 0 or
 * decreasing offsets; sub_index[b] >= n_sub; a selected subcircuit that does not own exactly n_portals entries; a descriptor
 * pair other than the compiled (t 4, alpha 5) / (t 3, alpha 17), constants that end before its tables do; one of the three
 * column ranges not inside [1, n_v) or two of them overlapping (the membership block's length as hk_poseidon_path computes
 * it); batch >= 2^20 or (7 + 5 k) batch >= 2^31. */
typedef struct {
    uint32_t n_sub;                 /* subcircuits of the job = rows of evals / leaves / siblings; power of two >= 2 */
    uint32_t n_portals;             /* k >= 1: entries a subcircuit of this class owns in EACH order */
    uint32_t depth;                 /* log2(n_sub) */
    const uint32_t* offsets;        /* [h] n_sub + 1, as hk_exec_tree */
    const void* time_entries_mont;  /* [h|d] offsets[n_sub] x 2 Fr (addr, val): hk_exec_tree's inputs, entry_fields = 2 */
    const void* addr_entries_mont;  /* [h|d] same shape, address order */
    const void* challenges_mont;    /* [h] 2 Fr: entry_chal, tr_chal */
    const void* evals_mont;         /* [h|d] n_sub x 2 Fr      } */
    const void* leaves_mont;        /* [h|d] n_sub x 4 Fr      } exactly what hk_exec_tree wrote */
    const void* siblings_mont;      /* [h|d] n_sub x depth Fr  } */
    const void* root_mont;          /* [h|d] 1 Fr              } */
    const void* consts_mont; size_t n_consts;
    const hk_poseidon_desc* leaf_hash; const hk_poseidon_desc* node_hash;   /* as hk_poseidon_path / hk_exec_tree */
    uint32_t inst_col0;             /* columns inst_col0 .. +2 <- entry_chal, tr_chal, root */
    uint32_t col0;                  /* first column of the portal block (10 k + 4 columns, order above) */
    uint32_t pos_col0;              /* first column of the membership block (hk_poseidon_path's col0) */
} hk_stage1_desc;
hk_status hk_stage1_witness(hk_ctx* ctx, const hk_stage1_desc* desc, const uint32_t* sub_index /* [h] batch */,
                            size_t batch, size_t n_v, void* z_out /* [d] batch x n_v Fr */);

/* ---- the address-ordered trace (distributed-prover/src/coordinator.rs:92-123 `sort_subtraces_by_addr`) ---------------
 * The coordinator flattens the time-ordered subtraces, sorts them with Rust's stable sort_by_key - by addr as a u64 for ROM
 * (coordinator.rs:104), by (addr u64, timestamp u32) compared lexicographically for RAM (coordinator.rs:107) - and cuts the
 * result into chunks of the same lengths.  Both orders share one `offsets`, so re-chunking is the identity on the flat
 * array and hk_trace_sort takes no offsets: addr_entries_mont_out is the stable sort of the n_entries flattened entries by
 * that key, in hk_exec_tree's layout (entry_fields Montgomery Fr per entry, to_field_elements() order: field 0 the address,
 * for RAM field 2 the timestamp).  Entries of equal key keep their time order; val and is_read are payload and never
 * compared.  perm_out (may be NULL): address-ordered entry j = time-ordered entry perm_out[j].  The result is the same from
 * run to run, byte for byte.  The call runs on the caller's lane; a host-resident input is staged in lane scratch, a device-
 * resident one is read in place; the outputs are copied out of scratch last, so a refused or failed call leaves them
 * untouched.  n_entries == 0: HK_OK, nothing done.  HK_ERR_ARG before any device work: entry_fields not 2 / 4,
 * n_entries >= 2^31, a NULL input or addr_entries_mont_out, an output range that overlaps the input range.  HK_ERR_ARG found
 * on the device, outputs untouched: an address >= 2^64 or a timestamp >= 2^32 (neither is a value of the reference's
 * types). */
hk_status hk_trace_sort(hk_ctx* ctx, uint32_t entry_fields,             /* 2 = ROM (addr, val); 4 = RAM (addr, val, timestamp, is_read) */
                        const void* time_entries_mont, size_t n_entries, /* [h|d] n_entries x entry_fields Fr */
                        void* addr_entries_mont_out,                     /* [h|d] same shape */
                        uint32_t* perm_out);                             /* [h|d] n_entries, or NULL */

/* ---- a subcircuit's stage-0 witness (distributed-prover/src/worker.rs:91-146 `process_stage0_request`) ----------------
 * Row b of w_out is the stage-0 witness of subcircuit i = sub_index[b] (any order, repeats allowed): (addr, val) of its
 * n_portals time-ordered entries, then of its n_portals address-ordered entries - entries [offsets[i], offsets[i + 1]) of
 * each trace, two contiguous copies; the variable order of hekaton_system_amd/sha_circuit.py `ShaMerkleJob.stage0_ints` /
 * `ShaMerkleSubcircuit._program`.  w_out is what hk_commit_batch takes as w_mont [d].  ROM entries only, as
 * hk_stage1_witness (RAM: hk_ram_stage0_witness).  Host-resident traces are staged in lane scratch, device-resident ones are read in place.
 * batch == 0: HK_OK, nothing done.  HK_ERR_ARG, before any device work and with w_out untouched: a NULL pointer;
 * n_portals == 0; offsets[0] != 0 or decreasing offsets; sub_index[b] >= n_sub; a selected subcircuit that does not own
 * exactly n_portals entries; w_out not in device memory; batch >= 2^20 or batch x n_portals >= 2^28. */
hk_status hk_stage0_witness(hk_ctx* ctx, const uint32_t* offsets /* [h] n_sub + 1 */, uint32_t n_sub, uint32_t n_portals,
                            const void* time_entries_mont, const void* addr_entries_mont,   /* [h|d] offsets[n_sub] x 2 Fr */
                            const uint32_t* sub_index /* [h] batch */, size_t batch,
                            void* w_out /* [d] batch x 4 n_portals Fr */);

/* ---- R1CS satisfaction of device-resident assignments (ark `cs.is_satisfied()` / `which_is_unsatisfied()`:
 * cp-groth16/src/lib.rs:158,291; distributed-prover/src/subcircuit_circuit.rs:311-399) -------------------------------------
 * For each of `batch` assignments (row b at z_mont + b * n_v Fr, host or device; a device one is read in place) every row i of
 * the class's matrices is tested: <A_i,z> * <B_i,z> == <C_i,z> on canonical values.  verdicts[b] says how many rows fail and
 * which is the first.  With bad_rows and cap > 0, bad_rows[b] holds the first min(n_bad, cap) failing rows in ascending order
 * and 0xFFFFFFFF in every further slot; with bad_vals as well, the three dot products (a, b, c) of exactly those rows,
 * canonical Montgomery, and zeros in the unused slots.  cap == 0 or bad_rows == NULL: verdicts only.  Every byte of every
 * output is defined and a function of the inputs alone (no value depends on the order in which anything lands).
 * batch == 0: HK_OK, nothing done.  HK_ERR_ARG, before any launch and with the outputs untouched: a NULL context or matrix;
 * NULL z_mont or verdicts with batch > 0; unequal n_rows; n_rows >= 2^32 or n_v >= 2^32; bad_vals without bad_rows;
 * n_v == 0 (a row of z has column 0); batch >= 2^31 or batch x cap >= 2^31.  hk_r1cs_check validates the matrices against n_v
 * as hk_witness_map does (a malformed one: HK_ERR_ARG, outputs untouched).  hk_pk_r1cs_check uses the matrices the key was
 * uploaded with, nothing re-uploaded or re-validated: HK_ERR_ARG for a key of another context or one uploaded without matrices,
 * HK_ERR_LEN (as hk_prove) when n_v is not the key's. */
typedef struct {
    uint32_t n_bad;      /* rows i with <A_i,z> * <B_i,z> != <C_i,z>                          */
    uint32_t first_bad;  /* the smallest such i; 0xFFFFFFFF when n_bad == 0                   */
} hk_r1cs_verdict;       /* cs.is_satisfied() <=> n_bad == 0; which_is_unsatisfied() <=> first_bad */
hk_status hk_r1cs_check(hk_ctx* ctx, const hk_csr* A, const hk_csr* B, const hk_csr* C,
                        const void* z_mont /* [h|d] batch x n_v Fr */, size_t n_v, size_t batch,
                        hk_r1cs_verdict* verdicts /* [h] batch */,
                        uint32_t* bad_rows /* [h|d] batch x cap, may be NULL */,
                        void* bad_vals    /* [h|d] batch x cap x 3 Fr (a, b, c; Montgomery), may be NULL */,
                        size_t cap);
hk_status hk_pk_r1cs_check(hk_ctx* ctx, const hk_pk* pk, const void* z_mont, size_t n_v, size_t batch,
                           hk_r1cs_verdict* verdicts, uint32_t* bad_rows, void* bad_vals, size_t cap);

/* ---- the big-merkle job's data tree and time-ordered trace (distributed-prover/src/tree_hash_circuit.rs:313-470
 * `MerkleTreeCircuit::get_portal_subtraces`) ---------------------------------------------------------------------------------
 * The head of a job's chain: from the n_sub / 2 leaves of 64 bytes to the tree of iterated SHA-256 hashes and the ROM trace
 * every later call reads (hekaton_system_amd/sha_circuit.py `ShaMerkleJob`).  Subcircuit order: leaves 0 .. n_sub / 2 - 1,
 * parents level by level (the level of width w starts at subcircuit n_sub - 2 w; node k of it has the children 2 k and
 * 2 k + 1 of the level below), the root at n_sub - 2, the padding subcircuit at n_sub - 1.
 *   digest of a leaf        SHA-256 applied ns times to its 64 bytes (every application after the first hashes a 32-byte digest)
 *   digest of the padding   the same over 64 zero bytes
 *   digest of a parent      SHA-256 applied ns times to the first 27 bytes of its left child's digest followed by the first
 *                           27 of its right child's (54 bytes)
 *   val(j)                  bytes 0 .. 26 of digest j read as a little-endian integer (216 bits: below r on both curves)
 * time_entries_mont_out holds n_portals (addr, val) entries per subcircuit, address 0 the placeholder portal (0, 0),
 * address 1 + j the hash of node j:
 *   leaf i      placeholders, then (1 + i, val(i))              root      (1 + l, val(l)), (1 + r, val(r)), placeholders
 *   parent j    (1 + l, val(l)), (1 + r, val(r)), placeholders, then (1 + j, val(j))      padding   placeholders only
 * - what hk_trace_sort, hk_exec_tree and hk_stage0_witness take as time_entries_mont with offsets[i] = i n_portals.  The
 * result is the same from run to run, byte for byte.  The call runs on the caller's lane; host-resident leaves are staged in
 * lane scratch, device-resident ones are read in place; the outputs are copied out of scratch last, so a refused or failed
 * call leaves them untouched.  HK_ERR_ARG, before any device work and with the outputs untouched: a NULL context, leaves or
 * out, or all three outputs NULL; n_sub not a power of two in [4, 2^20]; ns == 0 or ns >= 2^16; n_portals < 3;
 * n_sub x n_portals >= 2^28; an output range that overlaps the leaves. */
typedef struct {                 /* every pointer [h|d]; any may be NULL, not all three */
    void* digests_out;           /* n_sub x 32 B, hashlib's byte order, subcircuit order, padding last */
    void* time_entries_mont_out; /* n_sub * n_portals x 2 Fr: hk_trace_sort / hk_exec_tree / hk_stage0_witness input */
    void* sha_root_mont_out;     /* 1 Fr: val(n_sub - 2), the data tree's root (a witness of the root class) */
} hk_sha_tree_out;
hk_status hk_sha_tree(hk_ctx* ctx, const void* leaves /* [h|d] n_sub/2 x 64 B */, uint32_t n_sub, uint32_t ns,
                      uint32_t n_portals, const hk_sha_tree_out* out);

/* The word-program inputs (hk_wprog_run's `inputs`) of any subcircuits of ONE kind, row b for subcircuit sub_index[b] (any
 * order, repeats allowed) - hekaton_system_amd/sha_circuit.py `program_inputs`:
 *   n_inputs 16   a leaf (i < n_sub / 2): its 64 bytes as 16 big-endian words; the padding subcircuit (n_sub - 1): 16 zeros
 *   n_inputs 54   a parent or the root (n_sub / 2 <= i <= n_sub - 2): the first 27 bytes of its left child's digest, then of
 *                 its right child's, one byte per word
 * leaves may be NULL when n_inputs == 54, digests (hk_sha_tree's digests_out) when n_inputs == 16.  Staging, lane and output
 * as hk_sha_tree.  batch == 0: HK_OK, nothing done.  HK_ERR_ARG, before any device work and with inputs_out untouched: a NULL
 * context, sub_index or inputs_out; n_sub not a power of two in [4, 2^20]; n_inputs not 16 / 54; the input n_inputs needs
 * NULL; a sub_index[b] of the other kind or >= n_sub; batch >= 2^20; inputs_out overlapping an input range. */
hk_status hk_sha_tree_inputs(hk_ctx* ctx, const void* leaves /* [h|d], may be NULL when n_inputs == 54 */,
                             const void* digests /* [h|d] n_sub x 32 B, may be NULL when n_inputs == 16 */,
                             uint32_t n_sub, uint32_t n_inputs /* 16 | 54 */,
                             const uint32_t* sub_index /* [h] batch */, size_t batch,
                             uint32_t* inputs_out /* [h|d] batch x n_inputs */);

/* ---- the witness of a RAM portal subcircuit (distributed-prover/src/portal_manager/ram_portal_manager.rs:150-230,
 * transcript/ram_transcript.rs:260-390, subcircuit_circuit.rs:166-273; the VM job of vm/vm_constraints.rs) ------------------
 * The RAM siblings of hk_stage0_witness and hk_stage1_witness: they read hk_trace_sort's and hk_exec_tree's entry_fields = 4
 * layout (addr, val, timestamp, is_read per entry) and write the columns hekaton_system_amd/vm_circuit.py
 * `RamSubcircuit._program` allocates.  An entry takes 35 columns: val, addr, timestamp bit 0 .. 31 (least significant
 * first), read.  Row b is subcircuit i = sub_index[b]; indices may come in any order and may repeat.  With k = n_portals:
 *   stage 0                the k time-ordered entries, then the k address-ordered ones                          70 k
 *   inst_col0 + 0 .. 4     entry_chal_1, entry_chal_2, entry_chal_3, tr_chal, root
 *   col0 ..                the previous leaf's last address-ordered entry: entry offsets[i] - 1, all zero when
 *                          offsets[i] == 0                                                                      35
 *                          time chain: evals[i - 1][0] (1 for i = 0), then per entry p1 = c1 addr, p2 = c2 ts,
 *                          e = val + p1 + p2 + c3 read and cur <- cur (tr_chal - e)                              1 + 4 k
 *                          address chain, the same from evals[i - 1][1]                                         1 + 4 k
 *                          per consecutive pair of [previous] + address entries, d = addr' - addr: inv = 1 / d
 *                          (0 when d = 0), same = [d == 0], sr = same read', then bit 0 .. 31 of
 *                          ts' - ts - 1 (mod 2^32) when same, else 32 zeros                                     35 k
 *   pos_col0 ..            the membership block of leaf leaves[i] (six fields), path siblings[i], index i: the values and
 *                          order of hk_poseidon_path
 * hk_ram_stage0_witness writes the 70 k stage-0 columns alone, as rows of 70 k Fr: what hk_commit_batch takes as w_mont [d].
 * hk_ram_stage1_witness writes a whole assignment row in one call: when template_mont is non-NULL every row of z_out is first
 * set to it (n_v Fr: column 0 and whatever is the same for every subcircuit of the class); then the instance values, the
 * stage-0 columns at stage0_col0, the portal block and the membership block.  Every other column keeps its bytes, or the
 * template's.  Both calls run on the caller's lane; host-resident inputs are staged in lane scratch, device-resident ones are
 * read in place.  batch == 0: HK_OK, nothing done.  HK_ERR_ARG, before any device work and with the output untouched: a NULL
 * pointer (template_mont excepted); n_portals == 0; offsets[0] != 0 or decreasing offsets; sub_index[b] >= n_sub; a selected
 * subcircuit that does not own exactly n_portals entries; the output not in device memory; hk_ram_stage1_witness also:
 * n_sub not a power of two >= 2 or depth != log2(n_sub); a descriptor pair other than the compiled (t 4, alpha 5) /
 * (t 3, alpha 17), constants that end before its tables do; one of the four column ranges not inside [1, n_v) or two of
 * them overlapping.  Lane counts: every kernel of the two calls indexes its lanes with 64 bits and is launched as
 * ceil(lanes / 256) blocks, at most batch x max(40 + 105 k, n_v) lanes, so the calls refuse k > 2^16, batch >= 2^20,
 * batch x (40 + 105 k) >= 2^38 and batch x n_v >= 2^38 (below 2^30 blocks).  HK_ERR_ARG found on the device, the output
 * untouched: in a SELECTED subcircuit a timestamp >= 2^32 or a read flag other than 0 / 1 (neither is a value of the
 * reference's types); such a value elsewhere in the traces is not looked at. */
hk_status hk_ram_stage0_witness(hk_ctx* ctx, const uint32_t* offsets /* [h] n_sub + 1 */, uint32_t n_sub, uint32_t n_portals,
                                const void* time_entries_mont, const void* addr_entries_mont,   /* [h|d] offsets[n_sub] x 4 Fr */
                                const uint32_t* sub_index /* [h] batch */, size_t batch,
                                void* w_out /* [d] batch x 70 n_portals Fr */);
typedef struct {
    uint32_t n_sub;                 /* subcircuits of the job = rows of evals / leaves / siblings; power of two >= 2 */
    uint32_t n_portals;             /* k >= 1: entries a subcircuit of this class owns in EACH order */
    uint32_t depth;                 /* log2(n_sub) */
    const uint32_t* offsets;        /* [h] n_sub + 1, as hk_exec_tree */
    const void* time_entries_mont;  /* [h|d] offsets[n_sub] x 4 Fr (addr, val, timestamp, is_read): hk_exec_tree's inputs */
    const void* addr_entries_mont;  /* [h|d] same shape, address order */
    const void* challenges_mont;    /* [h] 4 Fr: entry_chal_1, entry_chal_2, entry_chal_3, tr_chal */
    const void* evals_mont;         /* [h|d] n_sub x 2 Fr      } */
    const void* leaves_mont;        /* [h|d] n_sub x 6 Fr      } exactly what hk_exec_tree wrote with entry_fields = 4 */
    const void* siblings_mont;      /* [h|d] n_sub x depth Fr  } */
    const void* root_mont;          /* [h|d] 1 Fr              } */
    const void* consts_mont; size_t n_consts;
    const hk_poseidon_desc* leaf_hash; const hk_poseidon_desc* node_hash;   /* as hk_poseidon_path / hk_exec_tree */
    const void* template_mont;      /* [h|d] n_v Fr, or NULL: every row of z_out starts as a copy of it */
    uint32_t inst_col0;             /* columns inst_col0 .. +4 <- the four challenges, root */
    uint32_t stage0_col0;           /* first of the 70 k stage-0 columns */
    uint32_t col0;                  /* first column of the portal block (43 k + 37 columns, order above) */
    uint32_t pos_col0;              /* first column of the membership block (hk_poseidon_path's col0) */
} hk_ram_stage1_desc;
hk_status hk_ram_stage1_witness(hk_ctx* ctx, const hk_ram_stage1_desc* desc, const uint32_t* sub_index /* [h] batch */,
                                size_t batch, size_t n_v, void* z_out /* [d] batch x n_v Fr */);

/* ---- the partitioned R1CS job (distributed-prover/src/partitioned_r1cs_circuit.rs:116-220; portal_manager/
 * rom_portal_manager.rs:34-117 `SetupRomPortalManager`) ----------------------------------------------------------------------
 * A circom R1CS cut into P partitions that exchange their shared wires through ROM portals, repeated over T transactions
 * (hekaton_system_amd/r1cs_circuit.py `PartitionedR1csJob`): subcircuit i is partition i % P of transaction i / P.  The
 * descriptor states the job once.  A transaction's witness block is the P partitions' witnesses back to back, wire order as
 * the reference's (wire 0 the constant, the partition's own wires, its owned ones, its borrowed ones); transaction g reads
 * the block at g * tx_stride Fr of witness_mont, or block 0 when tx_stride == 0.  A partition's portal slots are, in time
 * order, its owned `set`s, its borrowed `get`s and, in a one-partition job, the dummy `set`; slot s carries the value at
 * index slot_src[s] of the block - for a borrowed slot the OWNER's wire - or 0 for HK_R1CS_SRC_ZERO, at address
 * 1 + g * sets_per_tx + slot_rank[s]: addresses are handed out from 1 in the order of the `set`s.
 * hk_r1cs_job_trace writes `get_portal_subtraces`: the flattened time-ordered trace, n_txs * slot_offsets[n_parts] entries of
 * (addr, val) in subcircuit order - what hk_trace_sort(2, ...), hk_exec_tree and hk_stage0_witness take, with
 * offsets[i + 1] - offsets[i] = the slots of partition i % P.
 * hk_r1cs_job_witness writes, into row b of z_out for subcircuit i = sub_index[b] (any order, repeats allowed, all of ONE
 * partition p): column 0 <- 1 and columns body_col0 .. body_col0 + body_len[p] - 1 <- wires 1 .. body_len[p] of that
 * subcircuit's witness (body_len = own wires + owned wires; a borrowed wire is the `val` column of its trace entry and has no
 * column here).  Every other column keeps its bytes: hk_stage1_witness on the same rows completes the assignment.
 * Both calls run on the caller's lane; a host-resident witness is staged in lane scratch, a device-resident one is read in
 * place.  batch == 0 or a job without slots: HK_OK, nothing done.  HK_ERR_ARG, before any device work and with the output
 * untouched: a NULL pointer; n_parts, n_txs or tx_len 0, or n_parts x n_txs > 2^24; slot_offsets[0] != 0 or decreasing; a
 * slot_rank >= sets_per_tx; a slot_src that is neither HK_R1CS_SRC_ZERO nor < tx_len; 1 + n_txs x sets_per_tx >= 2^32;
 * 2^31 entries or more; 0 < tx_stride < tx_len; an output range that overlaps the witness.  hk_r1cs_job_witness also:
 * wit_offsets[0] != 0, not increasing or not ending at tx_len; body_len[p] not below partition p's wires; sub_index[b] >=
 * n_parts x n_txs; selected subcircuits of different partitions; the body range not inside [1, n_v); z_out not in device
 * memory; batch >= 2^20, n_v >= 2^31 or batch x n_v >= 2^38. */
#define HK_R1CS_SRC_ZERO 0xFFFFFFFFu
typedef struct {
    uint32_t n_parts;               /* P >= 1 */
    uint32_t n_txs;                 /* T >= 1 */
    const uint32_t* slot_offsets;   /* [h] P + 1: partition p owns slots [slot_offsets[p], slot_offsets[p + 1]) of a transaction */
    const uint32_t* slot_rank;      /* [h] slot_offsets[P]: the slot's wire is the rank-th `set` of its transaction */
    const uint32_t* slot_src;       /* [h] slot_offsets[P]: index of its value in the witness block, or HK_R1CS_SRC_ZERO */
    uint32_t sets_per_tx;           /* O: `set`s of one transaction */
    uint32_t tx_len;                /* Fr of one witness block */
    uint32_t tx_stride;             /* Fr from one transaction's block to the next; 0: every transaction reads block 0 */
    const uint32_t* wit_offsets;    /* [h] P + 1: partition p's witness is [wit_offsets[p], wit_offsets[p + 1]) of a block */
    const uint32_t* body_len;       /* [h] P: own + owned wires of partition p, wire 0 not counted */
    const void* witness_mont;       /* [h|d] (n_txs - 1) x tx_stride + tx_len Fr */
} hk_r1cs_job_desc;                 /* wit_offsets / body_len: read by hk_r1cs_job_witness only */
hk_status hk_r1cs_job_trace(hk_ctx* ctx, const hk_r1cs_job_desc* desc,
                            void* time_entries_mont_out /* [h|d] n_txs * slot_offsets[n_parts] x 2 Fr */);
hk_status hk_r1cs_job_witness(hk_ctx* ctx, const hk_r1cs_job_desc* desc, const uint32_t* sub_index /* [h] batch */,
                              size_t batch, size_t n_v, size_t body_col0, void* z_out /* [d] batch x n_v Fr */);

/* ---- the verifiable key directory job (distributed-prover/src/vkd/vkd.rs:362-617 `vkd_update_to_subcircuit`,
 * vkd_constraints.rs:70-193 `get_portal_subtraces`, :237-342 `generate_constraints`; vkd/hash.rs) --------------------------------
 * A batch of U directory updates over a sparse Merkle tree of `depth` levels (hekaton_system_amd/vkd_circuit.py `VkdJob`): a
 * leaf is 66 bytes, hashed at rate 3 over its 27-byte chunks; a node is the low 216 bits of a digest; an update is two paths of
 * `depth` two-to-one hashes cut into `split` segments of L = depth / split levels, level l from the leaf using bit l of the
 * user's index (bit 1: the current node is the right child).  N = 8 + 2 split U subcircuits: 6 paddings, write-pp, 2 split per
 * update, the final equality.  The descriptor states the job once; every traced value lives once in the VALUE TABLE of
 * V = 3 + U (2 + 3 split) Fr:
 *     0 initial root   1 final root   2 null leaf (the leaf hash of 32 zero bytes)
 *     base(u) = 3 + u (2 + 3 split):  + 0 hash of leaf_old (0 for an append)  + 1 hash of leaf_new  + 2 + s index word s
 *                                     + 2 + split + p split + s the node after segment s of path p (p = 0 old, 1 new)
 * and time-ordered slot e of the whole job is (slot_addr[e], value[slot_src[e]]), or 0 for HK_VKD_SRC_ZERO (the paddings'
 * dummies): the host resolves names to addresses and sources, as `SetupRomPortalManager` does.
 * hk_vkd_trace computes the value table (roots copied from roots_mont; every hash on the device: one quad of lanes per leaf /
 * username hash, one quad per (update, path) for the chain of `depth` dependent hashes - path 0 of an append starts from the
 * null leaf) and the flattened trace: n_slots (addr, val) pairs, what hk_trace_sort(2, ...), hk_exec_tree and hk_stage0_witness
 * take.  values_mont is not read.
 * hk_vkd_witness writes, into row b of z_out for subcircuit i = sub_index[b] (any order, repeats allowed, all of the ONE class
 * cols->kind), column 0 <- 1 and the BODY columns of VkdSubcircuit: at hash_col0 the "hash leaf" part (528 leaf bit columns, the permutation's
 * trace in hk_poseidon_path's order, the digest's bits, the canon columns), at index_col0 the "get index" part (trace, bits,
 * canon), at path_col0 the "compute path" part (L index bits; per level sibling, left, trace, bits, canon and - but for the
 * last level - the next node).  A segment starts from the value its `get` slot names in values_mont.  Every other column
 * keeps its bytes: hk_stage1_witness on the same rows completes the assignment.  A class without body columns (padding, write
 * pp, equality) gets its column 0 only.
 * Both calls run on the caller's lane; host-resident arrays are staged in lane scratch, device-resident ones read in place.
 * One lane per Fr of the trace and four lanes per hash chain: 2 n_slots and 4 batch lanes stay below 2^31.
 * HK_ERR_ARG / HK_ERR_LEN, before any device work and with the outputs untouched: a NULL pointer; split < 2, depth 0, above
 * 256, no multiple of 8 split, or L < 8; n_updates 0 or above 2^20; a kind that is neither HK_VKD_APPEND nor HK_VKD_UPDATE;
 * N above 2^24; n_slots 0 or >= 2^30 (LEN); a slot_src that is neither HK_VKD_SRC_ZERO nor < V; Poseidon descriptors other
 * than the two instances hk_exec_tree takes; an output range that overlaps an input or the other output.  hk_vkd_witness
 * also: values_mont NULL; cols->kind no class; batch >= 2^20, n_v 0 or >= 2^31 or batch x n_v >= 2^38 (LEN); a part of the class
 * that does not fit [1, n_v) or overlaps the part before it (LEN); n_slots other than the layout's; sub_index[b] >= N or of
 * another class than cols->kind; z_out not in device memory. */
#define HK_VKD_SRC_ZERO 0xFFFFFFFFu
#define HK_VKD_APPEND 0u
#define HK_VKD_UPDATE 1u
typedef struct {
    uint32_t depth;                 /* levels of the sparse tree */
    uint32_t split;                 /* segments of a path */
    uint32_t n_updates;             /* U */
    const uint32_t* kinds;          /* [h] U: HK_VKD_APPEND / HK_VKD_UPDATE */
    const uint8_t* leaves;          /* [h|d] U x 2 x 66 bytes: leaf_old (zeros for an append), leaf_new */
    const void* siblings_mont;      /* [h|d] U x depth Fr: the update's siblings, the leaf's first */
    const void* consts_mont; size_t n_consts;                               /* [h|d] as hk_poseidon_path / hk_exec_tree */
    const hk_poseidon_desc* leaf_hash; const hk_poseidon_desc* node_hash;
    const void* roots_mont;         /* [h] 2 Fr: initial root, final root */
    uint32_t n_slots;               /* time-ordered entries of the whole job */
    const uint32_t* slot_addr;      /* [h] n_slots */
    const uint32_t* slot_src;       /* [h] n_slots: index into the value table, or HK_VKD_SRC_ZERO */
    const void* values_mont;        /* [h|d] V Fr: hk_vkd_trace's values_mont_out; read by hk_vkd_witness only */
} hk_vkd_desc;
typedef struct {
    uint32_t kind;                  /* 0 padding, 1 write pp, 2 hash leaf + get index + compute path, 3 compute path,
                                       4 compute path + equality, 5 equality + hash leaf + compute path, 6 equality */
    uint32_t hash_col0;             /* first column of the "hash leaf" part (kinds 2, 5) */
    uint32_t index_col0;            /* first column of the "get index" part (kind 2) */
    uint32_t path_col0;             /* first column of the "compute path" part (kinds 2 .. 5) */
} hk_vkd_cols;
hk_status hk_vkd_trace(hk_ctx* ctx, const hk_vkd_desc* desc, void* values_mont_out /* [h|d] V Fr */,
                       void* time_entries_mont_out /* [h|d] n_slots x 2 Fr */);
hk_status hk_vkd_witness(hk_ctx* ctx, const hk_vkd_desc* desc, const uint32_t* sub_index /* [h] batch */, size_t batch,
                         size_t n_v, const hk_vkd_cols* cols, void* z_out /* [d] batch x n_v Fr */);

/* ---- a VKD batch applied to the directory (vkd/sparse_tree.rs:70-177 `SparseMerkleTree`) ------------
 * What hk_vkd_desc.siblings_mont and roots_mont want, from the leaves themselves: the directory holds leaves0 (one 66-byte
 * leaf per user, at the index the low `depth` bits of its username's digest give), and update u of the batch inserts
 * leaves[u][1] - its leaf_new - at its own index.  The outputs are byte for byte those of the host loop
 *     t = SparseTree(depth); for each initial leaf: t.insert(index, leaf); roots[0] = t.root
 *     for each update u: siblings[u] = t.lookup_path(index_u); t.insert(index_u, leaf_new_u)
 *     roots[1] = t.root
 * (hekaton_system_amd/vkd_circuit.py `directory_paths`).  An insert overwrites, as in the reference.  status_out only
 * reports what the batch meets - the siblings are written whatever the status is: an append onto an index that holds a
 * leaf, an update of an index that holds none, an update whose leaf_old differs from the 66 bytes its index holds.
 * Every hash runs on the device, one quad of lanes per event (initial leaf or update) and level: `depth` dependent launches,
 * each data-parallel over the M + U events; up to 64 events, one launch of one workgroup.  The call runs on the caller's
 * lane; host-resident buffers are staged in lane scratch, device-resident ones read and written in place.
 * HK_ERR_ARG / HK_ERR_LEN, before any device work and with the outputs untouched: a NULL pointer (leaves0 only when
 * n_leaves0 > 0; status_out may be NULL); a depth that is no multiple of 8 in 16 .. 256; n_updates 0 or above 2^20;
 * n_leaves0 + n_updates above 2^22 (LEN); a kind that is neither HK_VKD_APPEND nor HK_VKD_UPDATE; Poseidon descriptors other
 * than the two instances hk_exec_tree takes; an output range that overlaps an input or another output. */
#define HK_VKD_ST_OK       0u
#define HK_VKD_ST_OCCUPIED 1u   /* an append whose index already holds a leaf */
#define HK_VKD_ST_ABSENT   2u   /* an update whose index holds no leaf */
#define HK_VKD_ST_STALE    3u   /* an update whose leaf_old is not the 66 bytes that index holds */
typedef struct {
    uint32_t depth;             /* a multiple of 8, 16 .. 256 */
    uint32_t n_leaves0;         /* M: the directory before the batch; may be 0 */
    const uint8_t* leaves0;     /* [h|d] M x 66 bytes, one leaf per user; a later one replaces an earlier one of the same index */
    uint32_t n_updates;         /* U >= 1 */
    const uint32_t* kinds;      /* [h] U: HK_VKD_APPEND / HK_VKD_UPDATE */
    const uint8_t* leaves;      /* [h|d] U x 2 x 66: exactly hk_vkd_desc.leaves (leaf_old is not read for an append) */
    const void* consts_mont; size_t n_consts;
    const hk_poseidon_desc* leaf_hash; const hk_poseidon_desc* node_hash;   /* as hk_vkd_trace */
} hk_vkd_tree_desc;
hk_status hk_vkd_tree(hk_ctx* ctx, const hk_vkd_tree_desc* desc,
                      void* siblings_mont_out /* [h|d] U x depth Fr, the leaf's sibling first: hk_vkd_desc.siblings_mont */,
                      void* roots_mont_out    /* [h|d] 2 Fr: root before the batch, root after it */,
                      uint8_t* status_out     /* [h|d] U bytes, HK_VKD_ST_*; may be NULL */);

/* ---- the aggregator's scalar vectors ------------------------------------------------------------
 * What `TIPA::setup`, `agg_subcircuit_proofs` and `TIPA::prove` build one field product at a time on the host: the powers of
 * a trapdoor or of the twist, and the two KZG witness polynomials of the folded keys.  Both results may stay on the device,
 * where hk_fixed_base_*, hk_scalar_pairing_* and hk_msm_bases read them.
 *
 * out[j * n + i] = x^i (Fr, Montgomery), i < n, j < reps - `structured_scalar_power` (pairing_ops.rs:42-48); reps > 1
 * repeats the vector back to back (agg_front sweeps five G1 vectors with the same powers).
 * x_mont [h]: one Fr; out [h|d]: reps * n Fr.  n == 0 or reps == 0: HK_OK, nothing written.
 * HK_ERR_ARG (nothing written): a null pointer, n > 2^27, reps > 65535, reps * n > 2^27. */
hk_status hk_scalar_powers(hk_ctx* ctx, const void* x_mont, size_t n, size_t reps, void* out);

/* Quotient of f(X) = X^shift * prod_{k < l} (1 + c_k (rho X)^(2^k)) by (X - z), remainder dropped, padded with one zero to
 * f's own length shift + 2^l - the witness polynomial of kzg.rs:122-141 for f_v (rho = 1, shift = 0, inverse challenges
 * reversed) and f_w (rho = 1 / twist, shift = n).  challenges_mont [h]: l Fr; rho_mont, z_mont [h]: one Fr each;
 * q_out [h|d]: shift + 2^l Fr, Montgomery: what hk_msm_bases takes with mont = 1.
 * HK_ERR_ARG (nothing written): a null pointer, l > 26, shift + 2^l > 2^27. */
hk_status hk_ipa_quotient(hk_ctx* ctx, const void* challenges_mont, size_t l, const void* rho_mont, const void* z_mont,
                          size_t shift, void* q_out);

/* ---- the aggregate verifier's class sums ---------------------------------------------------------
 * The keys of a job differ by class (aggregation.rs:76), so the verifier forms prod_i e(alpha_i, beta_i)^(x^i) as
 * prod_c e(alpha_c, beta_c)^(sums[c]): its one computation that grows with the number of proofs.
 *
 * sums_out[c] = sum of x^i over the i < n with class_of[i] == c (Fr, Montgomery); a class without members gives 0.
 * x_mont [h]: one Fr; class_of [h|d]: n uint32; sums_out [h|d]: n_classes Fr.  n == 0: n_classes zeros.
 * HK_ERR_ARG, nothing written: a null pointer, n > 2^27, n_classes == 0 or > 1024, some class_of[i] >= n_classes. */
hk_status hk_class_power_sums(hk_ctx* ctx, const void* x_mont, const uint32_t* class_of, size_t n, size_t n_classes,
                              void* sums_out);

#ifdef __cplusplus
}
#endif
#endif /* HEKATON_H */
