// Host-compiled view of the PRODUCT's agg_scalars.cuh (g++): the HK_HD chunk bodies of hk_scalar_powers / hk_ipa_quotient
// run chunk by chunk over the host's own tables, with serial loops where the device scans in LDS - the same tiles, the same
// tile carries, the same multipliers.  Test-only; never part of libhekaton.
//
// Built twice by tests/test_agg_scalars_cpu.py: as a shared object (the extern "C" entries, compared with the Python mirror)
// and, with -DAGG_SCALARS_MAIN, as a stand-alone program that prints one digest per case (run plain and under
// -fsanitize=address,undefined: same digests, clean exit).
#include "../../hekaton_system_amd/csrc/agg_scalars.cuh"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace hk;

template <class Fr>
static void powers(const void* x_mont, size_t n, size_t reps, void* out) {
    Fr x, tab[AQ_PW_LEN];
    memcpy(&x, x_mont, sizeof(Fr));
    aq_powers_table<Fr>(x, tab);
    const u32 n_chunks = (u32)((n + AQ_CHUNK - 1) / AQ_CHUNK);
    u32 nbits = 0;
    while (((u64)1 << nbits) < n_chunks) nbits++;
    for (size_t y = 0; y < reps; y++)
        for (u32 t = 0; t < n_chunks; t++) aq_power_chunk<Fr>(tab, t, nbits, n, (Fr*)out + y * n);
}

template <class Fr>
static AqShape shape_of(size_t l, size_t shift) {
    AqShape s;
    s.shift = shift;
    s.len = shift + ((u64)1 << l);
    s.l = (u32)l;
    s.n_chunks = (u32)((s.len + AQ_CHUNK - 1) / AQ_CHUNK);
    return s;
}

template <class Fr>
static void quotient(const void* challenges, size_t l, const void* rho_mont, const void* z_mont, size_t shift, void* q_out) {
    const AqShape s = shape_of<Fr>(l, shift);
    const u32 n_tiles = (s.n_chunks + AQ_TILE - 1) / AQ_TILE, per = (n_tiles + AQ_TOPS_LANES - 1) / AQ_TOPS_LANES;
    Fr ch[AQ_MAX_L], rho, z;
    memcpy(ch, challenges, l * sizeof(Fr));
    memcpy(&rho, rho_mont, sizeof(Fr));
    memcpy(&z, z_mont, sizeof(Fr));
    std::vector<Fr> tab(AQ_LEN);
    aq_quotient_table<Fr>(ch, s.l, rho, z, per, tab.data());
    // (1) chunk values, (2a) the suffix sums within each tile and the tile totals
    std::vector<Fr> part((size_t)n_tiles * AQ_TILE, Fr::zero()), tops(n_tiles), lane((size_t)AQ_TOPS_LANES, Fr::zero());
    for (u32 t = 0; t < s.n_chunks; t++) part[t] = aq_chunk_horner<Fr>(tab.data(), s, t);
    for (u32 b = 0; b < n_tiles; b++) {
        for (u32 tid = AQ_TILE - 1; tid-- > 0;)
            part[b * AQ_TILE + tid] = Fr::add(part[b * AQ_TILE + tid], Fr::mul(tab[AQ_ZS], part[b * AQ_TILE + tid + 1]));
        tops[b] = part[(size_t)b * AQ_TILE];
    }
    // (2b) per lane of the tops scan its tiles' Horner value, the suffix over the lanes, the running value back down
    const Fr Q = tab[AQ_PZ + AQ_TILE];
    for (u32 k = 0; k < AQ_TOPS_LANES; k++)
        for (u32 j = per; j-- > 0;) {
            const u32 i = k * per + j;
            lane[k] = Fr::add(i < n_tiles ? tops[i] : Fr::zero(), Fr::mul(Q, lane[k]));
        }
    for (u32 k = AQ_TOPS_LANES - 1; k-- > 0;) lane[k] = Fr::add(lane[k], Fr::mul(tab[AQ_QP], lane[k + 1]));
    for (u32 k = 0; k < AQ_TOPS_LANES; k++) {
        Fr run = k + 1 < AQ_TOPS_LANES ? lane[k + 1] : Fr::zero();
        for (u32 j = per; j-- > 0;) {
            const u32 i = k * per + j;
            if (i >= n_tiles) continue;
            const Fr x = tops[i];
            tops[i] = run;
            run = Fr::add(x, Fr::mul(Q, run));
        }
    }
    // (3)
    for (u32 t = 0; t < s.n_chunks; t++) {
        const u32 tid = t % AQ_TILE;
        Fr next = tid + 1 < AQ_TILE && t + 1 < s.n_chunks ? part[t + 1] : Fr::zero();
        next = Fr::add(next, Fr::mul(tab[AQ_PZ + AQ_TILE - 1 - tid], tops[t / AQ_TILE]));
        aq_chunk_walk<Fr>(tab.data(), s, t, next, (Fr*)q_out);
    }
}

template <class Fr>
static void coeff(const void* challenges, size_t l, const void* rho_mont, size_t shift, size_t i, void* out) {
    const AqShape s = shape_of<Fr>(l, shift);
    Fr ch[AQ_MAX_L], rho;
    memcpy(ch, challenges, l * sizeof(Fr));
    memcpy(&rho, rho_mont, sizeof(Fr));
    std::vector<Fr> tab(AQ_LEN);
    aq_quotient_table<Fr>(ch, s.l, rho, Fr::one(), 1, tab.data());
    const Fr c = aq_coeff_at<Fr>(tab.data(), s, i);
    memcpy(out, &c, sizeof(Fr));
}

extern "C" {
// curve: 0 bn254, 1 bls12-381; the arguments of hk_scalar_powers / hk_ipa_quotient, host buffers only
void shim_scalar_powers(int curve, const void* x_mont, size_t n, size_t reps, void* out) {
    if (curve == 0) powers<Fp<Bn254FrP>>(x_mont, n, reps, out); else powers<Fp<Bls381FrP>>(x_mont, n, reps, out);
}
void shim_ipa_quotient(int curve, const void* challenges, size_t l, const void* rho, const void* z, size_t shift, void* q_out) {
    if (curve == 0) quotient<Fp<Bn254FrP>>(challenges, l, rho, z, shift, q_out);
    else quotient<Fp<Bls381FrP>>(challenges, l, rho, z, shift, q_out);
}
// coefficient i of f (Montgomery), 0 outside [shift, shift + 2^l)
void shim_ipa_coeff(int curve, const void* challenges, size_t l, const void* rho, size_t shift, size_t i, void* out) {
    if (curve == 0) coeff<Fp<Bn254FrP>>(challenges, l, rho, shift, i, out); else coeff<Fp<Bls381FrP>>(challenges, l, rho, shift, i, out);
}
}

#ifdef AGG_SCALARS_MAIN
static u64 fnv(const void* p, size_t n, u64 h = 1469598103934665603ull) {
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}
// field elements from a seed: Montgomery products and sums of what came before stay in [0, p)
template <class Fr>
static Fr next_value(Fr& state) {
    state = Fr::add(Fr::mul(state, state), Fr::r2());
    return state;
}
template <class Fr>
static void run_cases(const char* name) {
    Fr st = Fr::r2();
    const size_t pn[] = {1, 7, 8, 9, 513, 2049};
    for (size_t n : pn) {
        const Fr x = next_value(st);
        const size_t reps = n == 9 ? 5 : 1;
        std::vector<Fr> out(reps * n);
        powers<Fr>(&x, n, reps, out.data());
        printf("%s powers n=%zu reps=%zu %016llx\n", name, n, reps, (unsigned long long)fnv(out.data(), out.size() * sizeof(Fr)));
    }
    const size_t qc[][2] = {{0, 0}, {0, 1}, {3, 0}, {3, 8}, {4, 5}, {11, 0}, {11, 5}, {12, 4096}, {17, 131072}};
    for (auto& c : qc) {
        const size_t l = c[0], shift = c[1];
        Fr ch[AQ_MAX_L];
        for (size_t k = 0; k < l; k++) ch[k] = next_value(st);
        const Fr rho = next_value(st), z = next_value(st);
        std::vector<Fr> q(shift + ((size_t)1 << l));
        quotient<Fr>(ch, l, &rho, &z, shift, q.data());
        printf("%s quotient l=%zu shift=%zu %016llx\n", name, l, shift, (unsigned long long)fnv(q.data(), q.size() * sizeof(Fr)));
    }
}
int main() {
    run_cases<Fp<Bn254FrP>>("bn254");
    run_cases<Fp<Bls381FrP>>("bls12_381");
    return 0;
}
#endif
