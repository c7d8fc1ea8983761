// sha256_shim.cpp — csrc/sha256.cuh compiled for the host (tests/test_sha_tree_cpu.py compares it with hashlib): the three
// message shapes, the iteration, the digest's field value on both curves and the round constants.
#include "../../hekaton_system_amd/csrc/sha256.cuh"

using namespace hk;

static void words_in(const unsigned char* p, u32* w, int n) {
    for (int i = 0; i < n; i++) w[i] = ((u32)p[4 * i] << 24) | ((u32)p[4 * i + 1] << 16) | ((u32)p[4 * i + 2] << 8) | p[4 * i + 3];
}
static void digest_out(const u32 (&d)[8], unsigned char* out) {
    for (int j = 0; j < 32; j++) out[j] = (unsigned char)((d[j / 4] >> (24 - 8 * (j % 4))) & 0xff);
}

extern "C" {

void shim_sha_consts(u32* k64, u32* iv8) {
    for (int i = 0; i < 64; i++) k64[i] = Sha256Consts::K[i];
    for (int i = 0; i < 8; i++) iv8[i] = Sha256Consts::IV[i];
}

// out <- SHA-256 applied ns times to the 64-byte msg
void shim_sha_iter64(const unsigned char* msg, u32 ns, unsigned char* out) {
    u32 b[16], d[8];
    words_in(msg, b, 16);
    iterated_sha256(d, b, true, ns);
    digest_out(d, out);
}

// out <- SHA-256 applied ns times to bytes 0 .. 26 of l followed by bytes 0 .. 26 of r (l, r: 32-byte digests)
void shim_sha_iter54(const unsigned char* l, const unsigned char* r, u32 ns, unsigned char* out) {
    u32 lw[8], rw[8], b[16], d[8];
    words_in(l, lw, 8);
    words_in(r, rw, 8);
    sha_block_children(b, lw, rw);
    iterated_sha256(d, b, false, ns);
    digest_out(d, out);
}

// out <- SHA-256 applied ns times to the 32-byte digest dg
void shim_sha_iter32(const unsigned char* dg, u32 ns, unsigned char* out) {
    u32 w[8], b[16], d[8];
    words_in(dg, w, 8);
    sha_block_digest(b, w);
    iterated_sha256(d, b, false, ns);
    digest_out(d, out);
}

// one compression of the 64-byte block into state (8 words in, 8 words out)
void shim_sha_compress(u32* state, const unsigned char* block) {
    u32 s[8], b[16];
    for (int i = 0; i < 8; i++) s[i] = state[i];
    words_in(block, b, 16);
    sha256_compress(s, b);
    for (int i = 0; i < 8; i++) state[i] = s[i];
}

// out <- Montgomery limbs of node_hash_field(dg); curve 0 = BN254, 1 = BLS12-381
void shim_sha_digest_field(int curve, const unsigned char* dg, u32* out) {
    u32 w[8];
    words_in(dg, w, 8);
    if (curve == 0) {
        Fp<Bn254FrP> x = sha_digest_field<Fp<Bn254FrP>>(w);
        for (int i = 0; i < 8; i++) out[i] = x.v[i];
    } else {
        Fp<Bls381FrP> x = sha_digest_field<Fp<Bls381FrP>>(w);
        for (int i = 0; i < 8; i++) out[i] = x.v[i];
    }
}

}  // extern "C"
