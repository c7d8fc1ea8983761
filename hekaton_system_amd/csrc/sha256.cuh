// sha256.cuh — SHA-256 over the three message shapes a big-merkle job has (hk_sha_tree): a 64-byte
// leaf, a 32-byte digest, and the 54 bytes of two truncated child digests (tree_hash_circuit.rs `INNER_HASH_SIZE` = 27).
// Words are big-endian as FIPS 180-4 has them: digest byte j = (H[j / 4] >> (24 - 8 (j % 4))) & 0xff.  One lane hashes one
// message; the 64 rounds are unrolled over a 16-word rolling schedule, so state, schedule and constants are registers and
// immediates and no kernel that uses this owns private memory.  Also compiles as plain host C++ (tests build it with g++
// and compare with hashlib; the library never runs it on the CPU).
#pragma once
#include "ec.cuh"            // field.cuh's HK_HD / HK_UNROLL, HK_NOUNROLL

namespace hk {

constexpr u32 SHA_INNER_HASH_SIZE = 27;        // bytes of a child digest a parent hashes, and of a node's field value

struct Sha256Consts {
    // floor(frac(cbrt(p)) 2^32) of the first 64 primes, floor(frac(sqrt(p)) 2^32) of the first 8
    static constexpr u32 K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
        0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
        0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
        0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    static constexpr u32 IV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                                  0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
};

HK_HD u32 sha_rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }

HK_HD void sha256_init(u32 (&state)[8]) {
    HK_UNROLL for (int i = 0; i < 8; i++) state[i] = Sha256Consts::IV[i];
}

// state <- compress(state, block).  Round i keeps a .. h at s[(j - i) & 7]: nothing moves, and after 64 rounds a is s[0] again.
HK_HD void sha256_compress(u32 (&state)[8], const u32 (&block)[16]) {
    u32 w[16], s[8];
    HK_UNROLL for (int i = 0; i < 16; i++) w[i] = block[i];
    HK_UNROLL for (int i = 0; i < 8; i++) s[i] = state[i];
    HK_UNROLL for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const u32 w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
            w[i & 15] += (sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3)) + w[(i - 7) & 15] +
                         (sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10));
        }
        const u32 a = s[(0 - i) & 7], b = s[(1 - i) & 7], c = s[(2 - i) & 7];
        const u32 e = s[(4 - i) & 7], f = s[(5 - i) & 7], g = s[(6 - i) & 7];
        const u32 t1 = s[(7 - i) & 7] + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + ((e & f) ^ (~e & g)) +
                       Sha256Consts::K[i] + w[i & 15];
        const u32 t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        s[(3 - i) & 7] += t1;
        s[(7 - i) & 7] = t1 + t2;
    }
    HK_UNROLL for (int i = 0; i < 8; i++) state[i] += s[i];
}

// ---- the three message shapes ------------------------------------------------------------------------------------------
// the SECOND block of a 64-byte message (the first is its 16 words): 80 00 .. 00, length 512
HK_HD void sha_block_pad64(u32 (&b)[16]) {
    HK_UNROLL for (int i = 0; i < 16; i++) b[i] = 0;
    b[0] = 0x80000000u;
    b[15] = 512;
}
// the one block of a 32-byte digest: digest, 80, zeros, length 256
HK_HD void sha_block_digest(u32 (&b)[16], const u32 (&d)[8]) {
    HK_UNROLL for (int i = 0; i < 8; i++) b[i] = d[i];
    HK_UNROLL for (int i = 8; i < 16; i++) b[i] = 0;
    b[8] = 0x80000000u;
    b[15] = 256;
}
// the one block of two truncated child digests: bytes 0 .. 26 of l, bytes 0 .. 26 of r, 80, 00, length 432
HK_HD void sha_block_children(u32 (&b)[16], const u32 (&l)[8], const u32 (&r)[8]) {
    HK_UNROLL for (int i = 0; i < 6; i++) b[i] = l[i];
    b[6] = (l[6] & 0xffffff00u) | (r[0] >> 24);
    HK_UNROLL for (int i = 0; i < 6; i++) b[7 + i] = (r[i] << 8) | (r[i + 1] >> 24);
    b[13] = ((r[6] << 8) & 0xffff0000u) | 0x8000u;
    b[14] = 0;
    b[15] = 8 * 2 * SHA_INNER_HASH_SIZE;
}

// digest <- SHA-256 applied ns >= 1 times to the message whose first block is b: a 64-byte message when two_blocks (b = its
// 16 words; the padding block follows), else a message of one block (sha_block_children / sha_block_digest).  Every
// application after the first hashes the 32-byte digest before it.  One copy of the rounds: a loop of ns (+ 1) compressions,
// the next block and state chosen by selects; b is used up.
HK_HD void iterated_sha256(u32 (&digest)[8], u32 (&b)[16], bool two_blocks, u32 ns) {
    u32 h[8];
    sha256_init(h);
    const u32 steps = ns + (two_blocks ? 1u : 0u);
    HK_NOUNROLL for (u32 t = 0; t < steps; t++) {
        sha256_compress(h, b);
        const bool mid = two_blocks && t == 0;             // between the two blocks of the 64-byte message: the state goes on
        u32 pad[16], nxt[16];
        sha_block_pad64(pad);
        sha_block_digest(nxt, h);
        HK_UNROLL for (int i = 0; i < 16; i++) b[i] = mid ? pad[i] : nxt[i];
        HK_UNROLL for (int i = 0; i < 8; i++) {
            digest[i] = h[i];
            h[i] = mid ? h[i] : Sha256Consts::IV[i];
        }
    }
}

// `node_hash_field` in Montgomery form: bytes 0 .. 26 of the digest as a little-endian integer (216 bits, below r)
template <class Fr>
HK_HD Fr sha_digest_field(const u32 (&d)[8]) {
    static_assert(Fr::N == 8, "a 216-bit value in eight 32-bit limbs");
    Fr x;
    HK_UNROLL for (int i = 0; i < 6; i++) x.v[i] = __builtin_bswap32(d[i]);
    x.v[6] = __builtin_bswap32(d[6]) & 0x00ffffffu;
    x.v[7] = 0;
    return Fr::to_mont(x);
}

}  // namespace hk
