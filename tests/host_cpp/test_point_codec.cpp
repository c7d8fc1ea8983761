// The C++ host codecs (host/ark_serialize.hpp) against the Python codec, compressed: argv[1] = bn254 | bls12_381, argv[2] = a
// directory with what Python wrote -
//   g1_abi / g2_abi             packed Montgomery points (infinity among them)
//   g1_wire / g2_wire           ... as ArkCodec(curve).points_to_wire(compress=True) encodes them
//   proof_a, proof_b, proof_c, proof_d0, proof_d1; proof_wire   a proof's points and its compressed record
//   bad_wire                    one compressed G1 x that is on no curve point
// The program checks both directions of each and writes back cpp_g1_wire, cpp_g2_wire and cpp_proof_wire for Python to read.
#include <cstdio>
#include <fstream>
#include <iterator>
#include "../../hekaton_system_amd/csrc/host/ark_serialize.hpp"
using namespace hekaton;

static Bytes rd(const std::string& dir, const std::string& name) {
    std::ifstream f(dir + "/" + name, std::ios::binary);
    if (!f) throw std::runtime_error("missing " + name);
    return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void wr(const std::string& dir, const std::string& name, const Bytes& b) {
    std::ofstream f(dir + "/" + name, std::ios::binary);
    f.write((const char*)b.data(), (std::streamsize)b.size());
}
static void expect(bool ok, const char* what) {
    if (!ok) throw std::runtime_error(std::string("mismatch: ") + what);
}

template <class Codec>
static void run(const Codec& cd, const std::string& dir, size_t fq) {
    for (int group = 1; group <= 2; group++) {
        const std::string g = group == 1 ? "g1" : "g2";
        const Bytes abi = rd(dir, g + "_abi"), wire = rd(dir, g + "_wire");
        const size_t n = abi.size() / (2 * fq * group);
        expect(wire.size() == n * fq * group, "compressed size");
        const Bytes mine = cd.points_to_wire(group, abi, true);
        expect(mine == wire, "points_to_wire(compress) against Python's bytes");
        expect(cd.points_from_wire(group, wire.data(), n, true) == abi, "points_from_wire(compress) of Python's bytes");
        expect(cd.points_from_wire(group, wire.data(), n, true, true) == abi, "... validated");
        expect(cd.points_from_wire(group, cd.points_to_wire(group, abi).data(), n, false) == abi, "uncompressed round trip");
        wr(dir, "cpp_" + g + "_wire", mine);
    }
    Proof p;
    p.a = rd(dir, "proof_a"); p.b = rd(dir, "proof_b"); p.c = rd(dir, "proof_c");
    p.ds = {rd(dir, "proof_d0"), rd(dir, "proof_d1")};
    const Bytes pw = rd(dir, "proof_wire");
    const Bytes mine = cd.proof_to_wire(p, true);
    expect(mine == pw, "proof_to_wire(compress)");
    expect(pw.size() == 4 * fq + 8 + 2 * fq, "compressed proof size");
    const Proof back = cd.proof_from_wire(pw, true, true);
    expect(back.a == p.a && back.b == p.b && back.c == p.c && back.ds == p.ds, "proof_from_wire(compress)");
    const Proof full = cd.proof_from_wire(cd.proof_to_wire(p));
    expect(full.a == p.a && full.b == p.b && full.c == p.c && full.ds == p.ds, "proof round trip, uncompressed");
    wr(dir, "cpp_proof_wire", mine);
    const Bytes bad = rd(dir, "bad_wire");
    bool threw = false;
    try { cd.points_from_wire(1, bad.data(), 1, true); } catch (const SerializationError&) { threw = true; }
    expect(threw, "an x with no root raises");
    threw = false;
    try { cd.proof_from_wire(Bytes(pw.begin(), pw.end() - 1), true); } catch (const SerializationError&) { threw = true; }
    expect(threw, "a short record raises");
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s bn254|bls12_381 <dir>\n", argv[0]); return 2; }
    try {
        const std::string curve = argv[1], dir = argv[2];
        if (curve == "bn254") {
            Context ctx(HK_BN254, 0);
            run(ArkCodecBn254(ctx), dir, 32);
        } else {
            Context ctx(HK_BLS12_381, 0);
            run(ArkCodecBls381(ctx), dir, 48);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "FAILED: %s\n", e.what());
        return 1;
    }
    printf("POINT_CODEC_CPP_OK\n");
    return 0;
}
