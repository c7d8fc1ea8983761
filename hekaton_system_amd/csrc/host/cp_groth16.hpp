// cp_groth16.hpp — C++ host-side mirror of the reference's cp-groth16 / worker surface over the C ABI.
//
// The reference is Rust; no Rust toolchain exists in the build image, so the host side above the
// C ABI is written in C++ with the reference's names, argument meaning and error behaviour:
//   ProvingKey / CommitterKey / Proof            cp-groth16/src/data_structures.rs:7-16,66-114
//   MultiStageConstraintSystem                   cp-groth16/src/constraint_synthesizer.rs:14-117
//   MultiStageConstraintSynthesizer              cp-groth16/src/constraint_synthesizer.rs:119-134
//   CommitmentBuilder::{new,commit,prove}        cp-groth16/src/committer.rs:38-123
//   CPGroth16::prove_last_stage                  cp-groth16/src/prover.rs:53-156
//   Stage{0,1}Response, process_stage{0,1}_*     distributed-prover/src/worker.rs:20-195
// Header-only; all arithmetic is in libhekaton (HIP).  Field elements are opaque Montgomery byte
// strings on this side (the Rust side holds ark `Fp` values with the same bytes).
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/hekaton.h"

namespace hekaton {

struct Error : std::runtime_error {
    hk_status status;
    Error(hk_status s, const std::string& what) : std::runtime_error(what + ": " + hk_status_str(s)), status(s) {}
};
inline void check(hk_status s, const char* what) { if (s != HK_OK) throw Error(s, what); }

typedef std::vector<uint8_t> Bytes;

struct Sizes { size_t fr, fq, g1, g2; };

class Context {
public:
    Context(hk_curve curve, int device) : curve_(curve) {
        check(hk_ctx_create(curve, device, &ctx_), "hk_ctx_create");
        check(hk_ctx_sizes(ctx_, &sz_.fr, &sz_.fq, &sz_.g1, &sz_.g2), "hk_ctx_sizes");
    }
    ~Context() { hk_ctx_destroy(ctx_); }
    Context(const Context&) = delete;
    hk_ctx* raw() const { return ctx_; }
    const Sizes& sizes() const { return sz_; }
private:
    hk_curve curve_;
    hk_ctx* ctx_ = nullptr;
    Sizes sz_;
};

struct Csr { std::vector<uint64_t> row_ptr; std::vector<uint32_t> col; Bytes val_mont; };

// data_structures.rs:66-83 (+ the class's constraint matrices, uploaded with the key)
struct ProvingKey {
    Bytes alpha_g, beta_g, beta_h, last_delta_h;      // vk.alpha_g, beta_g, vk.beta_h, vk.deltas_h.last()
    Bytes a_g, b_g, b_h, h_g, deltas_g;
    std::vector<Bytes> ck_deltas_abc_g;               // ck.deltas_abc_g[stage]
    Csr A, B, C;
    size_t n_inst = 0, n_constraints = 0;
    hk_pk* device = nullptr;

    void upload(const Context& ctx) {
        if (device) return;
        const Sizes& z = ctx.sizes();
        std::vector<const void*> ckp;
        std::vector<size_t> ckl;
        for (auto& c : ck_deltas_abc_g) { ckp.push_back(c.data()); ckl.push_back(c.size() / z.g1); }
        hk_csr a{A.row_ptr.data(), A.col.data(), A.val_mont.data(), A.row_ptr.size() - 1, A.col.size()};
        hk_csr b{B.row_ptr.data(), B.col.data(), B.val_mont.data(), B.row_ptr.size() - 1, B.col.size()};
        hk_csr c{C.row_ptr.data(), C.col.data(), C.val_mont.data(), C.row_ptr.size() - 1, C.col.size()};
        hk_pk_desc d{};
        d.a_g = a_g.data(); d.a_len = a_g.size() / z.g1;
        d.b_g = b_g.data(); d.b_g_len = b_g.size() / z.g1;
        d.b_h = b_h.data(); d.b_h_len = b_h.size() / z.g2;
        d.h_g = h_g.data(); d.h_len = h_g.size() / z.g1;
        d.ck_stage = ckp.data(); d.ck_len = ckl.data(); d.n_stages = ckp.size();
        d.deltas_g = deltas_g.data(); d.last_delta_h = last_delta_h.data();
        d.alpha_g = alpha_g.data(); d.beta_g = beta_g.data(); d.beta_h = beta_h.data();
        d.A = &a; d.B = &b; d.C = &c; d.n_inst = n_inst; d.n_constraints = n_constraints;
        check(hk_pk_upload(ctx.raw(), &d, &device), "hk_pk_upload");
    }
    ~ProvingKey() { if (device) hk_pk_free(device); }
};

struct Proof { Bytes a, b, c; std::vector<Bytes> ds; };          // data_structures.rs:7-16

// generate_parameters past synthesis (generator.rs:66-224) in one device call (hk_keygen): the toxic waste (one Fr each,
// Montgomery bytes; deltas: one per stage, concatenated) and the class's matrices in, the key out - pk's matrices, sizes
// and every array it holds; the verifying-key parts it does not hold (gamma_h, gamma_abc_g, every stage's delta_h) go to
// the optional vk_* outputs.
struct SetupTrapdoor { Bytes alpha, beta, gamma, t, g1_scalar, g2_scalar, deltas; };
inline void generate_parameters(const Context& ctx, const Csr& A, const Csr& B, const Csr& C, size_t n_inst, size_t n_constraints,
                                size_t n_v, const std::vector<std::pair<uint64_t, uint64_t>>& stage_ranges,
                                const SetupTrapdoor& td, ProvingKey& pk, Bytes* vk_gamma_h = nullptr,
                                Bytes* vk_gamma_abc_g = nullptr, Bytes* vk_deltas_h = nullptr) {
    const Sizes& z = ctx.sizes();
    size_t m = 1;
    while (m < n_constraints + n_inst) m <<= 1;
    const size_t ns = stage_ranges.size();
    pk.A = A; pk.B = B; pk.C = C;
    pk.n_inst = n_inst; pk.n_constraints = n_constraints;
    pk.a_g.assign(n_v * z.g1, 0); pk.b_g.assign(n_v * z.g1, 0); pk.b_h.assign(n_v * z.g2, 0); pk.h_g.assign((m - 1) * z.g1, 0);
    pk.deltas_g.assign(ns * z.g1, 0); pk.alpha_g.assign(z.g1, 0); pk.beta_g.assign(z.g1, 0); pk.beta_h.assign(z.g2, 0);
    pk.ck_deltas_abc_g.assign(ns, Bytes());
    std::vector<void*> ckp(ns);
    std::vector<uint64_t> sr;
    for (size_t k = 0; k < ns; k++) {
        pk.ck_deltas_abc_g[k].assign((stage_ranges[k].second - stage_ranges[k].first) * z.g1, 0);
        ckp[k] = pk.ck_deltas_abc_g[k].data();
        sr.push_back(stage_ranges[k].first);
        sr.push_back(stage_ranges[k].second);
    }
    Bytes gamma_h(z.g2), gamma_abc_g(n_inst * z.g1), deltas_h(ns * z.g2);
    hk_csr a{A.row_ptr.data(), A.col.data(), A.val_mont.data(), A.row_ptr.size() - 1, A.col.size()};
    hk_csr b{B.row_ptr.data(), B.col.data(), B.val_mont.data(), B.row_ptr.size() - 1, B.col.size()};
    hk_csr c{C.row_ptr.data(), C.col.data(), C.val_mont.data(), C.row_ptr.size() - 1, C.col.size()};
    hk_keygen_desc d{&a, &b, &c, n_inst, n_constraints, n_v, sr.data(), ns, td.alpha.data(), td.beta.data(), td.gamma.data(),
                     td.t.data(), td.g1_scalar.data(), td.g2_scalar.data(), td.deltas.data()};
    hk_keygen_out o{pk.a_g.data(), pk.b_g.data(), pk.b_h.data(), pk.h_g.data(), ckp.data(), pk.deltas_g.data(), pk.alpha_g.data(),
                    pk.beta_g.data(), gamma_abc_g.data(), pk.beta_h.data(), gamma_h.data(), deltas_h.data(), nullptr};
    check(hk_keygen(ctx.raw(), &d, &o, nullptr), "hk_keygen");
    pk.last_delta_h.assign(deltas_h.end() - z.g2, deltas_h.end());
    if (vk_gamma_h) *vk_gamma_h = gamma_h;
    if (vk_gamma_abc_g) *vk_gamma_abc_g = gamma_abc_g;
    if (vk_deltas_h) *vk_deltas_h = deltas_h;
}

// ark `cs.which_is_unsatisfied()` for `batch` assignments of one class, where they lie (hk_pk_r1cs_check / hk_r1cs_check): z
// is host or device memory, batch x n_v Fr Montgomery.  Returns per assignment the first failing row, or -1 when it is
// satisfied (`cs.is_satisfied()`).  The first form uses the matrices an uploaded key carries, the second takes them directly.
inline std::vector<int64_t> which_is_unsatisfied(const Context& ctx, const ProvingKey& pk, const void* z, size_t n_v, size_t batch) {
    std::vector<hk_r1cs_verdict> v(batch);
    check(hk_pk_r1cs_check(ctx.raw(), pk.device, z, n_v, batch, v.data(), nullptr, nullptr, 0), "hk_pk_r1cs_check");
    std::vector<int64_t> out(batch);
    for (size_t b = 0; b < batch; b++) out[b] = v[b].n_bad ? (int64_t)v[b].first_bad : -1;
    return out;
}
inline std::vector<int64_t> which_is_unsatisfied(const Context& ctx, const Csr& A, const Csr& B, const Csr& C, const void* z, size_t n_v,
                                                 size_t batch) {
    hk_csr a{A.row_ptr.data(), A.col.data(), A.val_mont.data(), A.row_ptr.size() - 1, A.col.size()};
    hk_csr b{B.row_ptr.data(), B.col.data(), B.val_mont.data(), B.row_ptr.size() - 1, B.col.size()};
    hk_csr c{C.row_ptr.data(), C.col.data(), C.val_mont.data(), C.row_ptr.size() - 1, C.col.size()};
    std::vector<hk_r1cs_verdict> v(batch);
    check(hk_r1cs_check(ctx.raw(), &a, &b, &c, z, n_v, batch, v.data(), nullptr, nullptr, 0), "hk_r1cs_check");
    std::vector<int64_t> out(batch);
    for (size_t i = 0; i < batch; i++) out[i] = v[i].n_bad ? (int64_t)v[i].first_bad : -1;
    return out;
}


// constraint_synthesizer.rs:14-117 — assignments only (matrices are static per class and live with the key)
struct MultiStageConstraintSystem {
    size_t fr_bytes;
    Bytes instance_assignment, witness_assignment;      // Montgomery Fr, concatenated
    std::vector<std::pair<size_t, size_t>> variable_range_for_stage;
    explicit MultiStageConstraintSystem(size_t fr, const Bytes& one_mont) : fr_bytes(fr), instance_assignment(one_mont) {}
    void initialize_stage() { size_t s = num_witness_variables(); variable_range_for_stage.push_back({s, s}); }
    void finalize_stage() { variable_range_for_stage.back().second = num_witness_variables(); }
    void new_input_variable(const uint8_t* v) { instance_assignment.insert(instance_assignment.end(), v, v + fr_bytes); }
    void new_witness_variable(const uint8_t* v) { witness_assignment.insert(witness_assignment.end(), v, v + fr_bytes); }
    size_t num_instance_variables() const { return instance_assignment.size() / fr_bytes; }
    size_t num_witness_variables() const { return witness_assignment.size() / fr_bytes; }
    Bytes current_stage_witness_assignment() const {                    // :96-99
        auto r = variable_range_for_stage.back();
        return Bytes(witness_assignment.begin() + r.first * fr_bytes, witness_assignment.begin() + r.second * fr_bytes);
    }
    Bytes full_assignment() const {                                     // :102-106
        Bytes z = instance_assignment;
        z.insert(z.end(), witness_assignment.begin(), witness_assignment.end());
        return z;
    }
};

struct MultiStageConstraintSynthesizer {                               // constraint_synthesizer.rs:119-134
    virtual ~MultiStageConstraintSynthesizer() {}
    virtual size_t total_num_stages() const = 0;
    size_t last_stage() const { return total_num_stages() - 1; }
    virtual void generate_constraints(size_t stage, MultiStageConstraintSystem& cs) = 0;
};

// draws one Montgomery Fr (the reference's `E::ScalarField::rand(rng)`)
typedef std::function<Bytes()> FrRng;

struct CPGroth16 {                                                     // prover.rs:53-156
    static Proof prove_last_stage(const Context& ctx, MultiStageConstraintSystem& cs,
                                  MultiStageConstraintSynthesizer& circuit, ProvingKey& pk, const Bytes& r,
                                  const Bytes& s, const std::vector<Bytes>& comm_rands) {
        circuit.generate_constraints(circuit.last_stage(), cs);        // prover.rs:70
        Bytes z = cs.full_assignment();
        Bytes kap;
        for (auto& k : comm_rands) kap.insert(kap.end(), k.begin(), k.end());
        const Sizes& sz = ctx.sizes();
        Proof p;
        p.a.resize(sz.g1); p.b.resize(sz.g2); p.c.resize(sz.g1);
        check(hk_prove(ctx.raw(), pk.device, z.data(), z.size() / sz.fr, r.data(), s.data(),
                       kap.empty() ? nullptr : kap.data(), comm_rands.size(), p.a.data(), p.b.data(), p.c.data()),
              "hk_prove");
        return p;
    }
    // hk_prove_batch: `batch` proofs of one key class in one lock-step call (the stage-1 half of a worker's
    // compute_responses, node.rs:760-795).  z_rows: batch x n_v Fr row after row (host, or a device pointer); rs, ss:
    // batch Fr each; kappas: batch x n_kappas Fr.  Proof b equals prove_last_stage's on row b (ds left empty).
    static std::vector<Proof> prove_batch(const Context& ctx, ProvingKey& pk, const void* z_rows, size_t n_v, const Bytes& rs,
                                          const Bytes& ss, const Bytes& kappas, size_t n_kappas, size_t batch) {
        const Sizes& sz = ctx.sizes();
        Bytes a(sz.g1 * batch), b(sz.g2 * batch), c(sz.g1 * batch);
        check(hk_prove_batch(ctx.raw(), pk.device, z_rows, n_v, rs.data(), ss.data(), n_kappas ? kappas.data() : nullptr,
                             n_kappas, batch, a.data(), b.data(), c.data()),
              "hk_prove_batch");
        std::vector<Proof> out(batch);
        for (size_t k = 0; k < batch; k++) {
            out[k].a.assign(a.begin() + k * sz.g1, a.begin() + (k + 1) * sz.g1);
            out[k].b.assign(b.begin() + k * sz.g2, b.begin() + (k + 1) * sz.g2);
            out[k].c.assign(c.begin() + k * sz.g1, c.begin() + (k + 1) * sz.g1);
        }
        return out;
    }
};

class CommitmentBuilder {                                              // committer.rs:17-123
public:
    MultiStageConstraintSystem cs;
    MultiStageConstraintSynthesizer& circuit;
    CommitmentBuilder(const Context& ctx, MultiStageConstraintSynthesizer& c, ProvingKey& pk, const Bytes& one_mont)
        : cs(ctx.sizes().fr, one_mont), circuit(c), ctx_(ctx), pk_(pk) {
        if (!pk.device) throw std::logic_error("proving key not resident: call ProvingKey::upload (no CPU path)");
    }
    // committer.rs:55-98; returns (commitment, randomness) — randomness is the FIRST draw of rng
    std::pair<Bytes, Bytes> commit(const FrRng& rng) {
        circuit.generate_constraints(cur_stage_, cs);
        Bytes w = cs.current_stage_witness_assignment();
        if (cur_stage_ >= pk_.ck_deltas_abc_g.size()) throw std::out_of_range("no more values left in committing key");
        Bytes randomness = rng();
        Bytes com(ctx_.sizes().g1);
        check(hk_commit(ctx_.raw(), pk_.device, cur_stage_, w.empty() ? nullptr : w.data(), w.size() / ctx_.sizes().fr,
                        randomness.data(), com.data()), "hk_commit");   // HK_ERR_LEN <=> committer.rs:83 assert
        cur_stage_++;
        return {com, randomness};
    }
    // committer.rs:100-123
    Proof prove(const std::vector<Bytes>& comms, const std::vector<Bytes>& comm_rands, const FrRng& rng) {
        if (pk_.deltas_g.size() / ctx_.sizes().g1 != comm_rands.size() + 1)
            throw std::logic_error("assert_eq!(pk.deltas_g.len(), comm_rands.len() + 1)");   // committer.rs:112
        Bytes r = rng(), s = rng();                                      // prover.rs:28-29
        Proof p = CPGroth16::prove_last_stage(ctx_, cs, circuit, pk_, r, s, comm_rands);
        p.ds = comms;
        return p;
    }
private:
    const Context& ctx_;
    ProvingKey& pk_;
    size_t cur_stage_ = 0;
};

// ---- worker protocol (distributed-prover/src/worker.rs) -----------------------------------------------
struct Stage0Response { uint64_t subcircuit_idx; Bytes com; std::array<uint8_t, 32> com_seed; };   // :20-25
struct Stage1Response { uint64_t subcircuit_idx; Proof proof; };                                   // :49-52

}  // namespace hekaton
