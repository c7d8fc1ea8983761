// Host orchestration for CurveBn254
#include "curve_ops_impl.cuh"
#include "ntt_host.cuh"
#include "pk.cuh"
#include "group_ops.cuh"
#include "witness_host.cuh"
#include "pairing_ops.cuh"
#include "prove_impl.cuh"
#include "keygen.cuh"
#include "exec_tree.cuh"
#include "stage1.cuh"
#include "trace_sort.cuh"
#include "r1cs_check.cuh"
#include "sha_tree.cuh"
#include "ram_witness.cuh"
#include "r1cs_job.cuh"
#include "vkd.cuh"
#include "vkd_tree.cuh"
#include "agg_scalars.cuh"
#include "class_sums.cuh"
namespace hk {
extern template struct MsmRun<CurveBn254::Fq>;
extern template struct MsmRun<CurveBn254::Fq2>;
extern template struct MsmSort<CurveBn254::Fr>;
extern template struct PairRun<CurveBn254::Fq::Params>;
extern template struct VerifyRun<CurveBn254::Fq::Params>;
extern template struct CodecRun<CurveBn254::Fq::Params>;
CurveOps* curve_ops_bn254() {
    static Ops<CurveBn254> ops;
    return &ops;
}
}
