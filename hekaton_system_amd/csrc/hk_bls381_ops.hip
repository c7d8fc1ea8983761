// Host orchestration for CurveBls381
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
extern template struct MsmRun<CurveBls381::Fq>;
extern template struct MsmRun<CurveBls381::Fq2>;
extern template struct MsmSort<CurveBls381::Fr>;
extern template struct PairRun<CurveBls381::Fq::Params>;
extern template struct VerifyRun<CurveBls381::Fq::Params>;
extern template struct CodecRun<CurveBls381::Fq::Params>;
CurveOps* curve_ops_bls381() {
    static Ops<CurveBls381> ops;
    return &ops;
}
}
