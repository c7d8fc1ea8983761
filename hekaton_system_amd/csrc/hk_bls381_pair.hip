// Pairing and proof-verification kernels for CurveBls381 (explicit instantiation; see msm_driver.cuh)
#include "verify.cuh"
namespace hk {
extern template struct MsmRun<CurveBls381::Fq>;
}
template struct hk::PairRun<hk::Bls381FqP>;
template struct hk::VerifyRun<hk::Bls381FqP>;
