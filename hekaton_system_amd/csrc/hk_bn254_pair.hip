// Pairing and proof-verification kernels for CurveBn254 (explicit instantiation; see msm_driver.cuh)
#include "verify.cuh"
namespace hk {
extern template struct MsmRun<CurveBn254::Fq>;
}
template struct hk::PairRun<hk::Bn254FqP>;
template struct hk::VerifyRun<hk::Bn254FqP>;
