// Compressed-point kernels for CurveBn254 (explicit instantiation; see msm_driver.cuh)
#include "point_codec.cuh"
template struct hk::CodecRun<hk::Bn254FqP>;
