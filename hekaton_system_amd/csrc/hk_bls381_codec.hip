// Compressed-point kernels for CurveBls381 (explicit instantiation; see msm_driver.cuh)
#include "point_codec.cuh"
template struct hk::CodecRun<hk::Bls381FqP>;
