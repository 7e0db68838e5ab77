// psm_errors.h -- host arithmetic behind the per-frame error blocks (see psm_errors.cpp): plain C++, no HIP, so that it builds
// with any host compiler (tests/native/field_errors_sanitized.cpp runs it under ASan / UBSan).
#pragma once

// slots of one raw row, as psm_block_error_kernel leaves them (psm_eval.hip)
enum { PSM_ERR_N = 0, PSM_ERR_S1, PSM_ERR_S2, PSM_ERR_TMIN, PSM_ERR_TMAX, PSM_ERR_PMIN, PSM_ERR_PMAX, PSM_ERR_TNAN, PSM_ERR_RAW };
// slots of the metrics: normVal, biasNorm, stdeNorm, rmseNorm (the three in percent), mean_err, mean_sq_err
enum { PSM_MET_NORM = 0, PSM_MET_BIAS, PSM_MET_STDE, PSM_MET_RMSE, PSM_MET_MEAN_ERR, PSM_MET_MEAN_SQ_ERR, PSM_MET_COUNT };

namespace psm_impl {
// raw[8] -> out[6]; n == 0 (no finite difference): all NaN
void error_metrics_from_sums(const double* raw, double* out);
}
