// psm_errors.cpp -- the error summary every evaluator of the reference prints per frame (pressureSM_Poisson/SM_call.py:962-994;
// SM_call.py:696-724) from the eight sums the device reduction leaves (psm_block_error_kernel, psm_eval.hip): over the flow cells,
// with norm = max - min of the truth there and NaN differences left out,
//   BIAS = mean(pred - true) / norm, RMSE = sqrt(mean((pred - true)^2)) / norm, STDE = sqrt(RMSE^2 - BIAS^2), in percent,
// and the two values the reference appends to pred_minus_true / pred_minus_true_squared.  Statement for statement what
// surrogate.error_metrics does with the arrays: np.max of a truth with a NaN is NaN (tnan > 0), sqrt of a negative
// RMSE^2 - BIAS^2 is NaN.  Pure host code: no HIP, no handle, no GPU.
#include "psm_errors.h"

#include <cmath>
#include <limits>

#include "../../include/psm.h"

namespace psm_impl {

void error_metrics_from_sums(const double* raw, double* out) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double n = raw[PSM_ERR_N];
  if (!(n > 0.0)) {                          // NumPy raises on the empty selection; the C entry says NaN
    for (int q = 0; q < PSM_MET_COUNT; ++q) out[q] = nan;
    return;
  }
  const double norm = raw[PSM_ERR_TNAN] > 0.0 ? nan : raw[PSM_ERR_TMAX] - raw[PSM_ERR_TMIN];
  const double mean = raw[PSM_ERR_S1] / n, mean_sq = raw[PSM_ERR_S2] / n;
  const double bias = mean / norm * 100.0;
  const double rmse = std::sqrt(mean_sq) / norm * 100.0;
  const double var = rmse * rmse - bias * bias;
  out[PSM_MET_NORM] = norm;
  out[PSM_MET_BIAS] = bias;
  out[PSM_MET_STDE] = var < 0.0 ? nan : std::sqrt(var);
  out[PSM_MET_RMSE] = rmse;
  out[PSM_MET_MEAN_ERR] = mean / norm;
  out[PSM_MET_MEAN_SQ_ERR] = mean_sq / (norm * norm);
}

}  // namespace psm_impl

extern "C" int psm_error_metrics_from_sums(const double* raw, double* out) {
  if (!raw || !out) return PSM_ERR_ARG;
  psm_impl::error_metrics_from_sums(raw, out);
  return PSM_OK;
}
