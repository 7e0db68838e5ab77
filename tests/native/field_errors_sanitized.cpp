// CPU-only check of the host arithmetic behind the per-frame error blocks (csrc/psm_errors.cpp) under AddressSanitizer + UBSan:
// raw rows summed from random fields go through psm_error_metrics_from_sums and are compared with the metrics taken straight
// from the arrays (the statements of surrogate.error_metrics); the corner rows -- no finite difference, a NaN truth, a variance
// that rounds below zero, infinities from an empty min / max -- must come back as NaN, never trap.
// Built and run by tests/test_field_errors.py with g++ -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "psm.h"
#include "psm_errors.h"

static bool close(double got, double want, double rel) {
  if (std::isnan(want)) return std::isnan(got);
  return std::fabs(got - want) <= rel * std::fabs(want);
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::mt19937_64 rng(11);
  std::normal_distribution<double> gauss(0.0, 1.0);
  int rows = 0;
  for (int trial = 0; trial < 200; ++trial) {
    const int npix = 1 + (int)(rng() % 5000);
    const double offset = gauss(rng) * (trial % 3), scale = std::exp(gauss(rng) * 3.0);
    std::vector<double> pred(npix), truth(npix);
    double raw[PSM_ERR_RAW] = {0, 0, 0, inf, -inf, inf, -inf, 0};
    for (int i = 0; i < npix; ++i) {
      truth[i] = gauss(rng) * scale;
      pred[i] = truth[i] + (gauss(rng) * 0.1 + offset) * scale;
      if (rng() % 97 == 0) pred[i] = nan;
      if (trial % 7 == 6 && i == npix / 2) truth[i] = nan;
      if (truth[i] != truth[i]) raw[PSM_ERR_TNAN] += 1.0;
      else { raw[PSM_ERR_TMIN] = std::fmin(raw[PSM_ERR_TMIN], truth[i]); raw[PSM_ERR_TMAX] = std::fmax(raw[PSM_ERR_TMAX], truth[i]); }
      if (pred[i] == pred[i]) { raw[PSM_ERR_PMIN] = std::fmin(raw[PSM_ERR_PMIN], pred[i]); raw[PSM_ERR_PMAX] = std::fmax(raw[PSM_ERR_PMAX], pred[i]); }
      const double d = pred[i] - truth[i];
      if (d == d) { raw[PSM_ERR_N] += 1.0; raw[PSM_ERR_S1] += d; raw[PSM_ERR_S2] += d * d; }
    }
    double out[PSM_MET_COUNT];
    if (psm_error_metrics_from_sums(raw, out) != PSM_OK) { std::printf("trial %d: not PSM_OK\n", trial); return 1; }
    ++rows;
    const double n = raw[PSM_ERR_N];
    if (n == 0.0) {
      for (double v : out) if (!std::isnan(v)) { std::printf("trial %d: n == 0 must give NaN\n", trial); return 1; }
      continue;
    }
    const double norm = raw[PSM_ERR_TNAN] > 0 ? nan : raw[PSM_ERR_TMAX] - raw[PSM_ERR_TMIN];
    const double bias = raw[PSM_ERR_S1] / n / norm * 100, rmse = std::sqrt(raw[PSM_ERR_S2] / n) / norm * 100;
    const double var = rmse * rmse - bias * bias;
    const double want[PSM_MET_COUNT] = {norm, bias, var < 0 ? nan : std::sqrt(var), rmse, raw[PSM_ERR_S1] / n / norm, raw[PSM_ERR_S2] / n / (norm * norm)};
    if (!(std::isnan(norm) ? std::isnan(out[PSM_MET_NORM]) : out[PSM_MET_NORM] == norm)) { std::printf("trial %d: normVal\n", trial); return 1; }
    for (int q = 1; q < PSM_MET_COUNT; ++q)
      if (!close(out[q], want[q], 1e-12)) { std::printf("trial %d: metric %d is %.17g, expected %.17g\n", trial, q, out[q], want[q]); return 1; }
  }
  // corner rows
  const double corners[][PSM_ERR_RAW] = {
      {0, 0, 0, inf, -inf, inf, -inf, 0},              // an all-zero mask
      {0, 0, 0, -1, 1, inf, -inf, 0},                  // flow cells, every difference NaN
      {10, 1, 2, -1, 1, -1, 1, 1},                     // one NaN truth: np.max is NaN
      {4, 4, 4 * (1 - 1e-17), 0, 1, 0, 1, 0},          // rmse^2 < bias^2 after rounding
      {3, 3, 2.9999999, 0, 1, 0, 1, 0},                // rmse^2 < bias^2 outright
      {5, 1, 1, 2, 2, 0, 1, 0},                        // a constant truth: norm == 0, divisions by zero
      {5, inf, inf, 0, 1, 0, inf, 0},                  // overflowed sums
      {nan, nan, nan, nan, nan, nan, nan, nan}};
  for (const auto& raw : corners) {
    double out[PSM_MET_COUNT];
    if (psm_error_metrics_from_sums(raw, out) != PSM_OK) { std::printf("corner row: not PSM_OK\n"); return 1; }
    ++rows;
  }
  double out[PSM_MET_COUNT];
  psm_error_metrics_from_sums(corners[0], out);
  for (double v : out) if (!std::isnan(v)) { std::printf("n == 0 must give NaN\n"); return 1; }
  psm_error_metrics_from_sums(corners[2], out);
  for (double v : out) if (!std::isnan(v)) { std::printf("tnan > 0 must give NaN\n"); return 1; }
  psm_error_metrics_from_sums(corners[4], out);
  if (!std::isnan(out[PSM_MET_STDE]) || std::isnan(out[PSM_MET_RMSE]) || std::isnan(out[PSM_MET_BIAS])) { std::printf("negative variance must give NaN stde only\n"); return 1; }
  if (psm_error_metrics_from_sums(nullptr, out) != PSM_ERR_ARG || psm_error_metrics_from_sums(corners[0], nullptr) != PSM_ERR_ARG) {
    std::printf("null arguments must be refused\n");
    return 1;
  }
  std::printf("rows checked: %d\n", rows);
  return 0;
}
