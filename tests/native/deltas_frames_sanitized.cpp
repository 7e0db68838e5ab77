// CPU-only check of the host arithmetic behind the rows the deltas frame entries return (csrc/psm_errors.cpp) under
// AddressSanitizer + UBSan.  A frame's block row is the fold of its B partial rows in block order -- the statements of
// psm_block_error's host loop, which the fold launch of psm_block_errors_device repeats --; this program folds partial rows of
// random blocks that way, sends the row through psm_error_metrics_from_sums and compares mean_err / mean_sq_err / normVal with the
// statements of psm_block_error's out[0] / out[1] / out[2], bit for bit.  The corner rows of a frame -- no flow cell in any block
// (n == 0), a NaN label on a flow cell (tnan > 0), a variance that rounds below zero, a frame [2][8] with one row of each kind --
// must come back as NaN where the reference's NumPy gives NaN, never trap.
// Built and run by tests/test_deltas_frames.py with g++ -fsanitize=address,undefined.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "psm.h"
#include "psm_errors.h"

static bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || a == b; }

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::mt19937_64 rng(16);
  std::normal_distribution<double> gauss(0.0, 1.0);
  int rows = 0;
  for (int trial = 0; trial < 200; ++trial) {
    const int B = 1 + (int)(rng() % 9), cells = 1 + (int)(rng() % 700);
    const double scale = std::exp(gauss(rng) * 2.0);
    std::vector<double> part((size_t)B * PSM_ERR_RAW);
    for (int b = 0; b < B; ++b) {                      // one block's partial row, as a workgroup leaves it
      double* q = &part[(size_t)b * PSM_ERR_RAW];
      const double init[PSM_ERR_RAW] = {0, 0, 0, inf, -inf, inf, -inf, 0};
      std::copy(init, init + PSM_ERR_RAW, q);
      const bool empty = trial % 5 == 4 && b % 2 == 0;  // a block without flow cells
      for (int i = 0; i < cells && !empty; ++i) {
        const float label = (float)(gauss(rng) * 0.3);
        double truth = (double)label * scale;
        const double pred = (double)(float)(truth + gauss(rng) * 0.05 * scale);
        if (trial % 11 == 10 && b == B - 1 && i == cells / 2) truth = nan;
        if (truth != truth) q[PSM_ERR_TNAN] += 1.0;
        else { q[PSM_ERR_TMIN] = std::fmin(q[PSM_ERR_TMIN], truth); q[PSM_ERR_TMAX] = std::fmax(q[PSM_ERR_TMAX], truth); }
        q[PSM_ERR_PMIN] = std::fmin(q[PSM_ERR_PMIN], pred); q[PSM_ERR_PMAX] = std::fmax(q[PSM_ERR_PMAX], pred);
        const double d = pred - truth;
        if (d == d) { q[PSM_ERR_N] += 1.0; q[PSM_ERR_S1] += d; q[PSM_ERR_S2] += d * d; }
      }
    }
    // the fold in block order
    double n = 0, s1 = 0, s2 = 0, tmin = inf, tmax = -inf, pmin = inf, pmax = -inf, tnan = 0;
    for (int b = 0; b < B; ++b) {
      const double* q = &part[(size_t)b * PSM_ERR_RAW];
      n += q[0]; s1 += q[1]; s2 += q[2]; tnan += q[7];
      tmin = std::min(tmin, q[3]); tmax = std::max(tmax, q[4]); pmin = std::min(pmin, q[5]); pmax = std::max(pmax, q[6]);
    }
    const double raw[PSM_ERR_RAW] = {n, s1, s2, tmin, tmax, pmin, pmax, tnan};
    double out[PSM_MET_COUNT];
    if (psm_error_metrics_from_sums(raw, out) != PSM_OK) { std::printf("trial %d: not PSM_OK\n", trial); return 1; }
    ++rows;
    if (n == 0.0) {
      for (double v : out) if (!std::isnan(v)) { std::printf("trial %d: n == 0 must give NaN\n", trial); return 1; }
      continue;
    }
    const double norm = tnan > 0 ? nan : tmax - tmin;   // psm_block_error: out[2], out[0], out[1]
    if (!same(out[PSM_MET_NORM], norm) || !same(out[PSM_MET_MEAN_ERR], s1 / n / norm) || !same(out[PSM_MET_MEAN_SQ_ERR], s2 / n / (norm * norm))) {
      std::printf("trial %d: the row's metrics are not psm_block_error's statements\n", trial);
      return 1;
    }
    if (tnan > 0)
      for (double v : out) if (!std::isnan(v)) { std::printf("trial %d: a NaN truth must give NaN\n", trial); return 1; }
  }
  // one frame [2][8] per corner: the field's row and the blocks' row
  const double frames[][2][PSM_ERR_RAW] = {
      {{0, 0, 0, inf, -inf, inf, -inf, 0}, {0, 0, 0, inf, -inf, inf, -inf, 0}},            // no flow cell at all
      {{10, 1, 2, -1, 1, -1, 1, 0}, {0, 0, 0, -1, 1, inf, -inf, 0}},                       // blocks: every prediction NaN
      {{10, 1, 2, -1, 1, -1, 1, 1}, {40, 1, 2, -1, 1, -1, 1, 3}},                          // NaN truths
      {{4, 4, 4 * (1 - 1e-17), 0, 1, 0, 1, 0}, {3, 3, 2.9999999, 0, 1, 0, 1, 0}},          // rmse^2 < bias^2
      {{5, 1, 1, 2, 2, 0, 1, 0}, {5, inf, inf, 0, 1, 0, inf, 0}}};                         // a constant truth; overflowed sums
  double out[2][PSM_MET_COUNT];
  for (const auto& f : frames) {
    for (int r = 0; r < 2; ++r) {
      if (psm_error_metrics_from_sums(f[r], out[r]) != PSM_OK) { std::printf("corner row: not PSM_OK\n"); return 1; }
      ++rows;
    }
    const bool all_nan = &f == &frames[0] || &f == &frames[2];
    for (int r = 0; r < 2 && all_nan; ++r)
      for (double v : out[r]) if (!std::isnan(v)) { std::printf("n == 0 / tnan > 0 must give NaN\n"); return 1; }
    if (&f == &frames[1])
      for (double v : out[1]) if (!std::isnan(v)) { std::printf("n == 0 must give NaN\n"); return 1; }
    if (&f == &frames[3])
      for (int r = 0; r < 2; ++r)
        if ((r == 1 && !std::isnan(out[r][PSM_MET_STDE])) || std::isnan(out[r][PSM_MET_RMSE]) || std::isnan(out[r][PSM_MET_BIAS])) {
          std::printf("a negative variance must give a NaN stde and nothing else\n");
          return 1;
        }
  }
  if (psm_error_metrics_from_sums(nullptr, out[0]) != PSM_ERR_ARG || psm_error_metrics_from_sums(frames[0][0], nullptr) != PSM_ERR_ARG) {
    std::printf("null arguments must be refused\n");
    return 1;
  }
  std::printf("rows checked: %d\n", rows);
  return 0;
}
