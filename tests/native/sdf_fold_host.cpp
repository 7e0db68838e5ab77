// Host side of the SDF fold (csrc/psm_fold.cpp) on its own, built with -fsanitize=address,undefined by tests/test_sdf_fold_host.py:
// the packed basis over the leading channels unpacks to comp_in without its SDF columns, and sdf_coeffs equals a naive double loop.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "psm_fold.h"

static int check(int c_in) {
  const int S = 128, P = 33, B = 6, NT = 2, ny = 300, nx = 333;
  const int64_t SS = (int64_t)S * S, K = SS * c_in, KC = SS * (c_in - 1);
  std::mt19937_64 rng(17 + c_in);
  std::normal_distribution<double> nd(0.0, 1.0);
  std::vector<double> comp((size_t)P * K);
  for (double& v : comp) v = nd(rng) * 0.01;
  int bad = 0;
  // (1) pack -> unpack == comp without the last channel, rounded to float32; padded components are zero
  const std::vector<float> pack = psm_fold::pack_comp_in_fold(comp.data(), P, c_in, S, NT);
  if (pack.size() != (size_t)(SS / 64) * NT * (8 * (c_in - 1)) * 64 * 4) { printf("c_in %d: pack size %zu\n", c_in, pack.size()); return 1; }
  const std::vector<float> un = psm_fold::unpack_comp_in_fold(pack, P, c_in, S, NT);
  for (int p = 0; p < P && bad < 5; ++p)
    for (int64_t q = 0; q < SS; ++q)
      for (int ch = 0; ch < c_in - 1; ++ch)
        if (un[(size_t)p * KC + q * (c_in - 1) + ch] != (float)comp[(size_t)p * K + q * c_in + ch]) { ++bad; printf("c_in %d: unpack differs at p %d q %lld ch %d\n", c_in, p, (long long)q, ch); break; }
  double pad = 0.0;                                       // lanes of components P .. 32 NT - 1
  {
    const int G = 8 * (c_in - 1);
    for (size_t s = 0; s < (size_t)(SS / 64); ++s)
      for (int g = 0; g < G; ++g)
        for (int l = 0; l < 64; ++l)
          if (32 * (NT - 1) + (l & 31) >= P)
            for (int j = 0; j < 4; ++j) pad += std::fabs(pack[((((s * NT) + NT - 1) * G + g) * 64 + l) * 4 + j]);
  }
  if (pad != 0.0) { ++bad; printf("c_in %d: padded components not zero\n", c_in); }
  // (2) c_sdf against the naive double loop, one thread and several
  const std::vector<float> rows = psm_fold::last_channel_rows(comp.data(), P, c_in, S);
  std::vector<float> sdf((size_t)ny * nx), mean((size_t)SS);
  for (float& v : sdf) v = (float)std::fabs(nd(rng));
  for (float& v : mean) v = (float)(nd(rng) * 0.05);
  const int32_t yx[2 * B] = {0, 0, 0, 100, 0, nx - S, ny - S, 0, ny - S, 57, ny - S, nx - S};
  std::vector<double> want((size_t)B * P);
  for (int b = 0; b < B; ++b)
    for (int p = 0; p < P; ++p) {
      double acc = 0.0;
      for (int r = 0; r < S; ++r)
        for (int c = 0; c < S; ++c) {
          const double t = ((double)sdf[(size_t)(yx[2 * b] + r) * nx + yx[2 * b + 1] + c] - (double)mean[(size_t)r * S + c]) *
                           (double)(float)comp[(size_t)p * K + ((int64_t)r * S + c) * c_in + c_in - 1];
          acc += t;
        }
      want[(size_t)b * P + p] = acc;
    }
  for (int threads : {1, 5}) {
    std::vector<double> got((size_t)B * P, -1.0);
    psm_fold::sdf_coeffs(sdf.data(), nx, yx, B, S, rows.data(), mean.data(), P, got.data(), threads);
    double scale = 0.0;
    for (double v : want) scale = std::fmax(scale, std::fabs(v));
    for (size_t q = 0; q < want.size(); ++q)
      if (!(std::fabs(got[q] - want[q]) <= 1e-12 * scale)) { ++bad; printf("c_in %d threads %d: c_sdf[%zu] %.17g != %.17g\n", c_in, threads, q, got[q], want[q]); break; }
  }
  return bad;
}

int main() {
  int bad = 0;
  for (int c_in : {3, 4}) bad += check(c_in);
  if (bad) { printf("FAILED: %d\n", bad); return 1; }
  printf("sdf fold host routines: ok\n");
  return 0;
}
