// psm_fold.cpp -- see psm_fold.h.  No HIP call in this file.
#include "psm_fold.h"

#include <algorithm>
#include <thread>

namespace psm_fold {

template <typename T>
std::vector<float> pack_comp_in_fold(const T* comp, int P, int c_in, int S, int NT) {
  const int CH = c_in - 1, G = PIX_PER_SLICE * CH / 8, n_slices = S * S / PIX_PER_SLICE;
  const int64_t K = (int64_t)S * S * c_in;
  std::vector<float> out((size_t)n_slices * NT * G * 64 * 4, 0.f);
  for (int s = 0; s < n_slices; ++s)
    for (int t = 0; t < NT; ++t)
      for (int g = 0; g < G; ++g)
        for (int l = 0; l < 64; ++l) {
          const int p = 32 * t + (l & 31);
          if (p >= P) continue;
          float* o = &out[((((size_t)s * NT + t) * G + g) * 64 + l) * 4];
          for (int j = 0; j < 4; ++j) {
            const int kc = 8 * g + 4 * (l >> 5) + j, pix = kc / CH, ch = kc - pix * CH;
            o[j] = (float)comp[(int64_t)p * K + ((int64_t)s * PIX_PER_SLICE + pix) * c_in + ch];
          }
        }
  return out;
}
template std::vector<float> pack_comp_in_fold<double>(const double*, int, int, int, int);
template std::vector<float> pack_comp_in_fold<float>(const float*, int, int, int, int);

std::vector<float> unpack_comp_in_fold(const std::vector<float>& pack, int P, int c_in, int S, int NT) {
  const int CH = c_in - 1, G = PIX_PER_SLICE * CH / 8, n_slices = S * S / PIX_PER_SLICE;
  const int64_t KC = (int64_t)S * S * CH;
  std::vector<float> out((size_t)P * KC, 0.f);
  for (int s = 0; s < n_slices; ++s)
    for (int t = 0; t < NT; ++t)
      for (int g = 0; g < G; ++g)
        for (int l = 0; l < 64; ++l) {
          const int p = 32 * t + (l & 31);
          if (p >= P) continue;
          const float* o = &pack[((((size_t)s * NT + t) * G + g) * 64 + l) * 4];
          for (int j = 0; j < 4; ++j) out[(size_t)p * KC + (int64_t)s * PIX_PER_SLICE * CH + 8 * g + 4 * (l >> 5) + j] = o[j];
        }
  return out;
}

template <typename T>
std::vector<float> last_channel_rows(const T* comp, int P, int c_in, int S) {
  const int64_t SS = (int64_t)S * S;
  std::vector<float> out((size_t)P * SS);
  for (int p = 0; p < P; ++p)
    for (int64_t q = 0; q < SS; ++q) out[(size_t)p * SS + q] = (float)comp[((int64_t)p * SS + q) * c_in + (c_in - 1)];
  return out;
}
template std::vector<float> last_channel_rows<double>(const double*, int, int, int);
template std::vector<float> last_channel_rows<float>(const float*, int, int, int);

void sdf_coeffs(const float* sdf, int nx, const int32_t* y0x0, int B, int S, const float* comp_sdf, const float* mean_sdf, int P,
                double* out, int threads) {
  const int64_t SS = (int64_t)S * S;
  auto run = [&](int p0, int p1) {
    std::vector<double> d((size_t)SS);
    for (int b = 0; b < B; ++b) {
      const float* org = sdf + (int64_t)y0x0[2 * b] * nx + y0x0[2 * b + 1];
      for (int r = 0; r < S; ++r)
        for (int c = 0; c < S; ++c) d[(size_t)r * S + c] = (double)org[(int64_t)r * nx + c] - (double)mean_sdf[(size_t)r * S + c];
      for (int p = p0; p < p1; ++p) {
        const float* w = comp_sdf + (size_t)p * SS;
        double acc = 0.0;
        for (int64_t q = 0; q < SS; ++q) acc += d[(size_t)q] * (double)w[q];
        out[(size_t)b * P + p] = acc;
      }
    }
  };
  threads = std::max(1, std::min(threads, P));
  if (threads == 1) { run(0, P); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t) pool.emplace_back(run, (int)((int64_t)P * t / threads), (int)((int64_t)P * (t + 1) / threads));
  for (auto& th : pool) th.join();
}

}  // namespace psm_fold
