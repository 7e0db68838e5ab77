// psm_fold.h -- host side of the SDF fold of the bound single-case encode (PsmEncodeArgs::fold): on a bound geometry whose SDF
// channel is the last one, that channel's share of the PCA coefficients is a constant of the binding.  Plain C++ (no HIP): the
// routines are also built on their own, under the sanitizers, by tests/native/sdf_fold_host.cpp.
#pragma once
#include <cstdint>
#include <vector>

namespace psm_fold {
constexpr int PIX_PER_SLICE = 64;      // == PSM_PIX_PER_SLICE (psm_kernels.h; static_assert in psm_api_model.cpp)

// comp [P][S*S*c_in] (sklearn components_, channel fastest) -> the encode's packed basis over the c_in - 1 LEADING channels, in the
// layout of pack_comp_in for a (c_in - 1)-channel slice: [slice][ntile][G = 8 (c_in - 1)][64 lanes][4] floats; element j of lane l
// in group g is comp[32 t + (l & 31)][k] with compact index k' = 8 g + 4 (l >> 5) + j -> pixel 64 slice + k' / (c_in - 1), channel
// k' % (c_in - 1); zero for padded components.  T = double (the model as given) or float (the handle's rounded copy).
template <typename T>
std::vector<float> pack_comp_in_fold(const T* comp, int P, int c_in, int S, int NT);
// inverse, for the check: packed -> [P][S*S*(c_in - 1)]
std::vector<float> unpack_comp_in_fold(const std::vector<float>& pack, int P, int c_in, int S, int NT);
// the last channel's columns of comp, rounded to float32 like the packed basis: [P][S*S]
template <typename T>
std::vector<float> last_channel_rows(const T* comp, int P, int c_in, int S);
// c_sdf[b][p] = sum over the S*S pixels q = (r, c) of block b of (sdf[(y0_b + r) nx + x0_b + c] - mean_sdf[q]) * comp_sdf[p][q], accumulated
// in double in pixel order; y0x0 [B][2]; out [B][P].  `threads` > 1 splits the components over that many host threads.
void sdf_coeffs(const float* sdf, int nx, const int32_t* y0x0, int B, int S, const float* comp_sdf, const float* mean_sdf, int P,
                double* out, int threads);
}  // namespace psm_fold
