// ensemble_batched_host.cpp -- a bare C-ABI host (include/psm.h only) that advances an ensemble of PISO cases at the solver
// boundary as ONE batch: every case has its own mesh and obstacle, all share one grid shape, and one psm_solve_cases call per
// time step advances them all on one handle (one launch chain, not one per case as with psm_solve_begin / psm_solve_end).
//
//   g++ -std=c++17 -O2 -I include examples/ensemble_batched_host.cpp -L <dir of libpsm_hip.so> -lpsm_hip -o ensemble_batched_host
//   ./ensemble_batched_host ensemble.bin
//
// ensemble.bin (written by tests/test_mesh_cases.py): int32 header {p_in, p_out, n_dense, n_cases, n_steps}; float64 comp_in,
// mean_in, comp_out, mean_out, {in_a, out_a}, maxs[4]; per layer int32 {n_in, n_out}, float32 kernel, float32 bias; per case
// int32 {n, n_top, n_obst}, float64 top [n_top,2], obst [n_obst,2], then n_steps times cells [n,5] (Ux, Uy, Cx, Cy, p).
// Prints, per step and case, the sum of the bit patterns of p modulo 2^64 (an order-free checksum the test recomputes).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "psm.h"

#define CHECK(call)                                                                                     \
  do { const int rc_ = (call); if (rc_ != PSM_OK) { std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, psm_last_error(sm)); return 2; } } while (0)

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s ensemble.bin\n", argv[0]); return 1; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 1; }
  int32_t hd[5];
  if (std::fread(hd, sizeof(int32_t), 5, f) != 5) return 1;
  const int p_in = hd[0], p_out = hd[1], n_dense = hd[2], K = hd[3], n_steps = hd[4];
  const size_t Kp = 128u * 128u * 3, Ko = 128u * 128u;
  std::vector<double> comp_in, mean_in, comp_out, mean_out, sc, maxs;
  if (!rd(f, comp_in, p_in * Kp) || !rd(f, mean_in, Kp) || !rd(f, comp_out, p_out * Ko) || !rd(f, mean_out, Ko) || !rd(f, sc, 2) || !rd(f, maxs, 4)) return 1;

  psm_handle* sm = nullptr;
  psm_config cfg = {PSM_ABI_VERSION, PSM_VARIANT_CHAPTER5, 128, 0, 3, 1, p_in, p_out, n_dense, PSM_SCALER_MAX_ABS, 2, 0, /*max_cases*/ K, 0, PSM_PRECISION_F32};
  if (psm_create(&cfg, &sm) != PSM_OK) { std::fprintf(stderr, "psm_create: %s\n", psm_last_error(nullptr)); return 2; }
  CHECK(psm_set_pca(sm, comp_in.data(), mean_in.data(), comp_out.data(), mean_out.data()));
  CHECK(psm_set_scaler(sm, &sc[0], &sc[0], &sc[1], &sc[1]));
  for (int l = 0; l < n_dense; ++l) {
    int32_t sh[2];
    std::vector<float> W, b;
    if (std::fread(sh, sizeof(int32_t), 2, f) != 2 || !rd(f, W, (size_t)sh[0] * sh[1]) || !rd(f, b, sh[1])) return 1;
    CHECK(psm_set_dense(sm, l, sh[0], sh[1], W.data(), b.data()));
  }

  // the cases: boundary points once, the cell arrays of every time step
  std::vector<int64_t> n(K), n_top(K), n_obst(K);
  std::vector<std::vector<double>> top(K), obst(K);
  std::vector<std::vector<std::vector<double>>> cells(K, std::vector<std::vector<double>>(n_steps));
  for (int k = 0; k < K; ++k) {
    int32_t c[3];
    if (std::fread(c, sizeof(int32_t), 3, f) != 3) return 1;
    n[k] = c[0]; n_top[k] = c[1]; n_obst[k] = c[2];
    if (!rd(f, top[k], (size_t)c[1] * 2) || !rd(f, obst[k], (size_t)c[2] * 2)) return 1;
    for (int s = 0; s < n_steps; ++s)
      if (!rd(f, cells[k][s], (size_t)c[0] * 5)) return 1;
  }
  std::fclose(f);

  // init_func of all cases: tables built in C++ per case, K geometries bound, every per-step buffer reserved
  std::vector<const double*> pc(K), pt(K), po(K);
  for (int k = 0; k < K; ++k) { pc[k] = cells[k][0].data(); pt[k] = top[k].data(); po[k] = obst[k].data(); }
  CHECK(psm_set_case(sm, maxs.data(), 5e-3, 10, 0.05));
  CHECK(psm_init_geometry_cases(sm, K, pc.data(), n.data(), pt.data(), n_top.data(), po.data(), n_obst.data()));
  int32_t kk = 0;
  std::vector<int64_t> off(K + 1);
  CHECK(psm_mesh_cases(sm, &kk, off.data()));

  // the time loop: the solver's cell arrays side by side in one buffer, one call per step
  std::vector<double> all((size_t)off[K] * 5), p((size_t)off[K]);
  for (int s = 0; s < n_steps; ++s) {
    for (int k = 0; k < K; ++k) std::memcpy(&all[(size_t)off[k] * 5], cells[k][s].data(), (size_t)n[k] * 5 * sizeof(double));
    CHECK(psm_solve_cases(sm, all.data(), p.data()));
    for (int k = 0; k < K; ++k) {
      uint64_t sum = 0;
      for (int64_t i = off[k]; i < off[k + 1]; ++i) { uint64_t b; std::memcpy(&b, &p[(size_t)i], 8); sum += b; }
      std::printf("step %d case %d cells %lld checksum %016llx\n", s, k, (long long)n[k], (unsigned long long)sum);
    }
  }
  psm_destroy(sm);
  return 0;
}
