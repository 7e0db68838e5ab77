/* The case-batch entries of the solver boundary are plain C like the rest of include/psm.h: compiled with
 * `gcc -std=c99 -pedantic -Wall -Werror` by tests/test_mesh_cases.py (no linking, no GPU).  The function pointers pin the
 * prototypes a cgo / JNI / Fortran binding would declare. */
#include <stddef.h>

#include "psm.h"

int use_the_case_batch_entries(void) {
  int (*f1)(psm_handle*, int32_t, const int64_t*, int32_t, int32_t, const int32_t* const*, const double* const*,
            const int32_t* const*, const double* const*, const int32_t* const*, const double* const*, const double*, int32_t,
            int32_t, double) = psm_set_geometry_cases;
  int (*f2)(psm_handle*, int32_t, const double* const*, const int64_t*, const double* const*, const int64_t*,
            const double* const*, const int64_t*) = psm_init_geometry_cases;
  int (*f3)(psm_handle*, const double*, double*, void*) = psm_solve_cases_device;
  int (*f4)(psm_handle*, const double*, double*) = psm_solve_cases;
  int (*f5)(psm_handle*, const double*, double*) = psm_solve_cases_begin;
  int (*f6)(psm_handle*) = psm_solve_cases_end;
  int (*f7)(const psm_handle*, int32_t*, int64_t*) = psm_mesh_cases;
  return (f1 != 0) + (f2 != 0) + (f3 != 0) + (f4 != 0) + (f5 != 0) + (f6 != 0) + (f7 != 0) + PSM_ABI_VERSION;
}
