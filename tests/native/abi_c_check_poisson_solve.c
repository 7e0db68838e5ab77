/* The entries of the Poisson-model step at the solver boundary are plain C like the rest of include/psm.h: compiled with
 * `gcc -std=c99 -pedantic -Wall -Werror` by tests/test_poisson_solve_abi.py (no linking, no GPU).  The function pointers pin the
 * prototypes a cgo / JNI / Fortran binding would declare. */
#include <stddef.h>

#include "psm.h"

int use_the_poisson_solve_entries(void) {
  int (*f1)(psm_handle*, double, double, int32_t, int32_t) = psm_bind_poisson_solve;
  int (*f2)(psm_handle*) = psm_unbind_poisson_solve;
  int (*f3)(psm_handle*, const double*, int64_t) = psm_poisson_solve_push;
  int (*f4)(psm_handle*) = psm_poisson_solve_reset;
  int (*f5)(const psm_handle*, int32_t*, int64_t*) = psm_poisson_solve_state;
  int (*f6)(psm_handle*, const double*, int64_t, int32_t, double*) = psm_solve_poisson;
  int (*f7)(psm_handle*, const double*, double*, float*, double*, void*) = psm_solve_poisson_device;
  return (f1 != 0) + (f2 != 0) + (f3 != 0) + (f4 != 0) + (f5 != 0) + (f6 != 0) + (f7 != 0) + PSM_ABI_VERSION;
}
