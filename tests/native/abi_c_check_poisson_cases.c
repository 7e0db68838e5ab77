/* The case-set entries of the Poisson-model step at the solver boundary are plain C like the rest of include/psm.h: compiled with
 * `gcc -std=c99 -pedantic -Wall -Werror` by tests/test_poisson_cases_abi.py (no linking, no GPU).  The function pointers pin the
 * prototypes a cgo / JNI / Fortran binding would declare. */
#include <stddef.h>

#include "psm.h"

int use_the_poisson_cases_entries(void) {
  int (*f1)(psm_handle*, double, double, int32_t, int32_t) = psm_bind_poisson_solve_cases;
  int (*f2)(psm_handle*, const double*) = psm_poisson_solve_push_cases;
  int (*f3)(psm_handle*, const double*, double*) = psm_solve_cases_poisson;
  int (*f4)(psm_handle*, const double*, double*, float*, double*, void*) = psm_solve_cases_poisson_device;
  return (f1 != 0) + (f2 != 0) + (f3 != 0) + (f4 != 0) + PSM_ABI_VERSION;
}
