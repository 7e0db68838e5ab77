/* The entries of the gradient-model step at the solver boundary are plain C like the rest of include/psm.h: compiled with
 * `gcc -std=c99 -pedantic -Wall -Werror` by tests/test_gradp_solve_abi.py (no linking, no GPU).  The function pointers pin the
 * prototypes a cgo / JNI / Fortran binding would declare. */
#include <stddef.h>

#include "psm.h"

int use_the_gradp_solve_entries(void) {
  int (*f1)(psm_handle*, int32_t, int32_t, double, double, double, double, const double*, int32_t, int32_t) = psm_bind_gradp_solve;
  int (*f2)(psm_handle*, const int32_t*, const int32_t*, double, double, double, double, const double*, int32_t, int32_t) = psm_bind_gradp_solve_cases;
  int (*f3)(psm_handle*) = psm_unbind_gradp_solve;
  int (*f4)(psm_handle*, const double*, int64_t, int32_t, double*) = psm_solve_gradp;
  int (*f5)(psm_handle*, const double*, double*, float*, float*, float*, double*, void*) = psm_solve_gradp_device;
  int (*f6)(psm_handle*, const double*, double*) = psm_solve_cases_gradp;
  int (*f7)(psm_handle*, const double*, double*, float*, float*, float*, double*, void*) = psm_solve_cases_gradp_device;
  return (f1 != 0) + (f2 != 0) + (f3 != 0) + (f4 != 0) + (f5 != 0) + (f6 != 0) + (f7 != 0) + PSM_GRADP_REF_NONE + PSM_GRADP_REF_OUTLET +
         PSM_ABI_VERSION;
}
