/* The delta-step entries of the solver boundary are plain C like the rest of include/psm.h: compiled with
 * `gcc -std=c99 -pedantic -Wall -Werror` by tests/test_delta_abi.py (no linking, no GPU).  The function pointers pin the
 * prototypes a cgo / JNI / Fortran binding would declare. */
#include <stddef.h>

#include "psm.h"

int use_the_delta_entries(void) {
  int (*f1)(psm_handle*, const double*, int64_t) = psm_delta_prime;
  int (*f2)(psm_handle*) = psm_delta_reset;
  int (*f3)(const psm_handle*, int32_t*, int64_t*) = psm_delta_state;
  int (*f4)(psm_handle*, const double*, int64_t, int32_t, double*) = psm_solve_delta;
  int (*f5)(psm_handle*, const double*, int64_t, int32_t, double*) = psm_solve_delta_begin;
  int (*f6)(psm_handle*) = psm_solve_delta_end;
  int (*f7)(psm_handle*, const double*) = psm_delta_prime_cases;
  int (*f8)(psm_handle*, const double*, double*, void*) = psm_solve_cases_delta_device;
  int (*f9)(psm_handle*, const double*, double*) = psm_solve_cases_delta;
  int (*f10)(psm_handle*, const double*, double*) = psm_solve_cases_delta_begin;
  int (*f11)(psm_handle*) = psm_solve_cases_delta_end;
  return (f1 != 0) + (f2 != 0) + (f3 != 0) + (f4 != 0) + (f5 != 0) + (f6 != 0) + (f7 != 0) + (f8 != 0) + (f9 != 0) + (f10 != 0) +
         (f11 != 0) + PSM_ABI_VERSION;
}
