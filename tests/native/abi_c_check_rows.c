/* The rows entries (a frame's dataset rows -> scalars + columns on the device, and the evaluators' steps behind that stage) are
 * plain C like the rest of include/psm.h: compiled with `gcc -std=c99 -pedantic -Wall -Werror` by tests/test_rows_abi.py (no
 * linking, no GPU).  The function pointers pin the prototypes a cgo / JNI / Fortran binding would declare. */
#include <stddef.h>

#include "psm.h"

int use_the_rows_entries(void) {
  int (*f1)(psm_handle*, int32_t) = psm_bind_rows;
  int (*f2)(psm_handle*) = psm_unbind_rows;
  int (*f3)(psm_handle*, int32_t, const float*, int32_t, int64_t, int32_t, const double*, double*, double*, void*) = psm_rows_prepare_device;
  int (*f4)(psm_handle*, const float*, int32_t, int32_t, double, int32_t, float*, double*, double*, double*, void*) = psm_deltas_rows_device;
  int (*f5)(psm_handle*, const float*, int32_t, int32_t, double, int32_t, float*, double*, double*, double*) = psm_deltas_rows;
  int (*f6)(psm_handle*, const float*, int32_t, int32_t, double, double, int32_t, int32_t, double*, float*, float*, float*, double*,
            void*) = psm_poisson_rows_device;
  int (*f7)(psm_handle*, const float*, int32_t, int32_t, double, double, int32_t, int32_t, double*, float*, float*, float*, double*) =
      psm_poisson_rows;
  int (*f8)(psm_handle*, const float*, int32_t, int32_t, double, double, int32_t, int32_t, double*, float*, float*, float*, double*,
            double*, void*) = psm_poisson_rows_errors_device;
  int (*f9)(psm_handle*, const float*, int32_t, int32_t, double, double, int32_t, int32_t, double*, double*) = psm_poisson_rows_errors;
  int (*f10)(psm_handle*, const float*, int32_t, int32_t, double, double, int32_t, float*, float*, double*, double*, double*, void*) =
      psm_gradp_rows_device;
  int (*f11)(psm_handle*, const float*, int32_t, int32_t, double, double, int32_t, float*, float*, double*, double*, double*) =
      psm_gradp_rows;
  int kinds[3];
  kinds[PSM_ROWS_DELTAS] = 3; kinds[PSM_ROWS_POISSON] = 8; kinds[PSM_ROWS_GRADP] = 5;     /* three distinct indices below 3 */
  return (f1 != 0) + (f2 != 0) + (f3 != 0) + (f4 != 0) + (f5 != 0) + (f6 != 0) + (f7 != 0) + (f8 != 0) + (f9 != 0) + (f10 != 0) +
         (f11 != 0) + kinds[0] + kinds[1] + kinds[2] + PSM_ABI_VERSION;
}
