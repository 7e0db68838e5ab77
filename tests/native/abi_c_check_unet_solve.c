/* The mesh binding of the convolutional path is plain C like the rest of include/psm_unet.h: compiled with
 * `gcc -std=c99 -pedantic -Wall -Werror` by tests/test_unet_solve_abi.py (no linking, no GPU).  The function pointers pin the
 * prototypes a cgo / JNI / Fortran binding would declare. */
#include <stddef.h>

#include "psm.h"
#include "psm_unet.h"

int use_the_unet_mesh_entries(void) {
  int (*f1)(int32_t, int32_t, int32_t, int32_t*, int32_t*) = psm_unet_canvas_shape;
  int (*f2)(psm_unet*, int32_t, int32_t, int32_t, int32_t, int32_t, psm_unet_mesh**) = psm_unet_mesh_create;
  void (*f3)(psm_unet_mesh*) = psm_unet_mesh_destroy;
  const char* (*f4)(const psm_unet_mesh*) = psm_unet_mesh_last_error;
  int (*f5)(psm_unet_mesh*, int32_t, const int64_t*, int32_t, int32_t, const int32_t* const*, const double* const*, const int32_t* const*,
            const double* const*, const int32_t* const*, const double* const*, const double*, int32_t, int32_t, double) = psm_unet_mesh_set_geometry;
  int (*f6)(psm_unet_mesh*, const double*, double*) = psm_unet_solve;
  int (*f7)(psm_unet_mesh*, const double*, double*, void*) = psm_unet_solve_device;
  int (*f8)(psm_unet_mesh*, const double*) = psm_unet_mesh_prime;
  int (*f9)(psm_unet_mesh*) = psm_unet_mesh_reset;
  int (*f10)(const psm_unet_mesh*, int32_t*, int64_t*) = psm_unet_mesh_state;
  int (*f11)(psm_unet_mesh*, int32_t, void*, int64_t) = psm_unet_mesh_read;
  return (f1 != 0) + (f2 != 0) + (f3 != 0) + (f4 != 0) + (f5 != 0) + (f6 != 0) + (f7 != 0) + (f8 != 0) + (f9 != 0) + (f10 != 0) + (f11 != 0) +
         PSM_UNET_STEP_ABSOLUTE + PSM_UNET_STEP_DELTA + PSM_UNET_READ_CANVAS + PSM_UNET_READ_FIELD + PSM_UNET_READ_UMAX + PSM_ABI_VERSION;
}
