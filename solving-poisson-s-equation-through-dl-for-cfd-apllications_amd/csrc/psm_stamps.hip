// psm_stamps.hip -- psm_read_stamps, and under -DPSM_STAMPS (make stamps) the one translation unit of the PCA-path stage files,
// which then share the stamp slots of psm_stamps.h.  The shipped library compiles each stage file on its own.
#include "psm_kernels.h"
#include "psm_stamps.h"

#ifdef PSM_STAMPS
#include "psm_encode.hip"
#include "psm_dense.hip"
#include "psm_decode.hip"
#include "psm_assemble.hip"
#include "psm_bound.hip"
hipError_t psm_read_stamps(unsigned long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_psm_stamps), sizeof(g_psm_stamps)); }
#else
hipError_t psm_read_stamps(unsigned long long* out) { for (int i = 0; i < 64; ++i) out[i] = 0; return hipSuccess; }
#endif
