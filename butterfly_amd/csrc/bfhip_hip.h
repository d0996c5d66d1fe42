/* bfhip_hip.h -- the device layer's one translation of a HIP status into the library's error (code + recorded message).
 * Included by every .hip file after <hip/hip_runtime.h>; the C host never sees a hipError_t. */
#ifndef BFHIP_HIP_H
#define BFHIP_HIP_H

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"

static inline int bfHipFail(hipError_t e, char const *what) {
  if (e == hipSuccess) return 0;
  int code = (e == hipErrorOutOfMemory) ? BFABI_ERROR_MEMORY_ERROR : BFABI_ERROR_RUNTIME_ERROR;
  return bfhipFail(code, "%s: %s", what, hipGetErrorString(e));
}

#endif
