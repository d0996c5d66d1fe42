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

/* *d = a fresh device copy of h[0..count) (the builder's problem lists and tables) */
template <typename T> static inline int uploadArrayB(T **d, T const *h, uint64_t count, char const *what) {
  *d = NULL;
  int rc = bfHipFail(hipMalloc((void **)d, count * sizeof(T)), what);
  if (rc) return rc;
  return bfHipFail(hipMemcpy(*d, h, count * sizeof(T), hipMemcpyHostToDevice), what);
}

#endif
