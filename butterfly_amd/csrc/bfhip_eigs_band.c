/* bfhip_eigs_band.c -- successive eigenbands by deflation (bfhipChebCovEigsBandDevice, bfhipChebCovEigsMassNormaliseDevice,
 * include/bfhip.h).  The iteration is bfhip_eigs.c's (bfEigsSolve); this file gives it the projection
 * against the locked block, whose kernels are bfhip_eigs.hip's, and holds the in-place mass normalisation. */
#include <stdint.h>

#include "bfhip_internal.h"
#include "../../include/bfhip.h"
#include "../../include/bfhip_abi.h"

int bfhipChebCovEigsBandDevice(BfhipChebCov *c, BfhipEigsOptions const *opt, BfhipEigsLocked const *locked, size_t nev, double *lam, double *residual,
                               double *dU, size_t ldu, BfhipEigsInfo *info, void *stream) {
  static BfEigsDeflation const defl = { bfdevEigsProject, bfdevEigsCrossChunkRows };
  return bfEigsSolve(c, opt, locked, &defl, nev, lam, residual, dU, ldu, info, stream);
}

/* the store kernel with source and destination the same block: an element's owner is its only reader */
int bfhipChebCovEigsMassNormaliseDevice(BfhipChebCov *c, double *dU, size_t ldu, size_t count, void *stream) {
  if (!c || (!dU && count)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (ldu < count) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "ldu is less than count");
  if (ldu > UINT32_MAX) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "ldu is more than 2^32 - 1");
  if (!count || !c->n) return 0;
  BfDevScope ds = {0};
  int rc = bfDevEnter(&ds, c->device);
  if (rc) return rc;
  if (!(rc = bfdevEigsStore(dU, c->n, (uint32_t)ldu, (uint32_t)count, (double const *)c->dD, dU, ldu, stream))) rc = bfdevSync(stream);
  bfDevLeave(&ds);
  return rc;
}
