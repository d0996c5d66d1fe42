/* bfhip_refine.c -- mixed-precision GMRES refinement: complex128 accuracy from mostly complex64 work.
 *
 * The outer loop computes TRUE residuals r = b - A x with the complex128 operator `op`; each correction A d = r is
 * solved by the GMRES of bfhip_gmres.c (bfGmresRun: CGS2 or MGS, optional left preconditioner) applying only the
 * complex64 operator `opLow`, from zero, to a loose relative tolerance; then x += d.  Per step:
 *
 *   1. r = b - A x (bfdevGmresResidual), each column scaled by 2^-e_p, e_p the binary exponent of its largest component, with
 *      the per-column |r|^2 partials of the scaled column: no sum of squares underflows or overflows;
 *   2. ||r_p|| = 2^e_p sqrt(sum), r^_p = (2^-e_p r_p) / sqrt(sum) (bfdevRefineScale).  The inner solver measures convergence as max_p |s| / max_p ||r_p||:
 *      without the scaling a column whose residual is already small would gain nothing from the inner solve.  A column
 *      whose residual is exactly zero gets the unit right-hand side 1/sqrt(n) and the scale 0;
 *   3. A_low d = r^ to innerTol, maxInner Krylov vectors;
 *   4. x_p += ||r_p|| d_p (bfdevRefineUpdate; a column of scale 0 keeps x_p bit for bit).
 *
 * The Krylov basis stays complex128, so the Gram-Schmidt kernels are the tested ones; the complex64 operator (and a
 * complex64 preconditioner) is wrapped as demote V_j -> apply -> promote into W.  The inner workspace is allocated once
 * per call.  The solve stops at tol, after maxOuter steps, or when a step does not bring the residual below half the
 * previous one (stagnation: rc 0, the residual reported as it is).  dX receives the iterate of the smallest true
 * residual seen.
 *
 * Range of b.  Every norm is taken of a column scaled by a power of two, exactly as the plain solver takes them, so the
 * solve is exactly equivariant under b -> 2^k b (x0 = NULL): x scales by 2^k bit for bit and the counts, the residual and
 * the history do not change, as long as b, A x and x themselves stay normal finite complex128 numbers.  Columns of 2^-600
 * next to columns of 2^+600 are tested; each column has its own exponent.  The inner solve
 * sees r^ only, whose components are at most 1, so the complex64 operator's narrower exponent range does not limit b.  A
 * NaN anywhere in b or x0 makes the residual NaN: the loop does not start, x0 (or zeros) comes back with rc 0.
 *
 * Every argument is checked before the "no device" test, so plan-only operators reach each refusal. */
#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#define BF_REFINE_INNER_TOL_DEFAULT 1e-6   /* include/bfhip.h: BfhipGmresRefineOptions.innerTol */

/* a complex64 operator applied to complex128 vectors: demote, apply, promote (buffers of n * nrhs complex64) */
typedef struct BfLowApply {
  BfhipOperator *op;
  void *dIn, *dOut;
  uint64_t n;
} BfLowApply;

static int applyLow(void *ctx, void const *dX, size_t nrhs, void *dY, void *stream) {
  BfLowApply const *L = ctx;
  uint64_t const count = L->n * nrhs;
  int rc = bfdevRefineDemote(dX, L->dIn, count, stream);
  if (!rc) rc = bfhipApplyDevice(L->op, L->dIn, nrhs, L->dOut, stream);
  if (!rc) rc = bfdevRefinePromote(L->dOut, dY, count, stream);
  return rc;
}

static int applyHigh(void *ctx, void const *dX, size_t nrhs, void *dY, void *stream) { return bfhipApplyDevice(ctx, dX, nrhs, dY, stream); }

static int statsOf(BfhipOperator *op, BfhipStats *st) {
  memset(st, 0, sizeof *st);
  st->structSize = sizeof *st;
  return bfhipGetStats(op, st);
}

/* everything that can be refused without a device; *n = order of the system, *lowM = the preconditioner is complex64 */
static int validate(BfhipOperator *op, BfhipOperator *opLow, BfhipGmresRefineOptions const *opt, size_t nrhs, uint64_t *n, int *lowM) {
  if (!op || !opLow || !opt) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator / options");
  BfhipStats st, sl;
  int rc = statsOf(op, &st);
  if (rc) return rc;
  if ((rc = statsOf(opLow, &sl))) return rc;
  if (st.dtype != BFHIP_C128) return bfhipFail(BFABI_ERROR_TYPE_ERROR, "refinement: the system operator must be complex128 (dtype %u)", st.dtype);
  if (sl.dtype != BFHIP_C64) return bfhipFail(BFABI_ERROR_TYPE_ERROR, "refinement: the inner operator must be complex64 (dtype %u)", sl.dtype);
  if (st.numRows != st.numCols) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "refinement needs a square operator");
  if (sl.numRows != st.numRows || sl.numCols != st.numCols)
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "the inner operator must be n x n like the system (n = %llu)", (unsigned long long)st.numRows);
  if (opt->structSize < sizeof(BfhipGmresRefineOptions)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BfhipGmresRefineOptions.structSize too small");
  *lowM = 0;
  if (opt->solveM) {
    BfhipStats sm;
    if ((rc = statsOf(opt->solveM, &sm))) return rc;
    if (sm.dtype != BFHIP_C128 && sm.dtype != BFHIP_C64) return bfhipFail(BFABI_ERROR_TYPE_ERROR, "the preconditioner must be complex128 or complex64");
    if (sm.numRows != st.numRows || sm.numCols != st.numCols) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "the preconditioner must be n x n");
    *lowM = sm.dtype == BFHIP_C64;
  }
  if (bfGmresResolveOrth(opt->orthogonalization) < 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "unknown orthogonalization %u", opt->orthogonalization);
  if (opt->maxOuter == 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "maxOuter must be positive");
  if (opt->maxInner == 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "maxInner must be positive");
  if (!(opt->tol > 0)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "tol must be positive");
  if (!(opt->innerTol >= 0)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "innerTol must be >= 0 (0 = default)");
  if (nrhs == 0 || nrhs > 0xffffu) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "nrhs out of range");
  *n = st.numRows;
  return 0;
}

/* the device of `op`; opLow and solveM must share it */
static int deviceOf(BfhipOperator *op, BfhipOperator *opLow, BfhipOperator *solveM, int *dev) {
  *dev = bfhipOperatorDevice(op);
  if (*dev < 0) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "operator has no device (compiled with BFHIP_FLAG_PLAN_ONLY)");
  if (bfhipOperatorDevice(opLow) != *dev || (solveM && bfhipOperatorDevice(solveM) != *dev))
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "the inner operator and the preconditioner must live on the operator's device");
  return 0;
}

typedef struct BfRefine {
  BfhipOperator *op;
  void const *dB;
  uint64_t n;
  size_t nrhs;
  uint32_t nb;
  void *dR, *dRhat, *dPart, *dPartScaled;
  double *dExp, *dScale, *hScale, *bnorm;
} BfRefine;

/* max_p ||b_p - A x_p|| / ||b_p|| (a column with b_p = 0: ||A x_p||) with x = NULL meaning zeros; leaves r^ and the
 * column norms of r on the device for the next correction.  A NaN anywhere makes the result NaN. */
static int trueResidual(BfRefine *R, void const *dXc, double *res, void *stream) {
  int rc = 0;
  if (dXc) rc = bfhipApplyDevice(R->op, dXc, R->nrhs, R->dR, stream);
  if (!rc) rc = bfdevGmresResidual(R->dB, dXc ? R->dR : NULL, R->dR, R->dPart, R->n, (uint32_t)R->nrhs, R->nb, R->dExp, R->dPartScaled, stream);
  if (!rc) rc = bfdevRefineScale(R->dR, R->dPartScaled, R->dExp, R->dRhat, R->dScale, R->n, (uint32_t)R->nrhs, R->nb, stream);
  if (!rc) rc = bfdevMemcpyD2HAsync(R->hScale, R->dScale, R->nrhs * sizeof(double), stream);
  if (!rc) rc = bfdevSync(stream);
  if (rc) return rc;
  double m = 0;
  for (size_t p = 0; p < R->nrhs; ++p) {
    double const v = R->bnorm[p] > 0 ? R->hScale[p] / R->bnorm[p] : R->hScale[p];
    if (v > m || isnan(v)) m = v;
    if (isnan(m)) break;
  }
  *res = m;
  return 0;
}

static int refineDevice(BfhipOperator *op, BfhipOperator *opLow, BfhipGmresRefineOptions const *opt, uint64_t n, int lowM, void const *dB, size_t nrhs,
                        void const *dX0, size_t *numOuter, size_t *numInner, double *residual, double *history, void *dX, void *stream) {
  size_t const maxOuter = opt->maxOuter;
  double const tol = opt->tol, innerTol = opt->innerTol > 0 ? opt->innerTol : BF_REFINE_INNER_TOL_DEFAULT;
  size_t const vecBytes = (size_t)n * nrhs * 16;
  BfhipOperator *const solveM = opt->solveM;
  BfGmresWork w;
  memset(&w, 0, sizeof w);
  BfRefine R;
  memset(&R, 0, sizeof R);
  R.op = op; R.dB = dB; R.n = n; R.nrhs = nrhs;
  BfLowApply low = {opLow, NULL, NULL, n}, lowPre = {solveM, NULL, NULL, n};
  void *dD = NULL, *dXalt = NULL;
  size_t k = 0, inner = 0;
  double bestRes = NAN;
  void const *best = NULL;
  int rc = 0;
#define CHECK(expr) do { rc = (expr); if (rc) goto done; } while (0)
  CHECK(bfGmresWorkInit(&w, n, opt->maxInner, nrhs, bfGmresResolveOrth(opt->orthogonalization), solveM != NULL, 0));
  R.nb = w.nb;
  CHECK(bfdevMalloc(&R.dR, vecBytes));
  CHECK(bfdevMalloc(&R.dRhat, vecBytes));
  CHECK(bfdevMalloc(&R.dPart, (size_t)w.nb * nrhs * 16));
  CHECK(bfdevMalloc(&R.dPartScaled, (size_t)w.nb * nrhs * 16));
  CHECK(bfdevMalloc((void **)&R.dExp, nrhs * sizeof(double)));
  CHECK(bfdevMalloc((void **)&R.dScale, nrhs * sizeof(double)));
  CHECK(bfdevMalloc(&dD, vecBytes));
  CHECK(bfdevMalloc(&dXalt, vecBytes));
  CHECK(bfdevMalloc(&low.dIn, (size_t)n * nrhs * 8));
  CHECK(bfdevMalloc(&low.dOut, (size_t)n * nrhs * 8));
  lowPre.dIn = low.dIn; lowPre.dOut = low.dOut;      /* the inner operator and the preconditioner run one after the other */
  R.hScale = malloc(nrhs * sizeof(double));
  R.bnorm = malloc(nrhs * sizeof(double));
  if (!R.hScale || !R.bnorm) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto done; }

  /* ||b_p||: the residual of x = 0 with every bnorm taken as 1 */
  for (size_t p = 0; p < nrhs; ++p) R.bnorm[p] = 0;
  double ignored;
  CHECK(trueResidual(&R, NULL, &ignored, stream));
  memcpy(R.bnorm, R.hScale, nrhs * sizeof(double));

  BfGmresApplyFn const pre = !solveM ? NULL : lowM ? applyLow : applyHigh;
  void *const pctx = !solveM ? NULL : lowM ? (void *)&lowPre : (void *)solveM;
  void *const bufs[2] = {dX, dXalt};
  void const *cur = dX0;                             /* NULL: zeros */
  double r;
  CHECK(trueResidual(&R, cur, &r, stream));
  if (history) { for (size_t i = 0; i <= maxOuter; ++i) history[i] = NAN; history[0] = r; }
  best = cur; bestRes = r;
  while (k < maxOuter && !(r <= tol) && isfinite(r)) {
    size_t it = 0;
    double ires = 0;
    CHECK(bfGmresRun(&w, applyLow, &low, pre, pctx, R.dRhat, NULL, innerTol, &it, &ires, dD, stream));
    inner += it;
    void *const next = cur == bufs[0] ? bufs[1] : bufs[0];
    CHECK(bfdevRefineUpdate(cur, dD, R.dScale, next, n, (uint32_t)nrhs, stream));
    cur = next;
    ++k;
    double rk;
    CHECK(trueResidual(&R, cur, &rk, stream));
    if (history) history[k] = rk;
    if (rk < bestRes) { best = cur; bestRes = rk; }   /* a step that continues always improves: `best` is never overwritten */
    int const stagnated = !(rk < 0.5 * r);
    r = rk;
    if (stagnated) break;
  }
  if (best != dX) {
    if (best) CHECK(bfdevMemcpyD2DAsync(dX, best, vecBytes, stream));
    else CHECK(bfdevMemsetAsync(dX, 0, vecBytes, stream));
  }
  CHECK(bfdevSync(stream));
  if (numOuter) *numOuter = k;
  if (numInner) *numInner = inner;
  if (residual) *residual = bestRes;
done:
  (void)bfdevSync(stream);
  bfGmresWorkRelease(&w);
  bfdevFree(R.dR); bfdevFree(R.dRhat); bfdevFree(R.dPart); bfdevFree(R.dPartScaled); bfdevFree(R.dExp); bfdevFree(R.dScale);
  bfdevFree(dD); bfdevFree(dXalt); bfdevFree(low.dIn); bfdevFree(low.dOut);
  free(R.hScale); free(R.bnorm);
  return rc;
#undef CHECK
}

int bfhipSolveGMRESRefineDevice(BfhipOperator *op, BfhipOperator *opLow, BfhipGmresRefineOptions const *opt, void const *dB, size_t nrhs,
                                void const *dX0, size_t *numOuter, size_t *numInner, double *residual, double *history, void *dX, void *stream) {
  uint64_t n = 0;
  int lowM = 0, dev = -1;
  int rc = validate(op, opLow, opt, nrhs, &n, &lowM);
  if (rc) return rc;
  if (!dB || !dX) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if ((rc = deviceOf(op, opLow, opt->solveM, &dev))) return rc;
  BfDevScope ds;
  if ((rc = bfDevEnter(&ds, dev))) return rc;
  rc = refineDevice(op, opLow, opt, n, lowM, dB, nrhs, dX0, numOuter, numInner, residual, history, dX, stream);
  bfDevLeave(&ds);
  return rc;
}

int bfhipSolveGMRESRefine(BfhipOperator *op, BfhipOperator *opLow, BfhipGmresRefineOptions const *opt, void const *B, size_t ldb, size_t nrhs,
                          void const *X0, size_t ldx0, size_t *numOuter, size_t *numInner, double *residual, double *history, void *X, size_t ldx) {
  uint64_t n = 0;
  int lowM = 0, dev = -1;
  int rc = validate(op, opLow, opt, nrhs, &n, &lowM);
  if (rc) return rc;
  if (!B || !X) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (ldb < nrhs || ldx < nrhs || (X0 && ldx0 < nrhs)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "bad leading dimension");
  if ((rc = deviceOf(op, opLow, opt->solveM, &dev))) return rc;
  size_t const vecBytes = (size_t)n * nrhs * 16;
  void *dB = NULL, *dX0 = NULL, *dX = NULL;
  BfDevScope ds;
  char *pack = malloc(vecBytes ? vecBytes : 1);
  if (!pack) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  if ((rc = bfDevEnter(&ds, dev))) { free(pack); return rc; }
  if ((rc = bfdevMalloc(&dB, vecBytes))) goto done;
  if ((rc = bfdevMalloc(&dX, vecBytes))) goto done;
  for (uint64_t i = 0; i < n; ++i) memcpy(pack + i * nrhs * 16, (char const *)B + i * ldb * 16, nrhs * 16);
  if ((rc = bfdevMemcpyH2D(dB, pack, vecBytes))) goto done;
  if (X0) {
    if ((rc = bfdevMalloc(&dX0, vecBytes))) goto done;
    for (uint64_t i = 0; i < n; ++i) memcpy(pack + i * nrhs * 16, (char const *)X0 + i * ldx0 * 16, nrhs * 16);
    if ((rc = bfdevMemcpyH2D(dX0, pack, vecBytes))) goto done;
  }
  if ((rc = refineDevice(op, opLow, opt, n, lowM, dB, nrhs, dX0, numOuter, numInner, residual, history, dX, NULL))) goto done;
  if ((rc = bfdevMemcpyD2H(pack, dX, vecBytes))) goto done;
  for (uint64_t i = 0; i < n; ++i) memcpy((char *)X + i * ldx * 16, pack + i * nrhs * 16, nrhs * 16);
done:
  bfdevFree(dB); bfdevFree(dX0); bfdevFree(dX);
  free(pack);
  bfDevLeave(&ds);
  return rc;
}
