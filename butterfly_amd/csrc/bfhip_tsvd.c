/* bfhip_tsvd.c -- truncated SVD of a real f64 matrix on the device (bfhipTruncSvdDevice, include/bfhip.h; DESIGN.md section
 * 29): what the streamer's one numerical step needs (bfGetTruncatedSvd, reference src/linalg.c:1002-1082, cut by
 * bfTruncSpecGetNumTerms, src/linalg.c:26-35).  One-sided block Jacobi (Hestenes; the block form with a Gram-based pair solve
 * as in Becka, Oksa and Vajtersic, "Dynamic ordering for a parallel block-Jacobi SVD algorithm", Parallel Computing 28, 2002;
 * the sorting of a pair's columns by norm is de Rijk's, SIAM J. Sci. Stat. Comput. 10, 1989) on the taller orientation, no V
 * accumulated.  Host side: the argument checks, the sweep loop (one synchronisation per sweep, to read two counters), the sort
 * of the column norms, the count rule and the recovery of U and W.  The kernels are bfhip_tsvd.hip's, the geometry bfhip_tsvd.h's. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip_internal.h"
#include "../../include/bfhip.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_tsvd.h"

/* descending by norm, ties by the lower index: a total order, so the result does not depend on qsort's algorithm */
int tsvdColCmp(void const *a, void const *b) {
  TsvdCol const *x = a, *y = b;
  if (x->norm != y->norm) return x->norm > y->norm ? -1 : 1;
  return x->index < y->index ? -1 : x->index > y->index;
}

/* the reference's count (src/linalg.c:26-35): the number of leading s_j with s_j >= tol * s_0; 0 for an all-zero matrix */
uint64_t bfTsvdCount(double const *sigma, uint64_t count, double tol) {
  if (!count || !(sigma[0] > 0)) return 0;
  uint64_t k = 0;
  while (k < count && sigma[k] >= tol * sigma[0]) ++k;
  return k;
}

/* the argument checks of the entry, before the device is touched; 0 or the recorded failure */
int bfTsvdCheckArguments(double const *dA, size_t m, size_t n, size_t lda, BfhipTruncSvdOptions const *opt, double const *dSigma, double const *dU, size_t ldu,
                         size_t capU, double const *dW, size_t ldw, size_t capW, BfhipTruncSvdInfo const *info) {
  if (!dA || !opt || !dSigma) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (opt->structSize != sizeof *opt) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "structSize is not sizeof(BfhipTruncSvdOptions)");
  if (info && info->structSize != sizeof *info) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "structSize is not sizeof(BfhipTruncSvdInfo)");
  if (!(opt->tol > 0) || !(opt->tol < 1)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "tol is not in (0, 1)");
  if (opt->flags || opt->reserved) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "flags and reserved must be 0");
  size_t const N = m < n ? m : n;
  if (!N) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "min(m, n) is 0");
  if (N > BF_TSVD_MAX_DIM) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "min(m, n) is more than %u", BF_TSVD_MAX_DIM);
  if ((m > n ? m : n) > (1ull << 32)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "max(m, n) is more than 2^32");
  if (lda < n) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "lda is less than n");
  if (dU && ldu < capU) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "ldu is less than capU");
  if (dW && ldw < n) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "ldw is less than n");
  return 0;
}

/* doubles of the sweep workspace: the block, the pair-Gram partials (the column sums' partials share them), Q, the sums of squares */
uint64_t bfTsvdWorkspaceElems(uint64_t M, uint32_t ld, uint64_t *offPart, uint64_t *offQ, uint64_t *offSumSq) {
  uint64_t const pairs = ld / BF_TSVD_PAIR, rows = bfTsvdChunkRows(M, ld), chunks = (M + rows - 1) / rows;
  uint64_t off = M * ld;
  *offPart = off; off += chunks * pairs * BF_TSVD_PAIR * BF_TSVD_PAIR;
  *offQ = off; off += pairs * BF_TSVD_PAIR * BF_TSVD_PAIR;
  *offSumSq = off; off += ld;
  return off;
}

int bfhipTruncSvdDevice(int device, double const *dA, size_t m, size_t n, size_t lda, BfhipTruncSvdOptions const *opt, double *dSigma, double *dU,
                        size_t ldu, size_t capU, double *dW, size_t ldw, size_t capW, BfhipTruncSvdInfo *info, void *stream) {
  int rc = bfTsvdCheckArguments(dA, m, n, lda, opt, dSigma, dU, ldu, capU, dW, ldw, capW, info);
  if (rc) return rc;
  double const t0 = bfNowSeconds();
  int const transposed = m < n;
  uint64_t const M = transposed ? n : m, N = transposed ? m : n;
  uint32_t const ld = bfTsvdLd(N), nt = ld / BF_TSVD_TILE, pairs = nt / 2;
  uint32_t const maxSweeps = opt->maxSweeps ? opt->maxSweeps : 30;
  double const thr = bfTsvdThreshold(M), noise = bfTsvdNoise(N);
  uint64_t offPart, offQ, offSumSq;
  uint64_t const elems = bfTsvdWorkspaceElems(M, ld, &offPart, &offQ, &offSumSq);
  uint64_t bytes = elems * 8 + (uint64_t)pairs * 4 + sizeof(BfTsvdSweepState);
  void *dAll = NULL, *dFin = NULL;
  TsvdCol *cols = NULL;
  double *host = NULL;
  uint32_t *perm = NULL;
  uint32_t sweeps = 0;
  uint64_t k = 0;
  int converged = 0, haveSigma = 0;
  BfTsvdSweepState st = {0, 0};
  BfDevScope ds = {0};
  if ((rc = bfDevEnter(&ds, device))) return rc;
  cols = malloc(N * sizeof *cols);
  host = malloc((ld + 2 * N) * sizeof *host);          /* the sums of squares; sigma; the scales of the kept columns */
  perm = malloc(N * sizeof *perm);
  if (!cols || !host || !perm) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory"); goto out; }
  double *sumSq = host, *sigma = host + ld, *scale = sigma + N;
  if ((rc = bfdevMalloc(&dAll, bytes))) goto out;
  double *B = dAll, *part = B + offPart, *Q = B + offQ, *dSumSq = B + offSumSq;
  BfTsvdSweepState *dState = (BfTsvdSweepState *)(B + elems);
  uint32_t *flag = (uint32_t *)(dState + 1);

  /* the noise level: relative to the largest column norm of the block as loaded (between sigma_0 / sqrt(N) and sigma_0) */
  if ((rc = bfdevTsvdLoad(dA, m, n, lda, transposed, B, ld, stream)) || (rc = bfdevTsvdSumSq(B, M, ld, part, dSumSq, stream)) ||
      (rc = bfdevMemcpyD2HAsync(sumSq, dSumSq, (size_t)ld * 8, stream)) || (rc = bfdevSync(stream))) goto out;
  double gmax = 0;
  for (uint64_t j = 0; j < N; ++j) {
    if (!isfinite(sumSq[j])) { rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "truncated SVD: column %llu of the matrix is not finite", (unsigned long long)j); goto out; }
    if (sumSq[j] > gmax) gmax = sumSq[j];
  }
  double const noiseAbs = noise * noise * gmax;
  while (sweeps < maxSweeps) {
    ++sweeps;
    if ((rc = bfdevMemsetAsync(dState, 0, sizeof *dState, stream))) goto out;
    for (uint32_t step = 0; step + 1 < nt; ++step)
      if ((rc = bfdevTsvdStep(B, M, ld, step, thr, noiseAbs, part, Q, flag, dState, stream))) goto out;
    if ((rc = bfdevMemcpyD2HAsync(&st, dState, sizeof st, stream)) || (rc = bfdevSync(stream))) goto out;
    if (!st.rotated) { converged = 1; break; }
  }

  /* the singular values: the column norms, sorted */
  if ((rc = bfdevTsvdSumSq(B, M, ld, part, dSumSq, stream)) || (rc = bfdevMemcpyD2HAsync(sumSq, dSumSq, (size_t)ld * 8, stream)) ||
      (rc = bfdevSync(stream))) goto out;
  for (uint64_t j = 0; j < N; ++j) {
    if (!isfinite(sumSq[j])) { rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "truncated SVD: column %llu is not finite", (unsigned long long)j); goto out; }
    cols[j].norm = sqrt(sumSq[j]); cols[j].index = (uint32_t)j;
  }
  qsort(cols, N, sizeof *cols, tsvdColCmp);
  for (uint64_t j = 0; j < N; ++j) { sigma[j] = cols[j].norm; perm[j] = cols[j].index; }
  k = bfTsvdCount(sigma, N, opt->tol);
  if ((rc = bfdevMemcpyH2DAsync(dSigma, sigma, N * 8, stream)) || (rc = bfdevSync(stream))) goto out;
  haveSigma = 1;
  if (!converged) {
    double off;
    memcpy(&off, &st.offBits, sizeof off);
    rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "truncated SVD: %u sweeps did not converge (largest relative off-diagonal entry %.3g, threshold %.3g); "
                   "dSigma holds the column norms, U and W are not written", sweeps, off, thr);
    goto out;
  }
  if ((dU && k > capU) || (dW && k > capW)) {
    rc = bfhipFail(BFABI_ERROR_OUT_OF_RANGE, "truncated SVD: k = %llu terms do not fit (capU %zu, capW %zu); info->k says how many are needed",
                   (unsigned long long)k, capU, capW);
    goto out;
  }

  /* U and W.  Tall: U = B_k diag(1 / sigma), W = U^T A.  Wide: W = B_k^T, U = A B_k diag(1 / sigma^2) = (A^T)^T (B_k diag(..)) */
  if (k && (dU || dW)) {
    uint32_t const kld = (uint32_t)((k + 15) / 16 * 16);
    uint64_t const crows = bfTsvdContractChunkRows(M, ld), cchunks = (M + crows - 1) / crows;
    uint64_t const nx = transposed ? N : k, ny = transposed ? k : n;
    uint64_t const cpart = cchunks * ((nx + 15) / 16 * 16) * ((ny + 15) / 16 * 16);
    uint64_t const finElems = M * kld + cpart + k;          /* the gathered block, the contraction's partials, the scales; then perm */
    uint64_t const finBytes = finElems * 8 + k * 4;
    if ((rc = bfdevMalloc(&dFin, finBytes))) goto out;
    bytes += finBytes;
    double *Bs = dFin, *cp = Bs + M * kld, *dScale = cp + cpart;
    uint32_t *dPerm = (uint32_t *)(dScale + k);
    for (uint64_t j = 0; j < k; ++j) scale[j] = transposed ? 1 / (sigma[j] * sigma[j]) : 1 / sigma[j];
    if ((rc = bfdevMemcpyH2DAsync(dScale, scale, k * 8, stream)) || (rc = bfdevMemcpyH2DAsync(dPerm, perm, k * 4, stream))) goto out;
    if (!transposed) {
      if ((rc = bfdevTsvdGather(B, M, ld, dPerm, dScale, k, Bs, kld, stream))) goto out;
      if (dU && (rc = bfdevTsvdCopyCols(Bs, M, kld, k, dU, ldu, stream))) goto out;
      if (dW && (rc = bfdevTsvdContract(Bs, kld, k, dA, lda, n, M, crows, cp, dW, ldw, stream))) goto out;
    } else {
      if (dW && (rc = bfdevTsvdGatherT(B, M, ld, dPerm, k, dW, ldw, stream))) goto out;
      if (dU) {
        /* the block is not needed once its columns are gathered: A^T takes its place */
        if ((rc = bfdevTsvdGather(B, M, ld, dPerm, dScale, k, Bs, kld, stream)) || (rc = bfdevTsvdLoad(dA, m, n, lda, 1, B, ld, stream)) ||
            (rc = bfdevTsvdContract(B, ld, N, Bs, kld, k, M, crows, cp, dU, ldu, stream))) goto out;
      }
    }
    if ((rc = bfdevSync(stream))) goto out;
  }
out:
  if (info && (haveSigma || sweeps)) {
    uint32_t const ss = info->structSize;
    memset(info, 0, sizeof *info);
    info->structSize = ss; info->sweeps = sweeps; info->k = k; info->numSingular = N; info->transposed = (uint32_t)transposed;
    memcpy(&info->offNorm, &st.offBits, sizeof info->offNorm);
    info->workspaceBytes = bytes;
    info->seconds = bfNowSeconds() - t0;
  }
  if (dAll || dFin) { bfdevSync(stream); bfdevFree(dFin); bfdevFree(dAll); }
  free(perm); free(host); free(cols);
  bfDevLeave(&ds);
  return rc;
}
