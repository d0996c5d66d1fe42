/* bfhip_tsvd_batch.c -- many truncated SVDs in one call (bfhipTruncSvdBatchDevice, include/bfhip.h): the
 * host driver.  The algorithm, the geometry, the argument checks, the comparator and the count rule are the single call's
 * (bfhip_tsvd.c, bfhip_tsvd.h); what is new is that every launch covers all problems of a group and that the host waits once
 * per sweep of the group instead of once per sweep of every problem.  Per group: one allocation and one table upload; load and
 * sums of squares; ONE read-back of all sums (the noise levels are the host's, noise * noise * gmax as in the single call) and
 * one upload of the per-problem words; sweeps of max(nt) - 1 steps of three launches plus the end-of-sweep kernel, the words read
 * back in one copy; the final sums in one copy; sort and count per problem on the host; one allocation and one upload for the
 * recovery; the recovery's launches; one wait.  Synchronisations of a group: its largest sweep count + 3.
 * The kernels are bfhip_tsvd.hip's, the tables bfhip_tsvd_batch.h's. */
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip_internal.h"
#include "../../include/bfhip.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_tsvd_batch.h"

#define TSVD_BATCH_MAX_COUNT (1u << 20)

/* bfhip_tsvd.c; its types are bfhip.h's, so it is declared here and not in bfhip_tsvd.h */
int bfTsvdCheckArguments(double const *dA, size_t m, size_t n, size_t lda, BfhipTruncSvdOptions const *opt, double const *dSigma, double const *dU, size_t ldu,
                         size_t capU, double const *dW, size_t ldw, size_t capW, BfhipTruncSvdInfo const *info);

/* the geometry of one problem, host side */
typedef struct TsvdGeom {
  uint64_t M, N, offPart, offQ, elems;   /* elems: doubles of B, the partials and Q (the sums of squares are packed per group) */
  uint32_t ld, nt, chunks;
  int transposed;
} TsvdGeom;

static void tsvdGeom(BfhipTruncSvdProblem const *p, TsvdGeom *g) {
  g->transposed = p->m < p->n;
  g->M = g->transposed ? p->n : p->m;
  g->N = g->transposed ? p->m : p->n;
  g->ld = bfTsvdLd(g->N);
  g->nt = g->ld / BF_TSVD_TILE;
  uint64_t const rows = bfTsvdChunkRows(g->M, g->ld);
  g->chunks = (uint32_t)((g->M + rows - 1) / rows);
  uint64_t offSumSq;
  bfTsvdWorkspaceElems(g->M, g->ld, &g->offPart, &g->offQ, &offSumSq);
  g->elems = offSumSq;
}

/* the recovery's sizes for k kept terms: the gathered block and the contraction's partials, in doubles */
static void tsvdFinElems(BfhipTruncSvdProblem const *p, TsvdGeom const *g, uint64_t k, uint32_t *kld, uint64_t *crows, uint64_t *cchunks, uint64_t *gathered,
                         uint64_t *cpart) {
  *kld = (uint32_t)((k + 15) / 16 * 16);
  *crows = bfTsvdContractChunkRows(g->M, g->ld);
  *cchunks = (g->M + *crows - 1) / *crows;
  uint64_t const nx = g->transposed ? g->N : k, ny = g->transposed ? k : p->n;
  *gathered = g->M * *kld;
  *cpart = *cchunks * ((nx + 15) / 16 * 16) * ((ny + 15) / 16 * 16);
}

uint64_t bfTsvdBatchProblemBytes(uint64_t m, uint64_t n, int wantUW) {
  BfhipTruncSvdProblem p;
  memset(&p, 0, sizeof p);
  p.m = m; p.n = n;
  TsvdGeom g;
  tsvdGeom(&p, &g);
  uint64_t bytes = (g.elems + g.ld) * 8 + (uint64_t)(g.nt / 2) * 8 + sizeof(BfTsvdBatchItem) + sizeof(BfTsvdBatchWords);
  bytes += g.N * 20 + sizeof(BfTsvdBatchFin);          /* sigma, scale, perm */
  if (wantUW) {
    uint32_t kld;
    uint64_t crows, cchunks, gathered, cpart;
    tsvdFinElems(&p, &g, g.N, &kld, &crows, &cchunks, &gathered, &cpart);
    bytes += (gathered + cpart) * 8;
  }
  return bytes;
}

/* the call's running account: what the batch info reports, and the failure of the lowest index */
typedef struct TsvdBatchRun {
  BfhipTruncSvdProblem const *problems;
  BfhipTruncSvdOptions const *opt;
  BfhipTruncSvdInfo *infos;
  int32_t *status;
  void *stream;
  uint32_t maxSweeps;                 /* of the options */
  uint32_t groups, sweepsSeen, failed;
  uint64_t launches, syncs, peakBytes;
  size_t failIndex;
  int failCode;
  char failMessage[400];
} TsvdBatchRun;

static void tsvdBatchFailProblem(TsvdBatchRun *run, size_t i, int code, char const *fmt, ...) {
  ++run->failed;
  if (run->status) run->status[i] = code;
  if (run->failCode && run->failIndex < i) return;
  run->failCode = code;
  run->failIndex = i;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(run->failMessage, sizeof run->failMessage, fmt, ap);
  va_end(ap);
}

static void tsvdBatchFillInfo(TsvdBatchRun *run, size_t i, TsvdGeom const *g, BfTsvdBatchWords const *w, uint64_t k) {
  if (!run->infos) return;
  BfhipTruncSvdInfo *info = run->infos + i;
  uint32_t const ss = info->structSize;
  memset(info, 0, sizeof *info);
  info->structSize = ss; info->sweeps = w->sweeps; info->k = k; info->numSingular = g->N; info->transposed = (uint32_t)g->transposed;
  memcpy(&info->offNorm, &w->state.offBits, sizeof info->offNorm);
}

static uint64_t tsvdAlign(uint64_t bytes) { return (bytes + 255) / 256 * 256; }

/* the problems [first, first + count) as one group */
static int tsvdBatchGroup(TsvdBatchRun *run, size_t first, uint32_t count) {
  BfhipTruncSvdProblem const *prob = run->problems + first;
  void *stream = run->stream;
  int rc = 0;
  TsvdGeom *geom = malloc(count * sizeof *geom);
  uint32_t *nts = malloc(count * sizeof *nts), *pairFirst = malloc(((size_t)count + 1) * sizeof *pairFirst);
  uint64_t *offN = malloc(((size_t)count + 1) * sizeof *offN), *offLd = malloc(((size_t)count + 1) * sizeof *offLd);
  unsigned char *hTable = NULL, *hFin = NULL;
  double *hSumSq = NULL;
  TsvdCol *cols = NULL;
  void *dAll = NULL, *dFin = NULL;
  if (!geom || !nts || !pairFirst || !offN || !offLd) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory"); goto out; }

  /* ---- geometry and the layout of the group's one allocation:
   *      [B, partials, Q per problem][sums of squares, packed][items][owner][words][flags] ---- */
  uint64_t elems = 0, maxN = 0, maxElems = 0;
  uint32_t maxLd = 0;
  offN[0] = offLd[0] = 0;
  for (uint32_t i = 0; i < count; ++i) {
    tsvdGeom(prob + i, geom + i);
    nts[i] = geom[i].nt;
    elems += geom[i].elems;
    offN[i + 1] = offN[i] + geom[i].N;
    offLd[i + 1] = offLd[i] + geom[i].ld;
    if (geom[i].N > maxN) maxN = geom[i].N;
    if (geom[i].ld > maxLd) maxLd = geom[i].ld;
    if (geom[i].M * geom[i].ld > maxElems) maxElems = geom[i].M * geom[i].ld;
  }
  uint64_t const totalPairs = bfTsvdBatchPairTable(nts, count, pairFirst, NULL);
  if (!totalPairs) { rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "batched truncated SVD: a group of more than 2^31 - 1 tile pairs; lower the workspace limit"); goto out; }
  uint64_t const sumLd = offLd[count], sumN = offN[count];
  uint64_t const offItems = (elems + sumLd) * 8, itemsBytes = (uint64_t)count * sizeof(BfTsvdBatchItem);
  uint64_t const offOwner = offItems + itemsBytes, ownerBytes = (totalPairs * 4 + 7) / 8 * 8;
  uint64_t const offWords = offOwner + ownerBytes, wordsBytes = (uint64_t)count * sizeof(BfTsvdBatchWords);
  uint64_t const offFlags = offWords + wordsBytes, bytes = offFlags + totalPairs * 4;
  uint64_t groupBytes = bytes;
  if ((rc = bfdevMalloc(&dAll, bytes))) goto out;
  hTable = malloc(itemsBytes + ownerBytes + wordsBytes);
  hSumSq = malloc((sumLd ? sumLd : 1) * sizeof *hSumSq);
  cols = malloc((maxN ? maxN : 1) * sizeof *cols);
  if (!hTable || !hSumSq || !cols) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory"); goto out; }
  BfTsvdBatchItem *items = (BfTsvdBatchItem *)hTable;
  uint32_t *owner = (uint32_t *)(hTable + itemsBytes);
  BfTsvdBatchWords *words = (BfTsvdBatchWords *)(hTable + itemsBytes + ownerBytes);
  memset(hTable, 0, itemsBytes + ownerBytes + wordsBytes);
  bfTsvdBatchPairTable(nts, count, pairFirst, owner);
  double *dBase = dAll, *dSumSq = dBase + elems;
  BfTsvdBatchItem *dItems = (BfTsvdBatchItem *)((char *)dAll + offItems);
  uint32_t *dOwner = (uint32_t *)((char *)dAll + offOwner), *dFlags = (uint32_t *)((char *)dAll + offFlags);
  BfTsvdBatchWords *dWords = (BfTsvdBatchWords *)((char *)dAll + offWords);
  {
    uint64_t off = 0;
    for (uint32_t i = 0; i < count; ++i) {
      TsvdGeom const *g = geom + i;
      BfTsvdBatchItem *it = items + i;
      it->A = prob[i].dA; it->m = prob[i].m; it->n = prob[i].n; it->lda = prob[i].lda;
      it->B = dBase + off; it->part = it->B + g->offPart; it->Q = it->B + g->offQ; it->sumSq = dSumSq + offLd[i];
      it->flag = dFlags + pairFirst[i];
      it->M = g->M; it->chunkRows = bfTsvdChunkRows(g->M, g->ld);
      it->ld = g->ld; it->nt = g->nt; it->chunks = g->chunks; it->transposed = (uint32_t)g->transposed;
      it->pairBase = pairFirst[i];
      it->thr = bfTsvdThreshold(g->M);
      off += g->elems;
    }
  }
  uint32_t maxChunks = 0;
  for (uint32_t i = 0; i < count; ++i)
    if (geom[i].chunks > maxChunks) maxChunks = geom[i].chunks;

  /* ---- load; the noise levels: relative to the largest column norm of each block as loaded ---- */
  if ((rc = bfdevMemcpyH2DAsync(dItems, hTable, itemsBytes + ownerBytes, stream)) || (rc = bfdevTsvdBatchLoad(dItems, NULL, count, maxElems, stream)) ||
      (rc = bfdevTsvdBatchSumSq(dItems, count, maxChunks, maxLd, stream)) || (rc = bfdevMemcpyD2HAsync(hSumSq, dSumSq, sumLd * 8, stream)) ||
      (rc = bfdevSync(stream))) goto out;
  run->launches += 3;
  ++run->syncs;
  uint32_t active = 0;
  for (uint32_t i = 0; i < count; ++i) {
    double const *sumSq = hSumSq + offLd[i];
    double gmax = 0;
    int finite = 1;
    for (uint64_t j = 0; j < geom[i].N && finite; ++j) {
      if (!isfinite(sumSq[j])) {
        tsvdBatchFailProblem(run, first + i, BFABI_ERROR_INVALID_ARGUMENTS, "problem %zu: truncated SVD: column %llu of the matrix is not finite", first + i,
                             (unsigned long long)j);
        finite = 0;
      } else if (sumSq[j] > gmax) gmax = sumSq[j];
    }
    double const noise = bfTsvdNoise(geom[i].N);
    words[i].noiseAbs = noise * noise * gmax;
    words[i].active = (uint32_t)finite;
    active += (uint32_t)finite;
  }
  if ((rc = bfdevMemcpyH2DAsync(dWords, words, wordsBytes, stream))) goto out;

  /* ---- the sweeps: every step one Gram, one solve and one rotate launch over the pairs of all problems ---- */
  uint32_t groupSweeps = 0;
  while (active) {
    uint32_t maxNt = 0, chunksNow = 0;
    uint64_t rowsNow = 0;
    for (uint32_t i = 0; i < count; ++i)
      if (words[i].active) {
        if (geom[i].nt > maxNt) maxNt = geom[i].nt;
        if (geom[i].chunks > chunksNow) chunksNow = geom[i].chunks;
        if (geom[i].M > rowsNow) rowsNow = geom[i].M;
      }
    for (uint32_t step = 0; step + 1 < maxNt; ++step) {
      if ((rc = bfdevTsvdBatchStep(dItems, dWords, dOwner, (uint32_t)totalPairs, step, chunksNow, rowsNow, stream))) goto out;
      run->launches += 3;
    }
    if ((rc = bfdevTsvdBatchEndSweep(dWords, count, run->maxSweeps, stream)) || (rc = bfdevMemcpyD2HAsync(words, dWords, wordsBytes, stream)) ||
        (rc = bfdevSync(stream))) goto out;
    ++run->launches;
    ++run->syncs;
    ++groupSweeps;
    active = 0;
    for (uint32_t i = 0; i < count; ++i) active += words[i].active ? 1u : 0u;
    if (groupSweeps > run->maxSweeps) { rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "batched truncated SVD: a problem is still active after maxSweeps sweeps"); goto out; }
  }
  if (groupSweeps > run->sweepsSeen) run->sweepsSeen = groupSweeps;

  /* ---- the singular values: the column norms, sorted; the count; what the recovery of each problem needs ---- */
  if ((rc = bfdevTsvdBatchSumSq(dItems, count, maxChunks, maxLd, stream)) || (rc = bfdevMemcpyD2HAsync(hSumSq, dSumSq, sumLd * 8, stream)) ||
      (rc = bfdevSync(stream))) goto out;
  run->launches += 2;
  ++run->syncs;
  /* staging of the one upload: [sigma, packed][scale, packed][fin table][perm, packed] */
  uint64_t const finTableOff = sumN * 16, permOff = finTableOff + (uint64_t)count * sizeof(BfTsvdBatchFin), stageBytes = permOff + sumN * 4;
  hFin = calloc(1, stageBytes ? stageBytes : 1);
  if (!hFin) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory"); goto out; }
  double *hSigma = (double *)hFin, *hScale = hSigma + sumN;
  BfTsvdBatchFin *fin = (BfTsvdBatchFin *)(hFin + finTableOff);
  uint32_t *hPerm = (uint32_t *)(hFin + permOff);
  uint64_t finElems = 0;
  uint32_t anyOps = 0, maxCChunks = 0;
  uint64_t maxGather = 0, maxMk = 0, maxTileWork = 0, maxStore = 0, maxReload = 0;
  for (uint32_t i = 0; i < count; ++i) {
    TsvdGeom const *g = geom + i;
    BfhipTruncSvdProblem const *p = prob + i;
    BfTsvdBatchFin *f = fin + i;
    if (!words[i].sweeps) continue;                      /* refused at the load: nothing is written, as in the single call */
    double const *sumSq = hSumSq + offLd[i];
    double *sigma = hSigma + offN[i], *scale = hScale + offN[i];
    uint32_t *perm = hPerm + offN[i];
    uint64_t bad = g->N;
    for (uint64_t j = 0; j < g->N; ++j) {
      if (!isfinite(sumSq[j])) { bad = j; break; }
      cols[j].norm = sqrt(sumSq[j]); cols[j].index = (uint32_t)j;
    }
    if (bad < g->N) {
      tsvdBatchFailProblem(run, first + i, BFABI_ERROR_RUNTIME_ERROR, "problem %zu: truncated SVD: column %llu is not finite", first + i, (unsigned long long)bad);
      tsvdBatchFillInfo(run, first + i, g, words + i, 0);
      continue;
    }
    qsort(cols, g->N, sizeof *cols, tsvdColCmp);
    for (uint64_t j = 0; j < g->N; ++j) { sigma[j] = cols[j].norm; perm[j] = cols[j].index; }
    uint64_t const k = bfTsvdCount(sigma, g->N, run->opt->tol);
    tsvdBatchFillInfo(run, first + i, g, words + i, k);
    f->dSigma = p->dSigma; f->dU = p->dU; f->dW = p->dW; f->ldu = p->ldu; f->ldw = p->ldw;
    f->k = k; f->N = g->N;
    f->ops = BF_TSVD_FIN_SIGMA;
    if (words[i].state.rotated) {
      double off;
      memcpy(&off, &words[i].state.offBits, sizeof off);
      tsvdBatchFailProblem(run, first + i, BFABI_ERROR_RUNTIME_ERROR, "problem %zu: truncated SVD: %u sweeps did not converge (largest relative off-diagonal "
                           "entry %.3g, threshold %.3g); dSigma holds the column norms, U and W are not written", first + i, words[i].sweeps, off, items[i].thr);
    } else if ((p->dU && k > p->capU) || (p->dW && k > p->capW)) {
      tsvdBatchFailProblem(run, first + i, BFABI_ERROR_OUT_OF_RANGE, "problem %zu: truncated SVD: k = %llu terms do not fit (capU %llu, capW %llu); the "
                           "problem's info.k says how many are needed", first + i, (unsigned long long)k, (unsigned long long)p->capU,
                           (unsigned long long)p->capW);
    } else if (k && (p->dU || p->dW)) {
      /* U and W.  Tall: U = B_k diag(1 / sigma), W = U^T A.  Wide: W = B_k^T, U = A B_k diag(1 / sigma^2) */
      for (uint64_t j = 0; j < k; ++j) scale[j] = g->transposed ? 1 / (sigma[j] * sigma[j]) : 1 / sigma[j];
      uint64_t gathered, cpart;
      tsvdFinElems(p, g, k, &f->kld, &f->crows, &f->cchunks, &gathered, &cpart);
      uint64_t const nx = g->transposed ? g->N : k, ny = g->transposed ? k : p->n;
      uint64_t const tileWork = ((nx + 15) / 16) * (((ny + 15) / 16 + 3) / 4);
      if (!g->transposed) {
        f->ops |= BF_TSVD_FIN_GATHER | (p->dU ? BF_TSVD_FIN_COPY : 0) | (p->dW ? BF_TSVD_FIN_CONTRACT : 0);
      } else {
        f->ops |= (p->dW ? BF_TSVD_FIN_GATHERT : 0) | (p->dU ? BF_TSVD_FIN_GATHER | BF_TSVD_FIN_RELOAD | BF_TSVD_FIN_CONTRACT : 0);
      }
      if (f->ops & BF_TSVD_FIN_GATHER) {
        /* offsets now, pointers once the allocation exists */
        f->Bs = (double *)(uintptr_t)finElems; finElems += gathered;
        f->cpart = (double *)(uintptr_t)finElems; finElems += cpart;
        if (gathered > maxGather) maxGather = gathered;
      }
      if (g->M * k > maxMk) maxMk = g->M * k;
      if (f->ops & BF_TSVD_FIN_CONTRACT) {
        if (f->cchunks > maxCChunks) maxCChunks = (uint32_t)f->cchunks;
        if (tileWork > maxTileWork) maxTileWork = tileWork;
        if (nx * ny > maxStore) maxStore = nx * ny;
      }
      if ((f->ops & BF_TSVD_FIN_RELOAD) && g->M * g->ld > maxReload) maxReload = g->M * g->ld;
    }
    anyOps |= f->ops;
  }
  if (anyOps) {
    /* the recovery's one allocation: [gathered blocks and partials][the staged arrays] */
    uint64_t const stageOff = tsvdAlign(finElems * 8), finBytes = stageOff + stageBytes;
    if ((rc = bfdevMalloc(&dFin, finBytes))) goto out;
    groupBytes += finBytes;
    double *dFinBase = dFin;
    char *dStage = (char *)dFin + stageOff;
    for (uint32_t i = 0; i < count; ++i) {
      BfTsvdBatchFin *f = fin + i;
      if (!f->ops) continue;
      f->sigma = (double const *)dStage + offN[i];
      f->scale = (double const *)dStage + sumN + offN[i];
      f->perm = (uint32_t const *)(dStage + permOff) + offN[i];
      if (f->ops & BF_TSVD_FIN_GATHER) { f->Bs = dFinBase + (uintptr_t)f->Bs; f->cpart = dFinBase + (uintptr_t)f->cpart; }
    }
    BfTsvdBatchFin const *dFinTable = (BfTsvdBatchFin const *)(dStage + finTableOff);
    if ((rc = bfdevMemcpyH2DAsync(dStage, hFin, stageBytes, stream)) || (rc = bfdevTsvdBatchSigma(dFinTable, count, maxN, stream))) goto out;
    ++run->launches;
    if (anyOps & BF_TSVD_FIN_GATHER) { if ((rc = bfdevTsvdBatchGather(dItems, dFinTable, count, maxGather, stream))) goto out; ++run->launches; }
    if (anyOps & BF_TSVD_FIN_GATHERT) { if ((rc = bfdevTsvdBatchGatherT(dItems, dFinTable, count, maxMk, stream))) goto out; ++run->launches; }
    if (anyOps & BF_TSVD_FIN_COPY) { if ((rc = bfdevTsvdBatchCopyCols(dItems, dFinTable, count, maxMk, stream))) goto out; ++run->launches; }
    /* the block is not needed once its columns are gathered: A^T takes its place (the wide case's U) */
    if (anyOps & BF_TSVD_FIN_RELOAD) { if ((rc = bfdevTsvdBatchLoad(dItems, dFinTable, count, maxReload, stream))) goto out; ++run->launches; }
    if (anyOps & BF_TSVD_FIN_CONTRACT) {
      if ((rc = bfdevTsvdBatchContract(dItems, dFinTable, count, maxCChunks, maxTileWork, stream)) ||
          (rc = bfdevTsvdBatchContractStore(dItems, dFinTable, count, maxStore, stream))) goto out;
      run->launches += 2;
    }
  }
  if ((rc = bfdevSync(stream))) goto out;
  ++run->syncs;
  if (groupBytes > run->peakBytes) run->peakBytes = groupBytes;
out:
  if (dAll || dFin) { if (rc) bfdevSync(stream); bfdevFree(dFin); bfdevFree(dAll); }
  free(cols); free(hSumSq); free(hFin); free(hTable); free(offLd); free(offN); free(pairFirst); free(nts); free(geom);
  return rc;
}

int bfhipTruncSvdBatchDevice(int device, BfhipTruncSvdProblem const *problems, size_t count, BfhipTruncSvdOptions const *opt, uint64_t workspaceLimitBytes,
                             BfhipTruncSvdInfo *infos, int32_t *status, BfhipTruncSvdBatchInfo *batch, void *stream) {
  if (!opt || (!problems && count)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (opt->structSize != sizeof *opt) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "structSize is not sizeof(BfhipTruncSvdOptions)");
  if (batch && batch->structSize != sizeof *batch) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "structSize is not sizeof(BfhipTruncSvdBatchInfo)");
  if (count > TSVD_BATCH_MAX_COUNT) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "count is more than 2^20");
  for (size_t i = 0; i < count; ++i) {
    BfhipTruncSvdProblem const *p = problems + i;
    int const rc = bfTsvdCheckArguments(p->dA, p->m, p->n, p->lda, opt, p->dSigma, p->dU, p->ldu, p->capU, p->dW, p->ldw, p->capW, infos ? infos + i : NULL);
    if (rc) {
      char single[320];
      snprintf(single, sizeof single, "%s", bfhipLastErrorMessage());
      return bfhipFail(rc, "problem %zu: %s", i, single);
    }
  }
  double const t0 = bfNowSeconds();
  TsvdBatchRun run;
  memset(&run, 0, sizeof run);
  run.problems = problems; run.opt = opt; run.infos = infos; run.status = status; run.stream = stream;
  run.maxSweeps = opt->maxSweeps ? opt->maxSweeps : 30;
  for (size_t i = 0; status && i < count; ++i) status[i] = 0;
  int rc = 0;
  BfDevScope ds = {0};
  if (count) {
    if ((rc = bfDevEnter(&ds, device))) return rc;
    uint64_t const limit = workspaceLimitBytes ? workspaceLimitBytes : BF_TSVD_BATCH_DEFAULT_LIMIT;
    /* consecutive groups whose summed workspace fits the limit; a problem above it is a group of its own */
    size_t first = 0;
    while (first < count && !rc) {
      uint64_t sum = 0, pairs = 0;
      size_t end = first;
      while (end < count) {
        BfhipTruncSvdProblem const *p = problems + end;
        uint64_t const b = bfTsvdBatchProblemBytes(p->m, p->n, p->dU || p->dW), pr = bfTsvdLd(p->m < p->n ? p->m : p->n) / BF_TSVD_PAIR;
        if (end > first && (sum + b > limit || pairs + pr > (1u << 24))) break;
        sum += b; pairs += pr; ++end;
      }
      ++run.groups;
      rc = tsvdBatchGroup(&run, first, (uint32_t)(end - first));
      first = end;
    }
    bfDevLeave(&ds);
  }
  if (batch) {
    uint32_t const ss = batch->structSize;
    memset(batch, 0, sizeof *batch);
    batch->structSize = ss; batch->groups = run.groups; batch->failed = run.failed;
    batch->launches = run.launches; batch->synchronisations = run.syncs; batch->workspaceBytes = run.peakBytes;
    batch->seconds = bfNowSeconds() - t0;
    batch->maxSweeps = run.sweepsSeen;
  }
  if (rc) return rc;
  if (run.failCode) return bfhipFail(run.failCode, "%s", run.failMessage);
  return 0;
}
