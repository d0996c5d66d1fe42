/* The host side of bfhipTruncSvdBatchDevice alone (butterfly_amd/csrc/bfhip_tsvd_batch.c + bfhip_tsvd.c + their headers: the
 * argument checks, the flat pair table, the grouping under a workspace limit, the layout of a group's allocations, the sweep
 * loop with its retiring problems, sort, count, per-problem status and the recovery tables), with every launch replaced by a
 * plain-C stand-in on malloc'd memory.  Built by tests/test_tsvd_batch_cpu.py with -fsanitize=address,undefined and run as a
 * program of its own: an offset or a size that is too small is a heap overflow here.  The single call's stand-ins are those of
 * tsvd_host_check.c (included below with its main renamed); a batched stand-in walks the device tables as the kernels do and
 * calls the single one per problem, so the single call on the same matrix is an exact oracle: the batch must give its bits.
 * Checked: the owner / prefix tables for nt = 2, 4, 10 and 66 in one group; every refusal in the header's order with the
 * problem's index; count == 0; a mixed batch against single calls; the grouping (every problem alone, a problem above the limit,
 * several per group) with identical results and the stated synchronisation count; a problem that never converges and one with
 * too little capacity beside problems that succeed. */
#define main tsvd_single_check_main
#include "tsvd_host_check.c"
#undef main

#include "bfhip_tsvd_batch.h"

char const *bfhipLastErrorMessage(void) { return lastMessage; }

static double const *neverConverges;          /* the dA of the problem whose sweeps the stand-in never lets end */

int bfdevTsvdBatchLoad(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream) {
  for (uint32_t p = 0; p < count; ++p) {
    BfTsvdBatchItem const *it = items + p;
    if (fin && !(fin[p].ops & BF_TSVD_FIN_RELOAD)) continue;
    if (it->M * it->ld > maxElems) return 99;
    bfdevTsvdLoad(it->A, it->m, it->n, it->lda, (int)it->transposed, it->B, it->ld, stream);
  }
  return 0;
}

int bfdevTsvdBatchStep(BfTsvdBatchItem const *items, BfTsvdBatchWords *words, uint32_t const *owner, uint32_t totalPairs, uint32_t step,
                       uint32_t maxChunks, uint64_t maxRows, void *stream) {
  uint32_t last = 0xffffffffu;
  for (uint32_t flat = 0; flat < totalPairs; ++flat) {
    uint32_t const p = owner[flat];
    BfTsvdBatchItem const *it = items + p;
    uint32_t pair, ti, tj;
    if (flat < it->pairBase || flat - it->pairBase >= it->nt / 2) return 98;
    if (!words[p].active || !bfTsvdBatchPair(it->nt, it->pairBase, flat, step, &pair, &ti, &tj)) continue;
    if (p == last) continue;                    /* the single stand-in does all pairs of a problem's step at once */
    last = p;
    if (it->chunks > maxChunks || it->M > maxRows) return 97;
    bfdevTsvdStep(it->B, it->M, it->ld, step, it->thr, words[p].noiseAbs, it->part, it->Q, it->flag, &words[p].state, stream);
    if (it->A == neverConverges) words[p].state.rotated += 1;
  }
  return 0;
}

int bfdevTsvdBatchEndSweep(BfTsvdBatchWords *words, uint32_t count, uint32_t maxSweeps, void *stream) {
  (void)stream;
  for (uint32_t p = 0; p < count; ++p) {
    BfTsvdBatchWords *w = words + p;
    if (!w->active) continue;
    uint32_t const sweeps = ++w->sweeps;
    if (!w->state.rotated || sweeps >= maxSweeps) w->active = 0;
    else { w->state.rotated = 0; w->state.offBits = 0; }
  }
  return 0;
}

int bfdevTsvdBatchSumSq(BfTsvdBatchItem const *items, uint32_t count, uint32_t maxChunks, uint32_t maxLd, void *stream) {
  for (uint32_t p = 0; p < count; ++p) {
    if (items[p].chunks > maxChunks || items[p].ld > maxLd) return 96;
    bfdevTsvdSumSq(items[p].B, items[p].M, items[p].ld, items[p].part, items[p].sumSq, stream);
  }
  return 0;
}

int bfdevTsvdBatchSigma(BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxN, void *stream) {
  (void)stream;
  for (uint32_t p = 0; p < count; ++p)
    if (fin[p].ops & BF_TSVD_FIN_SIGMA) {
      if (fin[p].N > maxN) return 95;
      memcpy(fin[p].dSigma, fin[p].sigma, fin[p].N * 8);
    }
  return 0;
}

int bfdevTsvdBatchGather(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream) {
  for (uint32_t p = 0; p < count; ++p)
    if (fin[p].ops & BF_TSVD_FIN_GATHER) {
      if (items[p].M * fin[p].kld > maxElems) return 94;
      bfdevTsvdGather(items[p].B, items[p].M, items[p].ld, fin[p].perm, fin[p].scale, fin[p].k, fin[p].Bs, fin[p].kld, stream);
    }
  return 0;
}

int bfdevTsvdBatchGatherT(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream) {
  for (uint32_t p = 0; p < count; ++p)
    if (fin[p].ops & BF_TSVD_FIN_GATHERT) {
      if (items[p].M * fin[p].k > maxElems) return 93;
      bfdevTsvdGatherT(items[p].B, items[p].M, items[p].ld, fin[p].perm, fin[p].k, fin[p].dW, fin[p].ldw, stream);
    }
  return 0;
}

int bfdevTsvdBatchCopyCols(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream) {
  for (uint32_t p = 0; p < count; ++p)
    if (fin[p].ops & BF_TSVD_FIN_COPY) {
      if (items[p].M * fin[p].k > maxElems) return 92;
      bfdevTsvdCopyCols(fin[p].Bs, items[p].M, fin[p].kld, fin[p].k, fin[p].dU, fin[p].ldu, stream);
    }
  return 0;
}

int bfdevTsvdBatchContract(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint32_t maxChunks, uint64_t maxTileWork, void *stream) {
  for (uint32_t p = 0; p < count; ++p)
    if (fin[p].ops & BF_TSVD_FIN_CONTRACT) {
      BfTsvdBatchItem const *it = items + p;
      BfTsvdBatchFin const *f = fin + p;
      uint64_t const nx = it->transposed ? f->N : f->k, ny = it->transposed ? f->k : it->n;
      if (f->cchunks > maxChunks || ((nx + 15) / 16) * (((ny + 15) / 16 + 3) / 4) > maxTileWork) return 91;
      if (!it->transposed) bfdevTsvdContract(f->Bs, f->kld, f->k, it->A, it->lda, it->n, it->M, f->crows, f->cpart, f->dW, f->ldw, stream);
      else bfdevTsvdContract(it->B, it->ld, f->N, f->Bs, f->kld, f->k, it->M, f->crows, f->cpart, f->dU, f->ldu, stream);
    }
  return 0;
}

int bfdevTsvdBatchContractStore(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream) {
  (void)items; (void)fin; (void)count; (void)maxElems; (void)stream;          /* the contraction's stand-in has stored already */
  return 0;
}

/* ---- the flat pair table ---- */
static int checkPairTable(void) {
  uint32_t const nts[] = { 2, 4, 10, 66, 4, 2 };
  enum { COUNT = 6 };
  uint32_t first[COUNT + 1], owner[1 + 2 + 5 + 33 + 2 + 1];
  uint64_t const total = bfTsvdBatchPairTable(nts, COUNT, first, owner);
  CHECK(total == 44 && first[COUNT] == 44);
  for (uint32_t i = 0; i < COUNT; ++i)
    for (uint32_t f = first[i]; f < first[i + 1]; ++f) CHECK(owner[f] == i);
  for (uint32_t step = 0; step < 70; ++step) {
    unsigned seen[COUNT][33];
    memset(seen, 0, sizeof seen);
    unsigned char used[COUNT][66];
    memset(used, 0, sizeof used);
    for (uint32_t flat = 0; flat < total; ++flat) {
      uint32_t const i = owner[flat];
      uint32_t pair, a, b;
      if (!bfTsvdBatchPair(nts[i], first[i], flat, step, &pair, &a, &b)) { CHECK(step + 1 >= nts[i]); continue; }
      CHECK(step + 1 < nts[i] && pair < nts[i] / 2 && a < b && b < nts[i] && !used[i][a] && !used[i][b]);
      used[i][a] = used[i][b] = 1;
      ++seen[i][pair];
      uint32_t a1, b1;
      bfTsvdPair(nts[i], step, pair, &a1, &b1);
      CHECK(a == a1 && b == b1);
    }
    for (uint32_t i = 0; i < COUNT; ++i)
      for (uint32_t p = 0; p < 33; ++p) CHECK(seen[i][p] == (step + 1 < nts[i] && p < nts[i] / 2 ? 1u : 0u));
  }
  return 0;
}

/* ---- a mixed batch ---- */
enum { NPROB = 8 };
typedef struct Case { size_t m, n, lda; double *A, *sigma, *U, *W; size_t N; } Case;
static size_t const shapes[NPROB][3] = { {60, 40, 40}, {40, 60, 60}, {48, 40, 56}, {33, 20, 20}, {20, 33, 37}, {136, 130, 130}, {4, 4, 4}, {70, 64, 64} };

static void makeCase(Case *c, size_t m, size_t n, size_t lda, int zero) {
  size_t const N = m < n ? m : n;
  c->m = m; c->n = n; c->lda = lda; c->N = N;
  double *X = malloc(m * N * 8), *Y = malloc(n * N * 8);
  c->A = malloc(m * lda * 8); c->sigma = malloc(N * 8); c->U = malloc(m * N * 8); c->W = malloc(N * n * 8);
  orthonormal(X, m, N, 7u + (unsigned)m);
  orthonormal(Y, n, N, 11u + (unsigned)n);
  for (size_t i = 0; i < m * lda; ++i) c->A[i] = -3.0;
  for (size_t i = 0; i < m; ++i)
    for (size_t j = 0; j < n; ++j) {
      double s = 0;
      for (size_t r = 0; r < N; ++r) s += X[i * N + r] * pow(10.0, -(double)r / 4.0 - (r ? 0.1 : 0.0)) * Y[j * N + r];
      c->A[i * lda + j] = zero ? 0.0 : s;
    }
  free(X); free(Y);
}
static void fillOut(Case *c) {
  for (size_t i = 0; i < c->N; ++i) c->sigma[i] = -1;
  for (size_t i = 0; i < c->m * c->N; ++i) c->U[i] = -7;
  for (size_t i = 0; i < c->N * c->n; ++i) c->W[i] = -7;
}
static void freeCase(Case *c) { free(c->A); free(c->sigma); free(c->U); free(c->W); }
static BfhipTruncSvdProblem problemOf(Case const *c) {
  BfhipTruncSvdProblem p = { c->A, c->m, c->n, c->lda, c->sigma, c->U, c->N, c->N, c->W, c->n, c->N };
  return p;
}
static int sameOut(Case const *a, Case const *b) {
  return !memcmp(a->sigma, b->sigma, a->N * 8) && !memcmp(a->U, b->U, a->m * a->N * 8) && !memcmp(a->W, b->W, a->N * a->n * 8);
}

static int runBatches(void) {
  Case single[NPROB], batch[NPROB];
  BfhipTruncSvdOptions opt = { sizeof opt, 0, 1e-3, 0, 0 };
  BfhipTruncSvdInfo sinfo[NPROB], binfo[NPROB];
  BfhipTruncSvdProblem probs[NPROB];
  int32_t status[NPROB];
  uint64_t bytes[NPROB], all = 0;
  for (int i = 0; i < NPROB; ++i) {
    makeCase(single + i, shapes[i][0], shapes[i][1], shapes[i][2], i == 6);
    makeCase(batch + i, shapes[i][0], shapes[i][1], shapes[i][2], i == 6);
    fillOut(single + i);
    memset(sinfo + i, 0, sizeof sinfo[i]);
    sinfo[i].structSize = sizeof sinfo[i];
    Case *c = single + i;
    CHECK(bfhipTruncSvdDevice(0, c->A, c->m, c->n, c->lda, &opt, c->sigma, c->U, c->N, c->N, c->W, c->n, c->N, sinfo + i, NULL) == 0);
    probs[i] = problemOf(batch + i);
    bytes[i] = bfTsvdBatchProblemBytes(c->m, c->n, 1);
    all += bytes[i];
  }
  CHECK(sinfo[6].k == 0 && sinfo[0].k == 12 && sinfo[5].k == 12);
  /* limits: everything in one group; every problem alone; the largest problem above the limit while the small ones share groups */
  uint64_t const limits[] = { 0, 1, bytes[5] - 1 };
  for (int l = 0; l < 3; ++l) {
    uint32_t groups = 0, wantSyncs = 0;
    for (int i = 0; i < NPROB;) {          /* the grouping rule restated, with the synchronisations it implies */
      uint64_t sum = 0;
      uint32_t most = 0;
      int e = i;
      while (e < NPROB && (e == i || sum + bytes[e] <= (limits[l] ? limits[l] : (1ull << 30)))) { sum += bytes[e]; if (sinfo[e].sweeps > most) most = sinfo[e].sweeps; ++e; }
      ++groups; wantSyncs += most + 3; i = e;
    }
    for (int i = 0; i < NPROB; ++i) { fillOut(batch + i); memset(binfo + i, 0, sizeof binfo[i]); binfo[i].structSize = sizeof binfo[i]; status[i] = -1; }
    BfhipTruncSvdBatchInfo bi = { .structSize = sizeof bi };
    CHECK(bfhipTruncSvdBatchDevice(0, probs, NPROB, &opt, limits[l], binfo, status, &bi, NULL) == 0);
    CHECK(bi.groups == groups && bi.synchronisations == wantSyncs && bi.failed == 0 && bi.launches > 0 && bi.workspaceBytes > 0);
    if (l == 0) CHECK(groups == 1 && bi.workspaceBytes <= all);
    if (l == 1) CHECK(groups == NPROB);
    if (l == 2) CHECK(groups > 2 && groups < NPROB);
    uint32_t most = 0;
    for (int i = 0; i < NPROB; ++i) {
      CHECK(status[i] == 0 && sameOut(single + i, batch + i));
      CHECK(binfo[i].k == sinfo[i].k && binfo[i].sweeps == sinfo[i].sweeps && binfo[i].numSingular == sinfo[i].numSingular &&
            binfo[i].transposed == sinfo[i].transposed && binfo[i].offNorm == sinfo[i].offNorm && binfo[i].seconds == 0 && binfo[i].workspaceBytes == 0);
      if (sinfo[i].sweeps > most) most = sinfo[i].sweeps;
    }
    CHECK(bi.maxSweeps == most);
  }
  /* without infos, status and batch; values only for one problem */
  for (int i = 0; i < NPROB; ++i) fillOut(batch + i);
  probs[3].dU = NULL; probs[3].dW = NULL; probs[3].capU = probs[3].capW = 0;
  CHECK(bfhipTruncSvdBatchDevice(0, probs, NPROB, &opt, 0, NULL, NULL, NULL, NULL) == 0);
  for (int i = 0; i < NPROB; ++i)
    if (i != 3) CHECK(sameOut(single + i, batch + i));
  CHECK(!memcmp(single[3].sigma, batch[3].sigma, single[3].N * 8) && batch[3].U[0] == -7 && batch[3].W[0] == -7);
  probs[3] = problemOf(batch + 3);

  /* failures stay local: problem 4 never converges, problem 1 has room for k - 1 columns of U */
  neverConverges = batch[4].A;
  probs[1].capU = sinfo[1].k - 1;
  uint32_t cap = 0;                              /* the others converge within it: their sweep counts are the single calls' */
  for (int i = 0; i < NPROB; ++i) cap = sinfo[i].sweeps > cap ? sinfo[i].sweeps : cap;
  opt.maxSweeps = cap;
  for (int i = 0; i < NPROB; ++i) { fillOut(batch + i); memset(binfo + i, 0, sizeof binfo[i]); binfo[i].structSize = sizeof binfo[i]; status[i] = -1; }
  BfhipTruncSvdBatchInfo bi = { .structSize = sizeof bi };
  int rc = bfhipTruncSvdBatchDevice(0, probs, NPROB, &opt, 0, binfo, status, &bi, NULL);
  CHECK(rc == 5 && strstr(lastMessage, "problem 1:") && strstr(lastMessage, "do not fit"));
  CHECK(bi.failed == 2 && bi.maxSweeps == cap && bi.synchronisations == cap + 3);
  for (int i = 0; i < NPROB; ++i) {
    if (i == 1) { CHECK(status[i] == 5 && binfo[i].k == sinfo[i].k && batch[i].sigma[0] == single[i].sigma[0]); }
    else if (i == 4) { CHECK(status[i] == 2 && binfo[i].sweeps == cap && batch[i].sigma[0] > 0); }
    else { CHECK(status[i] == 0 && sameOut(single + i, batch + i)); continue; }
    for (size_t e = 0; e < batch[i].m * batch[i].N; ++e) CHECK(batch[i].U[e] == -7);
    for (size_t e = 0; e < batch[i].N * batch[i].n; ++e) CHECK(batch[i].W[e] == -7);
  }
  /* the lowest index decides the return code: with the capacity restored it is the non-convergence of problem 4 */
  probs[1] = problemOf(batch + 1);
  rc = bfhipTruncSvdBatchDevice(0, probs, NPROB, &opt, 1, binfo, status, &bi, NULL);
  CHECK(rc == 2 && strstr(lastMessage, "problem 4:") && strstr(lastMessage, "did not converge") && bi.failed == 1 && bi.groups == NPROB);
  neverConverges = NULL;
  opt.maxSweeps = 0;
  /* a non-finite matrix: its problem is refused at the load, the others are done */
  batch[2].A[5] = NAN;
  for (int i = 0; i < NPROB; ++i) { fillOut(batch + i); binfo[i].sweeps = 77; }
  rc = bfhipTruncSvdBatchDevice(0, probs, NPROB, &opt, 0, binfo, status, &bi, NULL);
  CHECK(rc == 1 && strstr(lastMessage, "problem 2:") && strstr(lastMessage, "not finite") && status[2] == 1 && binfo[2].sweeps == 77 && batch[2].sigma[0] == -1);
  for (int i = 0; i < NPROB; ++i)
    if (i != 2) CHECK(status[i] == 0 && sameOut(single + i, batch + i));
  for (int i = 0; i < NPROB; ++i) { freeCase(single + i); freeCase(batch + i); }
  return 0;
}

static int checkRefusals(void) {
  double a[16] = {0}, s[4], s2[4];
  BfhipTruncSvdOptions opt = { sizeof opt, 0, 1e-3, 0, 0 };
  BfhipTruncSvdInfo infos[2] = { { .structSize = sizeof infos[0] }, { .structSize = sizeof infos[0] } };
  BfhipTruncSvdBatchInfo bi = { .structSize = sizeof bi };
  BfhipTruncSvdProblem good = { a, 4, 4, 4, s, NULL, 0, 0, NULL, 0, 0 }, p[2];
  p[0] = good; p[1] = good; p[1].dSigma = s2;
  CHECK(bfhipTruncSvdBatchDevice(0, p, 2, NULL, 0, infos, NULL, &bi, NULL) == 1);
  CHECK(bfhipTruncSvdBatchDevice(0, NULL, 2, &opt, 0, infos, NULL, &bi, NULL) == 1);
  opt.structSize = 8;
  CHECK(bfhipTruncSvdBatchDevice(0, p, 2, &opt, 0, infos, NULL, &bi, NULL) == 1 && strstr(lastMessage, "BfhipTruncSvdOptions"));
  opt.structSize = sizeof opt;
  bi.structSize = 4;
  CHECK(bfhipTruncSvdBatchDevice(0, p, 2, &opt, 0, infos, NULL, &bi, NULL) == 1 && strstr(lastMessage, "BfhipTruncSvdBatchInfo"));
  bi.structSize = sizeof bi;
  CHECK(bfhipTruncSvdBatchDevice(0, p, (1u << 20) + 1, &opt, 0, NULL, NULL, &bi, NULL) == 1 && strstr(lastMessage, "2^20"));
  /* per problem, the single call's refusals in its order, the second problem being the bad one */
#define REFUSED(word) (bfhipTruncSvdBatchDevice(0, p, 2, &opt, 0, infos, NULL, &bi, NULL) == 1 && strstr(lastMessage, "problem 1: ") && strstr(lastMessage, word))
  p[1].dA = NULL; CHECK(REFUSED("NULL")); p[1] = good;
  p[1].dSigma = NULL; CHECK(REFUSED("NULL")); p[1] = good;
  infos[1].structSize = 3; CHECK(REFUSED("BfhipTruncSvdInfo")); infos[1].structSize = sizeof infos[1];
  double const badTol[] = { 0.0, -1.0, 1.0, 2.0, NAN };
  for (int i = 0; i < 5; ++i) {
    opt.tol = badTol[i];
    CHECK(bfhipTruncSvdBatchDevice(0, p, 2, &opt, 0, infos, NULL, &bi, NULL) == 1 && strstr(lastMessage, "problem 0: ") && strstr(lastMessage, "tol"));
  }
  opt.tol = 1e-3;
  opt.flags = 1; CHECK(bfhipTruncSvdBatchDevice(0, p, 2, &opt, 0, infos, NULL, &bi, NULL) == 1 && strstr(lastMessage, "flags")); opt.flags = 0;
  p[1].m = 0; CHECK(REFUSED("min(m, n) is 0")); p[1] = good;
  p[1].n = 0; p[1].lda = 0; CHECK(REFUSED("min(m, n) is 0")); p[1] = good;
  p[1].m = p[1].n = p[1].lda = 16385; CHECK(REFUSED("16384")); p[1] = good;
  p[1].m = (1ull << 32) + 1; CHECK(REFUSED("2^32")); p[1] = good;
  p[1].lda = 3; CHECK(REFUSED("lda")); p[1] = good;
  p[1].dU = a; p[1].ldu = 2; p[1].capU = 4; CHECK(REFUSED("ldu")); p[1] = good;
  p[1].dW = a; p[1].ldw = 3; p[1].capW = 4; CHECK(REFUSED("ldw")); p[1] = good;
#undef REFUSED
  /* count == 0: nothing to do, with or without an array */
  CHECK(bfhipTruncSvdBatchDevice(0, NULL, 0, &opt, 0, NULL, NULL, &bi, NULL) == 0 && bi.groups == 0 && bi.launches == 0 && bi.synchronisations == 0);
  CHECK(bfhipTruncSvdBatchDevice(0, p, 0, &opt, 0, NULL, NULL, NULL, NULL) == 0);
  return 0;
}

int main(void) {
  if (checkPairTable() || checkRefusals() || runBatches()) return 1;
  printf("ok\n");
  return 0;
}
