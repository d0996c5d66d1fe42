/* examples/trunc_svd_batch_device.c -- several truncated SVDs in one device call (bfhipTruncSvdBatchDevice), in plain C against
 * include/bfhip.h: what one frontier of the streamer needs.  The driver
 *   1. builds a few small graded matrices A_i = X diag(sigma) Y^T on the host (tall and wide, 20 to 60 rows: the family the
 *      streamer produces most of) and uploads them as one packed buffer,
 *   2. factorizes each with a call of its own (bfhipTruncSvdDevice), then all of them with ONE batched call,
 *   3. checks that the batch gives every problem the single call's k and the single call's sigma, U and W bit for bit, and that
 *      the batch waited (largest sweep count + 3) times where the loop waits that often per problem,
 *   4. prints the figures and exits 0.
 *
 *   gcc -O2 -std=gnu11 -Wall -Werror -Iinclude examples/trunc_svd_batch_device.c -Lbutterfly_amd/csrc -lbfhip -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/butterfly_amd/csrc -Wl,-rpath,/opt/rocm/lib -o /tmp/trunc_svd_batch_device
 *   /tmp/trunc_svd_batch_device [tol = 1e-3]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip.h"

extern int hipMalloc(void **p, size_t bytes);
extern int hipFree(void *p);
extern int hipMemcpy(void *dst, void const *src, size_t bytes, int kind);   /* 1: H2D, 2: D2H */
extern int hipMemset(void *dst, int value, size_t bytes);

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s failed: %s (%s)\n", #call, bfhipErrorString(rc_), bfhipLastErrorMessage()); return 2; } } while (0)
#define HIP(call) do { if (call) { fprintf(stderr, "%s failed\n", #call); return 3; } } while (0)

static void orthonormal(double *Z, size_t rows, size_t cols, unsigned seed) {
  for (size_t i = 0; i < rows * cols; ++i) { seed = seed * 1664525u + 1013904223u; Z[i] = (double)(seed >> 8) / (1u << 24) - 0.5; }
  for (size_t j = 0; j < cols; ++j) {
    for (int pass = 0; pass < 2; ++pass)
      for (size_t k = 0; k < j; ++k) {
        double d = 0;
        for (size_t i = 0; i < rows; ++i) d += Z[i * cols + k] * Z[i * cols + j];
        for (size_t i = 0; i < rows; ++i) Z[i * cols + j] -= d * Z[i * cols + k];
      }
    double nn = 0;
    for (size_t i = 0; i < rows; ++i) nn += Z[i * cols + j] * Z[i * cols + j];
    nn = sqrt(nn);
    for (size_t i = 0; i < rows; ++i) Z[i * cols + j] /= nn;
  }
}

enum { COUNT = 6 };
static size_t const shape[COUNT][2] = { {28, 20}, {27, 20}, {32, 20}, {20, 45}, {60, 36}, {40, 70} };

int main(int argc, char **argv) {
  double const tol = argc > 1 ? strtod(argv[1], NULL) : 1e-3;
  size_t offA[COUNT + 1] = {0}, offS[COUNT + 1] = {0}, offU[COUNT + 1] = {0}, offW[COUNT + 1] = {0};
  for (int i = 0; i < COUNT; ++i) {
    size_t const m = shape[i][0], n = shape[i][1], N = m < n ? m : n;
    offA[i + 1] = offA[i] + m * n; offS[i + 1] = offS[i] + N; offU[i + 1] = offU[i] + m * N; offW[i + 1] = offW[i] + N * n;
  }

  /* ---- 1. the matrices, packed ---- */
  double *A = malloc(offA[COUNT] * 8);
  if (!A) return 1;
  for (int i = 0; i < COUNT; ++i) {
    size_t const m = shape[i][0], n = shape[i][1], N = m < n ? m : n;
    double *X = malloc(m * N * 8), *Y = malloc(n * N * 8);
    if (!X || !Y) return 1;
    orthonormal(X, m, N, 7u + (unsigned)i);
    orthonormal(Y, n, N, 11u + (unsigned)i);
    for (size_t r = 0; r < m; ++r)
      for (size_t c = 0; c < n; ++c) {
        double s = 0;
        for (size_t j = 0; j < N; ++j) s += X[r * N + j] * (j ? pow(10.0, -((double)j - 0.5) / 4.0) : 1.0) * Y[c * N + j];
        A[offA[i] + r * n + c] = s;
      }
    free(X); free(Y);
  }
  void *dA = NULL, *dS[2] = {0}, *dU[2] = {0}, *dW[2] = {0};          /* [0]: the loop of single calls, [1]: the batch */
  HIP(hipMalloc(&dA, offA[COUNT] * 8));
  HIP(hipMemcpy(dA, A, offA[COUNT] * 8, 1));
  for (int w = 0; w < 2; ++w) {
    HIP(hipMalloc(&dS[w], offS[COUNT] * 8)); HIP(hipMalloc(&dU[w], offU[COUNT] * 8)); HIP(hipMalloc(&dW[w], offW[COUNT] * 8));
    HIP(hipMemset(dS[w], 0, offS[COUNT] * 8)); HIP(hipMemset(dU[w], 0, offU[COUNT] * 8)); HIP(hipMemset(dW[w], 0, offW[COUNT] * 8));
  }

  /* ---- 2. one call per problem, then one call for all ---- */
  BfhipTruncSvdOptions opt = { .structSize = sizeof opt, .tol = tol };
  BfhipTruncSvdInfo single[COUNT], infos[COUNT];
  BfhipTruncSvdProblem prob[COUNT];
  int32_t status[COUNT];
  double loopSeconds = 0;
  unsigned loopSyncs = 0, most = 0;
  for (int i = 0; i < COUNT; ++i) {
    size_t const m = shape[i][0], n = shape[i][1], N = m < n ? m : n;
    memset(&single[i], 0, sizeof single[i]); single[i].structSize = sizeof single[i];
    memset(&infos[i], 0, sizeof infos[i]); infos[i].structSize = sizeof infos[i];
    CHECK(bfhipTruncSvdDevice(0, (double *)dA + offA[i], m, n, n, &opt, (double *)dS[0] + offS[i], (double *)dU[0] + offU[i], N, N,
                              (double *)dW[0] + offW[i], n, N, &single[i], NULL));
    loopSeconds += single[i].seconds;
    loopSyncs += single[i].sweeps + 3;
    if (single[i].sweeps > most) most = single[i].sweeps;
    BfhipTruncSvdProblem const p = { (double *)dA + offA[i], m, n, n, (double *)dS[1] + offS[i], (double *)dU[1] + offU[i], N, N,
                                     (double *)dW[1] + offW[i], n, N };
    prob[i] = p;
  }
  BfhipTruncSvdBatchInfo batch = { .structSize = sizeof batch };
  CHECK(bfhipTruncSvdBatchDevice(0, prob, COUNT, &opt, 0, infos, status, &batch, NULL));

  /* ---- 3. the checks ---- */
  double *hs[2], *hu[2], *hw[2];
  for (int w = 0; w < 2; ++w) {
    hs[w] = malloc(offS[COUNT] * 8); hu[w] = malloc(offU[COUNT] * 8); hw[w] = malloc(offW[COUNT] * 8);
    if (!hs[w] || !hu[w] || !hw[w]) return 1;
    HIP(hipMemcpy(hs[w], dS[w], offS[COUNT] * 8, 2)); HIP(hipMemcpy(hu[w], dU[w], offU[COUNT] * 8, 2)); HIP(hipMemcpy(hw[w], dW[w], offW[COUNT] * 8, 2));
  }
  int ok = 1;
  for (int i = 0; i < COUNT; ++i) {
    printf("problem %d: %zu x %zu  k = %llu  %u sweeps  %s\n", i, shape[i][0], shape[i][1], (unsigned long long)infos[i].k, infos[i].sweeps,
           infos[i].transposed ? "transposed" : "as given");
    ok = ok && status[i] == 0 && infos[i].k == single[i].k && infos[i].sweeps == single[i].sweeps && infos[i].k > 0;
  }
  ok = ok && !memcmp(hs[0], hs[1], offS[COUNT] * 8) && !memcmp(hu[0], hu[1], offU[COUNT] * 8) && !memcmp(hw[0], hw[1], offW[COUNT] * 8);
  printf("the loop: %u synchronisations at least, %.3f ms;  the batch: %llu launches, %llu synchronisations, %u group(s), %.3f ms, workspace %.2f MB\n",
         loopSyncs, 1e3 * loopSeconds, (unsigned long long)batch.launches, (unsigned long long)batch.synchronisations, batch.groups, 1e3 * batch.seconds,
         batch.workspaceBytes / 1e6);
  ok = ok && batch.groups == 1 && batch.failed == 0 && batch.maxSweeps == most && batch.synchronisations == most + 3;
  for (int w = 0; w < 2; ++w) { hipFree(dS[w]); hipFree(dU[w]); hipFree(dW[w]); free(hs[w]); free(hu[w]); free(hw[w]); }
  hipFree(dA);
  free(A);
  if (!ok) { fprintf(stderr, "the batch differs from the single calls\n"); return 5; }
  printf("ok\n");
  return 0;
}
