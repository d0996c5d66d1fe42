/* examples/trunc_svd_device.c -- the truncated SVD of a real f64 matrix on the device (bfhipTruncSvdDevice), in plain C against
 * include/bfhip.h: what the streamer's one numerical step needs.  The driver
 *   1. builds a graded m x n matrix A = X diag(sigma) Y^T on the host (sigma_0 = 1, sigma_j = 10^(-(j - 1/2) / 8) below it;
 *      X and Y orthonormal by modified Gram-Schmidt of a fixed fill) and uploads it,
 *   2. asks for the values alone, reads k from the info, sizes U [m x k] and W [k x n] from it and calls again,
 *   3. checks on the host: k against the spectrum it built; ||U^T U - I||_max <= 1e-12 / tol;
 *      ||A - U W||_F <= (the discarded tail) + 1e-12 ||A||_F; the rows of W of norm sigma_j to 1e-12 sigma_0;
 *   4. prints the figures and exits 0.
 *
 *   gcc -O2 -std=gnu11 -Wall -Werror -Iinclude examples/trunc_svd_device.c -Lbutterfly_amd/csrc -lbfhip -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/butterfly_amd/csrc -Wl,-rpath,/opt/rocm/lib -o /tmp/trunc_svd_device
 *   /tmp/trunc_svd_device [m = 300] [n = 96] [tol = 1e-3]          (m < n runs the transposed path)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip.h"

extern int hipMalloc(void **p, size_t bytes);
extern int hipFree(void *p);
extern int hipMemcpy(void *dst, void const *src, size_t bytes, int kind);   /* 1: H2D, 2: D2H */

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

int main(int argc, char **argv) {
  size_t const m = argc > 1 ? strtoull(argv[1], NULL, 10) : 300, n = argc > 2 ? strtoull(argv[2], NULL, 10) : 96;
  double const tol = argc > 3 ? strtod(argv[3], NULL) : 1e-3;
  size_t const N = m < n ? m : n;
  if (!N || N > 2048 || (m > n ? m : n) > 8192) { fprintf(stderr, "usage: %s [m] [n] [tol]   (min(m, n) <= 2048, max(m, n) <= 8192)\n", argv[0]); return 1; }

  /* ---- 1. the matrix ---- */
  double *X = malloc(m * N * 8), *Y = malloc(n * N * 8), *sig = malloc(N * 8), *A = malloc(m * n * 8);
  if (!X || !Y || !sig || !A) return 1;
  orthonormal(X, m, N, 7);
  orthonormal(Y, n, N, 11);
  for (size_t j = 0; j < N; ++j) sig[j] = j ? pow(10.0, -((double)j - 0.5) / 8.0) : 1.0;
  double normA = 0;
  for (size_t i = 0; i < m; ++i)
    for (size_t j = 0; j < n; ++j) {
      double s = 0;
      for (size_t r = 0; r < N; ++r) s += X[i * N + r] * sig[r] * Y[j * N + r];
      A[i * n + j] = s;
      normA += s * s;
    }
  normA = sqrt(normA);
  size_t kWant = 0;
  while (kWant < N && sig[kWant] >= tol * sig[0]) ++kWant;
  void *dA = NULL, *dSigma = NULL, *dU = NULL, *dW = NULL;
  HIP(hipMalloc(&dA, m * n * 8)); HIP(hipMalloc(&dSigma, N * 8));
  HIP(hipMemcpy(dA, A, m * n * 8, 1));

  /* ---- 2. values first, then U and W sized from k ---- */
  BfhipTruncSvdOptions opt = { .structSize = sizeof opt, .tol = tol };
  BfhipTruncSvdInfo info = { .structSize = sizeof info };
  CHECK(bfhipTruncSvdDevice(0, dA, m, n, n, &opt, dSigma, NULL, 0, 0, NULL, 0, 0, &info, NULL));
  size_t const k = info.k;
  printf("A %zu x %zu, tol %g: k = %zu (built: %zu), %u sweeps, %s orientation, off-diagonal %.2e, %.2f ms, workspace %.2f MB\n", m, n, tol, k, kWant,
         info.sweeps, info.transposed ? "transposed" : "given", info.offNorm, 1e3 * info.seconds, info.workspaceBytes / 1e6);
  if (k != kWant) { fprintf(stderr, "k differs from the spectrum the matrix was built with\n"); return 4; }
  HIP(hipMalloc(&dU, m * k * 8)); HIP(hipMalloc(&dW, k * n * 8));
  CHECK(bfhipTruncSvdDevice(0, dA, m, n, n, &opt, dSigma, dU, k, k, dW, n, k, &info, NULL));

  /* ---- 3. the checks ---- */
  double *sigma = malloc(N * 8), *U = malloc(m * k * 8), *W = malloc(k * n * 8);
  if (!sigma || !U || !W) return 1;
  HIP(hipMemcpy(sigma, dSigma, N * 8, 2)); HIP(hipMemcpy(U, dU, m * k * 8, 2)); HIP(hipMemcpy(W, dW, k * n * 8, 2));
  double eSigma = 0, eOrth = 0, eRows = 0, eRec = 0, tail = 0;
  for (size_t j = 0; j < N; ++j) eSigma = fmax(eSigma, fabs(sigma[j] - sig[j]) / sig[0]);
  for (size_t a = 0; a < k; ++a)
    for (size_t b = 0; b < k; ++b) {
      double d = 0;
      for (size_t i = 0; i < m; ++i) d += U[i * k + a] * U[i * k + b];
      eOrth = fmax(eOrth, fabs(d - (a == b)));
    }
  for (size_t r = 0; r < k; ++r) {
    double s = 0;
    for (size_t j = 0; j < n; ++j) s += W[r * n + j] * W[r * n + j];
    eRows = fmax(eRows, fabs(sqrt(s) - sig[r]) / sig[0]);
  }
  for (size_t i = 0; i < m; ++i)
    for (size_t j = 0; j < n; ++j) {
      double s = A[i * n + j];
      for (size_t r = 0; r < k; ++r) s -= U[i * k + r] * W[r * n + j];
      eRec += s * s;
    }
  eRec = sqrt(eRec);
  for (size_t j = k; j < N; ++j) tail += sig[j] * sig[j];
  tail = sqrt(tail);
  printf("sigma %.2e (<= 1e-12)   U^T U - I %.2e (<= %.0e)   rows of W %.2e (<= 1e-12)   A - U W %.6e (<= tail %.6e + %.1e)\n", eSigma, eOrth, 1e-12 / tol,
         eRows, eRec, tail, 1e-12 * normA);
  int const ok = eSigma <= 1e-12 && eOrth <= 1e-12 / tol && eRows <= 1e-12 && eRec <= tail + 1e-12 * normA;
  hipFree(dA); hipFree(dSigma); hipFree(dU); hipFree(dW);
  free(X); free(Y); free(sig); free(A); free(sigma); free(U); free(W);
  if (!ok) { fprintf(stderr, "a bound is not met\n"); return 5; }
  printf("ok\n");
  return 0;
}
