/* The host side of bfhipTruncSvdDevice alone (butterfly_amd/csrc/bfhip_tsvd.c + bfhip_tsvd.h: argument checks, round-robin
 * schedule, workspace layout, sweep loop, sort, count rule, recovery of U and W), with every launch of bfhip_tsvd.hip replaced
 * by a plain-C stand-in on malloc'd memory.  Built by tests/test_streamer_build_cpu.py with -fsanitize=address,undefined and
 * run as a program of its own: a workspace offset or a size that is too small is a heap overflow here.  The stand-ins honour
 * the launches' contracts (they write the whole of every buffer the kernels may write: all partials, all of Q, every flag),
 * the pair solve being plain Hestenes rotations on the pair's 32 columns -- another algorithm, the same fixed point.
 * Checked: the schedule meets every tile pair exactly once per sweep with disjoint pairs per step; every refusal; a tall, a
 * wide and a strided case against the known spectrum (k, sigma, U^T U, A - U W); capacity; maxSweeps = 1; the all-zero matrix. */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip.h"
#include "bfhip_tsvd.h"

static char lastMessage[512];
int bfhipFail(int code, char const *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(lastMessage, sizeof lastMessage, fmt, ap);
  va_end(ap);
  return code;
}
int bfdevSetDevice(int device) { (void)device; return 0; }
int bfdevGetDevice(int *device) { *device = 0; return 0; }
int bfdevMalloc(void **p, size_t bytes) { *p = malloc(bytes ? bytes : 16); return *p ? 0 : 4; }
void bfdevFree(void *p) { free(p); }
int bfdevSync(void *stream) { (void)stream; return 0; }
int bfdevMemsetAsync(void *dst, int value, size_t bytes, void *stream) { (void)stream; memset(dst, value, bytes); return 0; }
int bfdevMemcpyD2HAsync(void *dst, void const *src, size_t bytes, void *stream) { (void)stream; memcpy(dst, src, bytes); return 0; }
int bfdevMemcpyH2DAsync(void *dst, void const *src, size_t bytes, void *stream) { (void)stream; memcpy(dst, src, bytes); return 0; }

int bfdevTsvdLoad(double const *dA, uint64_t m, uint64_t n, uint64_t lda, int transpose, double *B, uint32_t ld, void *stream) {
  (void)stream;
  uint64_t const M = transpose ? n : m, N = transpose ? m : n;
  for (uint64_t i = 0; i < M; ++i)
    for (uint64_t j = 0; j < ld; ++j) B[i * ld + j] = j < N ? (transpose ? dA[j * lda + i] : dA[i * lda + j]) : 0.0;
  return 0;
}

int bfdevTsvdStep(double *B, uint64_t M, uint32_t ld, uint32_t step, double thr, double noiseAbs, double *part, double *Q, uint32_t *flag,
                  BfTsvdSweepState *state, void *stream) {
  (void)stream;
  uint32_t const nt = ld / BF_TSVD_TILE, pairs = nt / 2;
  uint64_t const rows = bfTsvdChunkRows(M, ld), chunks = (M + rows - 1) / rows;
  memset(part, 0, chunks * pairs * 1024 * sizeof *part);
  memset(Q, 0, (size_t)pairs * 1024 * sizeof *Q);
  for (uint32_t p = 0; p < pairs; ++p) {
    uint32_t ti, tj, col[32];
    bfTsvdPair(nt, step, p, &ti, &tj);
    for (uint32_t c = 0; c < 16; ++c) { col[c] = 16 * ti + c; col[16 + c] = 16 * tj + c; }
    double worst = 0;
    int rotated = 0;
    for (uint32_t a = 0; a < 32; ++a)
      for (uint32_t b = a + 1; b < 32; ++b) {
        double gaa = 0, gbb = 0, gab = 0;
        for (uint64_t r = 0; r < M; ++r) {
          double const x = B[r * ld + col[a]], y = B[r * ld + col[b]];
          gaa += x * x; gbb += y * y; gab += x * y;
        }
        if (!(fmin(gaa, gbb) > noiseAbs)) continue;
        double const rel = fabs(gab) / sqrt(gaa * gbb);
        if (rel > worst) worst = rel;
        if (!(rel > thr)) continue;
        double const tau = (gbb - gaa) / (2 * gab), t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1 + tau * tau));
        double const c = 1 / sqrt(1 + t * t), s = t * c;
        for (uint64_t r = 0; r < M; ++r) {
          double const x = B[r * ld + col[a]], y = B[r * ld + col[b]];
          B[r * ld + col[a]] = c * x - s * y;
          B[r * ld + col[b]] = s * x + c * y;
        }
        rotated = 1;
      }
    flag[p] = (uint32_t)rotated;
    state->rotated += (unsigned long long)rotated;
    unsigned long long bits;
    memcpy(&bits, &worst, sizeof bits);
    if (bits > state->offBits) state->offBits = bits;
  }
  return 0;
}

int bfdevTsvdSumSq(double const *B, uint64_t M, uint32_t ld, double *part, double *out, void *stream) {
  (void)stream;
  uint64_t const rows = bfTsvdChunkRows(M, ld), chunks = (M + rows - 1) / rows;
  memset(part, 0, chunks * ld * sizeof *part);
  for (uint32_t c = 0; c < ld; ++c) {
    double s = 0;
    for (uint64_t r = 0; r < M; ++r) s += B[r * ld + c] * B[r * ld + c];
    out[c] = s;
  }
  return 0;
}

int bfdevTsvdGather(double const *B, uint64_t M, uint32_t ld, uint32_t const *perm, double const *scale, uint64_t k, double *out, uint32_t kld,
                    void *stream) {
  (void)stream;
  for (uint64_t i = 0; i < M; ++i)
    for (uint32_t j = 0; j < kld; ++j) out[i * kld + j] = j < k ? scale[j] * B[i * ld + perm[j]] : 0.0;
  return 0;
}

int bfdevTsvdGatherT(double const *B, uint64_t M, uint32_t ld, uint32_t const *perm, uint64_t k, double *out, uint64_t ldo, void *stream) {
  (void)stream;
  for (uint64_t j = 0; j < k; ++j)
    for (uint64_t c = 0; c < M; ++c) out[j * ldo + c] = B[c * ld + perm[j]];
  return 0;
}

int bfdevTsvdContract(double const *X, uint64_t ldx, uint64_t nx, double const *Y, uint64_t ldy, uint64_t ny, uint64_t M, uint64_t chunkRows,
                      double *part, double *out, uint64_t ldo, void *stream) {
  (void)stream;
  uint64_t const chunks = (M + chunkRows - 1) / chunkRows, px = (nx + 15) / 16 * 16, py = (ny + 15) / 16 * 16;
  memset(part, 0, chunks * px * py * sizeof *part);
  for (uint64_t a = 0; a < nx; ++a)
    for (uint64_t b = 0; b < ny; ++b) {
      double s = 0;
      for (uint64_t r = 0; r < M; ++r) s += X[r * ldx + a] * Y[r * ldy + b];
      out[a * ldo + b] = s;
    }
  return 0;
}

int bfdevTsvdCopyCols(double const *X, uint64_t M, uint32_t ldx, uint64_t k, double *out, uint64_t ldo, void *stream) {
  (void)stream;
  for (uint64_t i = 0; i < M; ++i)
    for (uint64_t j = 0; j < k; ++j) out[i * ldo + j] = X[i * ldx + j];
  return 0;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, lastMessage); return 1; } } while (0)

static int checkSchedule(void) {
  for (uint32_t nt = 2; nt <= 66; nt += 2) {
    unsigned char *met = calloc((size_t)nt * nt, 1);
    for (uint32_t step = 0; step + 1 < nt; ++step) {
      unsigned char used[66] = {0};
      for (uint32_t p = 0; p < nt / 2; ++p) {
        uint32_t a, b;
        bfTsvdPair(nt, step, p, &a, &b);
        CHECK(a < b && b < nt && !used[a] && !used[b]);
        used[a] = used[b] = 1;
        CHECK(!met[a * nt + b]);
        met[a * nt + b] = 1;
      }
    }
    for (uint32_t a = 0; a < nt; ++a)
      for (uint32_t b = a + 1; b < nt; ++b) CHECK(met[a * nt + b]);
    free(met);
  }
  return 0;
}

/* A [m x n in lda] = X diag(sig) Y^T with X, Y made orthonormal by modified Gram-Schmidt of a fixed pseudo-random fill */
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

static int runCase(size_t m, size_t n, size_t lda, double tol, size_t kWant) {
  size_t const N = m < n ? m : n;
  double *X = malloc(m * N * 8), *Y = malloc(n * N * 8), *sig = malloc(N * 8), *A = malloc(m * lda * 8), *keep = malloc(m * lda * 8);
  double *sigma = malloc(N * 8), *U = malloc(m * N * 8), *W = malloc(N * n * 8);
  orthonormal(X, m, N, 7u + (unsigned)m);
  orthonormal(Y, n, N, 11u + (unsigned)n);
  for (size_t j = 0; j < N; ++j) sig[j] = pow(10.0, -(double)j / 4.0 - (j ? 0.1 : 0.0));
  for (size_t i = 0; i < m * lda; ++i) A[i] = -3.0;
  for (size_t i = 0; i < m; ++i)
    for (size_t j = 0; j < n; ++j) {
      double s = 0;
      for (size_t r = 0; r < N; ++r) s += X[i * N + r] * sig[r] * Y[j * N + r];
      A[i * lda + j] = s;
    }
  memcpy(keep, A, m * lda * 8);
  BfhipTruncSvdOptions opt = { sizeof opt, 0, tol, 0, 0 };
  BfhipTruncSvdInfo info = { .structSize = sizeof info };
  int rc = bfhipTruncSvdDevice(0, A, m, n, lda, &opt, sigma, U, N, N, W, n, N, &info, NULL);
  CHECK(rc == 0);
  CHECK(!memcmp(keep, A, m * lda * 8));
  CHECK(info.k == kWant && info.numSingular == N && info.transposed == (uint32_t)(m < n) && info.sweeps >= 1);
  for (size_t j = 0; j < N; ++j) CHECK(fabs(sigma[j] - sig[j]) <= 1e-12);
  size_t const k = info.k;
  for (size_t a = 0; a < k; ++a)
    for (size_t b = 0; b < k; ++b) {
      double d = 0;
      for (size_t i = 0; i < m; ++i) d += U[i * N + a] * U[i * N + b];
      CHECK(fabs(d - (a == b)) <= 1e-12 / tol);
    }
  double err = 0, tail = 0;
  for (size_t i = 0; i < m; ++i)
    for (size_t j = 0; j < n; ++j) {
      double s = A[i * lda + j];
      for (size_t r = 0; r < k; ++r) s -= U[i * N + r] * W[r * n + j];
      err += s * s;
    }
  for (size_t j = k; j < N; ++j) tail += sig[j] * sig[j];
  CHECK(sqrt(err) <= sqrt(tail) + 1e-12);
  /* capacity: one column too few */
  info.k = 0;
  rc = bfhipTruncSvdDevice(0, A, m, n, lda, &opt, sigma, U, N, k - 1, W, n, N, &info, NULL);
  CHECK(rc == 5 && info.k == kWant);
  /* values only */
  rc = bfhipTruncSvdDevice(0, A, m, n, lda, &opt, sigma, NULL, 0, 0, NULL, 0, 0, &info, NULL);
  CHECK(rc == 0 && info.k == kWant);
  /* one sweep is not enough */
  opt.maxSweeps = 1;
  rc = bfhipTruncSvdDevice(0, A, m, n, lda, &opt, sigma, U, N, N, W, n, N, &info, NULL);
  CHECK(rc == 2 && info.sweeps == 1 && info.offNorm > 0);
  free(X); free(Y); free(sig); free(A); free(keep); free(sigma); free(U); free(W);
  return 0;
}

int main(void) {
  if (checkSchedule()) return 1;
  /* refusals, in the header's order; no device (here: no stand-in) is reached */
  double a[16] = {0}, s[4];
  BfhipTruncSvdOptions opt = { sizeof opt, 0, 1e-3, 0, 0 };
  BfhipTruncSvdInfo info = { .structSize = sizeof info };
  CHECK(bfhipTruncSvdDevice(0, NULL, 4, 4, 4, &opt, s, NULL, 0, 0, NULL, 0, 0, &info, NULL) == 1);
  CHECK(bfhipTruncSvdDevice(0, a, 4, 4, 4, NULL, s, NULL, 0, 0, NULL, 0, 0, &info, NULL) == 1);
  CHECK(bfhipTruncSvdDevice(0, a, 4, 4, 4, &opt, NULL, NULL, 0, 0, NULL, 0, 0, &info, NULL) == 1);
  opt.structSize = 8;
  CHECK(bfhipTruncSvdDevice(0, a, 4, 4, 4, &opt, s, NULL, 0, 0, NULL, 0, 0, &info, NULL) == 1);
  opt.structSize = sizeof opt;
  double const badTol[] = { 0.0, -1.0, 1.0, 2.0, NAN };
  for (int i = 0; i < 5; ++i) {
    opt.tol = badTol[i];
    CHECK(bfhipTruncSvdDevice(0, a, 4, 4, 4, &opt, s, NULL, 0, 0, NULL, 0, 0, &info, NULL) == 1 && strstr(lastMessage, "tol"));
  }
  opt.tol = 1e-3;
  opt.flags = 1;
  CHECK(bfhipTruncSvdDevice(0, a, 4, 4, 4, &opt, s, NULL, 0, 0, NULL, 0, 0, &info, NULL) == 1);
  opt.flags = 0;
  CHECK(bfhipTruncSvdDevice(0, a, 0, 4, 4, &opt, s, NULL, 0, 0, NULL, 0, 0, &info, NULL) == 1);
  CHECK(bfhipTruncSvdDevice(0, a, 4, 0, 4, &opt, s, NULL, 0, 0, NULL, 0, 0, &info, NULL) == 1);
  CHECK(bfhipTruncSvdDevice(0, a, 16385, 16385, 16385, &opt, s, NULL, 0, 0, NULL, 0, 0, &info, NULL) == 1 && strstr(lastMessage, "16384"));
  CHECK(bfhipTruncSvdDevice(0, a, 4, 4, 3, &opt, s, NULL, 0, 0, NULL, 0, 0, &info, NULL) == 1 && strstr(lastMessage, "lda"));
  CHECK(bfhipTruncSvdDevice(0, a, 4, 4, 4, &opt, s, a, 2, 4, NULL, 0, 0, &info, NULL) == 1 && strstr(lastMessage, "ldu"));
  CHECK(bfhipTruncSvdDevice(0, a, 4, 4, 4, &opt, s, NULL, 0, 0, a, 3, 4, &info, NULL) == 1 && strstr(lastMessage, "ldw"));
  /* the all-zero matrix: k = 0, nothing of U or W written */
  double u[16], w[16];
  for (int i = 0; i < 16; ++i) u[i] = w[i] = -7;
  CHECK(bfhipTruncSvdDevice(0, a, 4, 4, 4, &opt, s, u, 4, 4, w, 4, 4, &info, NULL) == 0 && info.k == 0 && info.sweeps == 1);
  for (int i = 0; i < 16; ++i) CHECK(u[i] == -7 && w[i] == -7);
  /* sigma_j = 10^(-j / 4 - 0.1 [j > 0]): tol 1e-3 keeps j = 0 .. 11 */
  if (runCase(150, 40, 40, 1e-3, 12) || runCase(40, 150, 150, 1e-3, 12) || runCase(48, 40, 56, 1e-3, 12) || runCase(33, 20, 20, 1e-3, 12) ||
      runCase(20, 33, 37, 1e-3, 12)) return 1;
  printf("ok\n");
  return 0;
}
