/* The host eigen-routine of the device eigensolver alone (bfEigsSymEig, butterfly_amd/csrc/bfhip_eigs.c: Householder
 * tridiagonalisation + implicit QL), on a designed 130 x 130 spectrum with a triple eigenvalue, a double one, a zero and a
 * cluster 1e-9 wide.  Built by tests/test_lbo_eigs_cpu.py with -fsanitize=address,undefined together with bfhip_eigs.c and
 * run as a program of its own.  A = Z diag(lam) Z^T with Z a product of three Householder reflections, so ||A||_F and the
 * spectrum are known; checked:
 *     ||A Q - Q Theta||_F <= C p 2^-52 ||A||_F,   ||Q^T Q - I||_F <= C p 2^-52,   |theta_j - lam_j| <= C p 2^-52 ||A||_2,
 * with C = 8: tred2 / tql2 are backward stable with a constant that grows slowly with p (Wilkinson), the construction of A
 * itself costs a few p 2^-53 ||A||.  A second run embeds the matrix in a wider array (lda = 144) whose padding must come back
 * untouched.  The rest of bfhip_eigs.c needs the device layer: stand-ins that abort are below. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int bfEigsSymEig(size_t p, double *A, size_t lda, double *theta, double *work);

#define STUB(name) int name() { fprintf(stderr, "device layer reached: %s\n", #name); abort(); }
void bfdevFree(void *p) { if (p) abort(); }
int bfhipFail(int code, char const *fmt, ...) { (void)fmt; return code; }
STUB(bfdevMalloc) STUB(bfdevSync) STUB(bfdevSetDevice) STUB(bfdevGetDevice) STUB(bfdevMemcpyH2DAsync) STUB(bfdevMemcpyD2HAsync)
STUB(bfdevMemsetAsync) STUB(bfdevMemcpy2DAsync) STUB(bfdevFillNormal) STUB(bfdevEigsChunkRows) STUB(bfdevEigsStep) STUB(bfdevEigsGram)
STUB(bfdevEigsRotate) STUB(bfdevEigsResidual) STUB(bfdevEigsStore)

enum { P = 130, LDA = 144 };
#define C_BOUND 8.0

static double frob(double const *M, size_t rows, size_t cols, size_t ld) {
  double s = 0;
  for (size_t i = 0; i < rows; ++i)
    for (size_t j = 0; j < cols; ++j) s += M[i * ld + j] * M[i * ld + j];
  return sqrt(s);
}

static int cmpDouble(void const *a, void const *b) {
  double const x = *(double const *)a, y = *(double const *)b;
  return x < y ? -1 : x > y;
}

int main(void) {
  static double lam[P], Z[P * P], A[P * P], Q[P * LDA], theta[P], work[2 * P], v[P];
  /* the designed spectrum: spread over [-3, 40], then the special values */
  for (int j = 0; j < P; ++j) lam[j] = -3.0 + 43.0 * (double)((j * 37) % P) / P + 0.01 * sin(1.7 * j);
  lam[5] = lam[50] = lam[100] = 1.5;                   /* triple */
  lam[7] = lam[90] = 22.25;                            /* double */
  lam[11] = 0.0;
  lam[20] = 9.0; lam[21] = 9.0 + 1e-9; lam[22] = 9.0 - 1e-9;       /* a tight cluster */
  /* Z = H3 H2 H1, H = I - 2 v v^T / (v^T v) */
  memset(Z, 0, sizeof Z);
  for (int i = 0; i < P; ++i) Z[i * P + i] = 1;
  for (int h = 0; h < 3; ++h) {
    double vv = 0;
    for (int i = 0; i < P; ++i) { v[i] = cos(0.37 * (h + 1) * i + h) + 0.3 * ((i * (7 + 2 * h)) % 11) / 11.0; vv += v[i] * v[i]; }
    for (int j = 0; j < P; ++j) {
      double dot = 0;
      for (int i = 0; i < P; ++i) dot += v[i] * Z[i * P + j];
      for (int i = 0; i < P; ++i) Z[i * P + j] -= 2 * v[i] * dot / vv;
    }
  }
  for (int i = 0; i < P; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0;
      for (int k = 0; k < P; ++k) s += Z[i * P + k] * lam[k] * Z[j * P + k];
      A[i * P + j] = A[j * P + i] = s;
    }
  double const normA = frob(A, P, P, P), eps = ldexp(1.0, -52);
  double top = 0;
  for (int j = 0; j < P; ++j) top = fmax(top, fabs(lam[j]));
  qsort(lam, P, sizeof *lam, cmpDouble);

  int failures = 0;
  for (int run = 0; run < 2; ++run) {
    size_t const ld = run ? LDA : P;
    for (size_t i = 0; i < (size_t)P * LDA; ++i) Q[i] = -77.0;
    for (int i = 0; i < P; ++i) memcpy(Q + i * ld, A + i * P, P * sizeof(double));
    if (bfEigsSymEig(P, Q, ld, theta, work)) { printf("run %d: QL did not converge\n", run); return 1; }
    double res = 0, orth = 0, val = 0;
    for (int j = 0; j < P; ++j) {
      if (j && theta[j] < theta[j - 1]) { printf("run %d: theta not ascending at %d\n", run, j); ++failures; }
      val = fmax(val, fabs(theta[j] - lam[j]));
      for (int i = 0; i < P; ++i) {
        double s = 0;
        for (int k = 0; k < P; ++k) s += A[i * P + k] * Q[k * ld + j];
        s -= Q[i * ld + j] * theta[j];
        res += s * s;
      }
      for (int i = 0; i < P; ++i) {
        double s = 0;
        for (int k = 0; k < P; ++k) s += Q[k * ld + i] * Q[k * ld + j];
        s -= i == j;
        orth += s * s;
      }
    }
    res = sqrt(res); orth = sqrt(orth);
    double const bound = C_BOUND * P * eps;
    printf("run %d (lda %zu): ||AQ - Q Theta||_F / ||A||_F = %.3e, ||Q^T Q - I||_F = %.3e, max |theta - lam| / ||A||_2 = %.3e (bound %.3e)\n",
           run, ld, res / normA, orth, val / top, bound);
    if (!(res <= bound * normA) || !(orth <= bound) || !(val <= bound * top)) ++failures;
    if (run)
      for (int i = 0; i < P; ++i)
        for (size_t j = P; j < ld; ++j)
          if (Q[i * ld + j] != -77.0) { printf("padding written at (%d, %zu)\n", i, j); ++failures; i = P; break; }
  }
  if (failures) { printf("FAILED\n"); return 1; }
  printf("ok\n");
  return 0;
}
