/* examples/cov_likelihood_device.c -- the log marginal likelihood of point observations with its gradients, and exact
 * kriging variances, for the field of examples/cov_condition_device.c, in plain C against include/bfhip*.h: no Python, no
 * reference library.
 *
 * The operand is the synthetic real operator of that driver (the fac_streamer structure of the Laplace-Beltrami
 * eigenvector matrix of the unit sphere, values generated in HBM, fp64, with its adjoint plan).  The driver
 *   1. draws one prior sample and observes it at 32 points with noise: y,
 *   2. factors the 32 x 32 system once (bfhipCovCondCreate),
 *   3. evaluates logLik, d logLik / d log gamma_j for every weight and d logLik / d noiseVar[a] for every observation
 *      (bfhipCovCondLogLikelihoodDevice) -- what a fit of a parametric spectrum gamma(lambda; theta) needs per step,
 *   4. checks them against the homogeneity identity  sum_j g_j / 2 + sum_a h_a noiseVar[a] = (quad - k) / 2  (scaling
 *      every weight by t and every noise variance by t^2 scales K by t^2), within 8e-12 kappa (quad + k) with
 *      kappa <= trace(K) / min noiseVar, the trace taken from the prior variances at the observed points,
 *   5. prints the smallest and largest ratio of posterior to prior variance over 512 points, the observed ones among them
 *      (bfhipCovCondVarianceDevice), and exits 0 when the identity holds and every ratio lies in [0, 1].
 *
 *   gcc -O2 -std=gnu11 -Wall -Werror -Iinclude examples/cov_likelihood_device.c -Lbutterfly_amd/csrc -lbfhip -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/butterfly_amd/csrc -Wl,-rpath,/opt/rocm/lib -o /tmp/cov_likelihood_device
 *   /tmp/cov_likelihood_device [numPoints = 4096] [lmax = 15]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip.h"
#include "bfhip_build.h"

/* the HIP runtime calls the driver makes itself (no HIP headers needed) */
extern int hipMalloc(void **p, size_t bytes);
extern int hipFree(void *p);
extern int hipMemcpy(void *dst, void const *src, size_t bytes, int kind);   /* 1: H2D, 2: D2H */
extern int hipDeviceSynchronize(void);

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s failed: %s (%s)\n", #call, bfhipErrorString(rc_), bfhipLastErrorMessage()); return 2; } } while (0)
#define HIP(call) do { if (call) { fprintf(stderr, "%s failed\n", #call); return 3; } } while (0)

#define NUM_OBS 32
#define NUM_QUERY 512

int main(int argc, char **argv) {
  uint64_t const numPoints = argc > 1 ? strtoull(argv[1], NULL, 10) : 4096;
  uint64_t const lmax = argc > 2 ? strtoull(argv[2], NULL, 10) : 15;
  uint64_t const seed = 2025, noiseSeed = 2026;
  if (numPoints < NUM_QUERY || lmax < 1) { fprintf(stderr, "usage: %s [numPoints >= %d] [lmax >= 1]\n", argv[0], NUM_QUERY); return 1; }

  /* ---- the operand: Fibonacci points on the sphere, eigenfunctions of degree <= lmax fed band by band ---- */
  double *pts = malloc(3 * numPoints * sizeof *pts);
  if (!pts) return 1;
  for (uint64_t i = 0; i < numPoints; ++i) {
    double const x = 1 - 2.0 * ((double)i + 0.5) / (double)numPoints, r = sqrt(1 - x * x), th = M_PI * (sqrt(5.0) - 1) * (double)i;
    pts[3 * i] = x; pts[3 * i + 1] = r * cos(th); pts[3 * i + 2] = r * sin(th);
  }
  uint32_t treeDepth = 0;
  CHECK(bfhipStreamerOctreeDepth(pts, numPoints, &treeDepth));
  uint32_t const colDepth = treeDepth > 3 ? treeDepth - 3 : 0;
  double const wmax = sqrt((double)lmax * ((double)lmax + 1)) * 1.0001;
  uint64_t const numBands = 1ull << colDepth;
  uint64_t *bands = calloc(numBands, sizeof *bands);
  if (!bands) return 1;
  for (uint64_t l = 0;; ++l) {
    double const w = sqrt((double)l * ((double)l + 1));
    if (w >= wmax) break;
    uint64_t j = (uint64_t)(w / (wmax / (double)numBands));
    bands[j < numBands - 1 ? j : numBands - 1] += 2 * l + 1;
  }
  BfhipStreamerSpec spec;
  memset(&spec, 0, sizeof spec);
  spec.structSize = sizeof spec; spec.colDepth = colDepth; spec.wmax = wmax; spec.bandColumns = bands;
  BfhipStreamerLayout *layout = NULL;
  CHECK(bfhipStreamerLayoutCreate(pts, numPoints, &spec, &layout));
  BfhipOptions opts;
  memset(&opts, 0, sizeof opts);
  opts.structSize = sizeof opts; opts.device = -1; opts.flags = BFHIP_FLAG_ADJOINT; opts.seed = seed; opts.maxRhs = 64;
  BfhipOperator *op = NULL;
  CHECK(bfhipCompileDesc(bfhipStreamerLayoutGetDesc(layout), &opts, &op));
  bfhipStreamerLayoutFree(&layout);
  free(bands); free(pts);
  uint64_t const m = bfhipGetNumRows(op), n = bfhipGetNumCols(op);
  printf("operator: %llu rows x %llu columns, fp64, with its adjoint plan\n", (unsigned long long)m, (unsigned long long)n);
  CHECK(bfhipSetRealRhsBlocks(op, 2));
  CHECK(bfhipSetAdjointRhsBlocks(op, 2));

  /* ---- GammaLam (a smooth spectrum) and the row permutation (the reversal) ---- */
  double *gam = malloc(n * sizeof *gam), *z = malloc(m * sizeof *z), *g = malloc(n * sizeof *g);
  uint64_t *perm = malloc(m * sizeof *perm);
  if (!gam || !perm || !z || !g) return 1;
  for (uint64_t j = 0; j < n; ++j) gam[j] = 1.0 / (1.0 + 0.01 * (double)j);
  for (uint64_t i = 0; i < m; ++i) perm[i] = m - 1 - i;
  void *dGam = NULL, *dPerm = NULL, *dZ = NULL, *dY = NULL, *dValue = NULL, *dG = NULL, *dH = NULL, *dPrior = NULL, *dPost = NULL;
  HIP(hipMalloc(&dGam, n * 8)); HIP(hipMalloc(&dPerm, m * 8)); HIP(hipMalloc(&dZ, m * 8)); HIP(hipMalloc(&dY, NUM_OBS * 8));
  HIP(hipMalloc(&dValue, 3 * 8)); HIP(hipMalloc(&dG, n * 8)); HIP(hipMalloc(&dH, NUM_OBS * 8));
  HIP(hipMalloc(&dPrior, NUM_QUERY * 8)); HIP(hipMalloc(&dPost, NUM_QUERY * 8));
  HIP(hipMemcpy(dGam, gam, n * 8, 1)); HIP(hipMemcpy(dPerm, perm, m * 8, 1));

  /* ---- one prior draw, observed with noise ---- */
  CHECK(bfhipCovDrawDevice(op, dGam, dPerm, seed, 0, 1, dZ, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(z, dZ, m * 8, 2));
  double ms = 0;
  for (uint64_t i = 0; i < m; ++i) ms += z[i] * z[i];
  ms /= (double)m;
  uint64_t obs[NUM_OBS], query[NUM_QUERY];
  double y[NUM_OBS], noiseVar[NUM_OBS];
  for (int a = 0; a < NUM_OBS; ++a) {
    obs[a] = ((2 * (uint64_t)a + 1) * m) / (2 * NUM_OBS);
    noiseVar[a] = 1e-2 * ms * (1.0 + 0.5 * (double)(a % 3));
    y[a] = z[obs[a]] + sqrt(noiseVar[a]) * bfhipNormalValue(noiseSeed + 1, (uint64_t)a);
  }
  HIP(hipMemcpy(dY, y, sizeof y, 1));

  /* ---- factor once; the likelihood with both gradients ---- */
  BfhipCovCond *cond = NULL;
  CHECK(bfhipCovCondCreate(op, dGam, dPerm, obs, NUM_OBS, noiseVar, &cond, NULL));
  BfhipCovCondLikOptions lopt;
  memset(&lopt, 0, sizeof lopt);
  lopt.structSize = sizeof lopt;                       /* workspaceBytes 0: the default */
  CHECK(bfhipCovCondLogLikelihoodDevice(cond, dY, dValue, dG, dH, &lopt, NULL));
  HIP(hipDeviceSynchronize());
  double value[3], h[NUM_OBS], prior[NUM_QUERY], post[NUM_QUERY];
  HIP(hipMemcpy(value, dValue, sizeof value, 2)); HIP(hipMemcpy(g, dG, n * 8, 2)); HIP(hipMemcpy(h, dH, sizeof h, 2));
  printf("%d observations: logLik = %.12e  (quad = %.6e, logDet = %.6e)\n", NUM_OBS, value[0], value[1], value[2]);
  double gmax = 0, hmax = 0, lhs = 0;
  for (uint64_t j = 0; j < n; ++j) { lhs += 0.5 * g[j]; if (fabs(g[j]) > gmax) gmax = fabs(g[j]); }
  for (int a = 0; a < NUM_OBS; ++a) { lhs += h[a] * noiseVar[a]; if (fabs(h[a]) > hmax) hmax = fabs(h[a]); }
  printf("gradients: max |d logLik / d log gamma_j| = %.6e over %llu weights, max |d logLik / d noiseVar[a]| = %.6e\n", gmax, (unsigned long long)n, hmax);

  /* ---- kappa <= trace(K) / min noiseVar, the trace from the prior variances at the observed points ---- */
  CHECK(bfhipCovCondVarianceDevice(cond, obs, NUM_OBS, dPrior, NULL, NULL));
  HIP(hipMemcpy(prior, dPrior, NUM_OBS * 8, 2));
  double trace = 0, dmin = noiseVar[0];
  for (int a = 0; a < NUM_OBS; ++a) { trace += prior[a] + noiseVar[a]; if (noiseVar[a] < dmin) dmin = noiseVar[a]; }
  double const kappa = trace / dmin, rhs = 0.5 * (value[1] - NUM_OBS), residual = fabs(lhs - rhs), bound = 8e-12 * kappa * (value[1] + NUM_OBS);
  printf("homogeneity: sum g / 2 + sum h noiseVar = %.12e, (quad - k) / 2 = %.12e: residual %.3e (bound %.3e, kappa <= %.3e)\n", lhs, rhs, residual, bound, kappa);

  /* ---- exact kriging variances at 512 points, the observed ones among them when they fall on the stride ---- */
  for (int t = 0; t < NUM_QUERY; ++t) query[t] = (uint64_t)t * (m / NUM_QUERY);
  CHECK(bfhipCovCondVarianceDevice(cond, query, NUM_QUERY, dPrior, dPost, NULL));
  HIP(hipMemcpy(prior, dPrior, sizeof prior, 2)); HIP(hipMemcpy(post, dPost, sizeof post, 2));
  double lo = INFINITY, hi = -INFINITY;
  for (int t = 0; t < NUM_QUERY; ++t) { double const r = post[t] / prior[t]; if (r < lo) lo = r; if (r > hi) hi = r; }
  printf("posterior / prior variance over %d points: min %.6f, max %.6f\n", NUM_QUERY, lo, hi);

  bfhipCovCondFree(&cond);
  hipFree(dGam); hipFree(dPerm); hipFree(dZ); hipFree(dY); hipFree(dValue); hipFree(dG); hipFree(dH); hipFree(dPrior); hipFree(dPost);
  free(gam); free(perm); free(z); free(g);
  bfhipFree(&op);
  if (!(residual <= bound)) { fprintf(stderr, "the gradients miss the homogeneity identity\n"); return 5; }
  if (!(lo >= -1e-9 && hi <= 1 + 1e-9)) { fprintf(stderr, "a posterior variance lies outside [0, prior]\n"); return 6; }
  return 0;
}
