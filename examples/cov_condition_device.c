/* examples/cov_condition_device.c -- conditioning the field of examples/cov_sampling_device.c on point observations, in
 * plain C against include/bfhip*.h: no Python, no reference library.
 *
 * The operand is a synthetic real operator made from a descriptor: the fac_streamer structure of the N x J
 * Laplace-Beltrami eigenvector matrix of the unit sphere (bfhipStreamerLayoutCreate), values generated in HBM, fp64,
 * compiled with its adjoint plan.  The driver
 *   1. draws one prior sample z0 = P Phi GammaLam w0 (bfhipCovDrawDevice) and observes it at 32 points with noise: y,
 *   2. factors the 32 x 32 system once (bfhipCovCondCreate),
 *   3. takes the posterior mean (bfhipCovCondMeanDevice) and the pointwise moments of 256 conditioned draws
 *      (bfhipCovCondMomentsDevice; the draws are not stored),
 *   4. prints the rms misfit at the observed points of an independent prior draw (before conditioning), of the posterior
 *      mean and of the mean of the conditioned draws (after), and exits 0 when the posterior mean's is below the prior draw's.
 *
 *   gcc -O2 -std=gnu11 -Wall -Werror -Iinclude examples/cov_condition_device.c -Lbutterfly_amd/csrc -lbfhip -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/butterfly_amd/csrc -Wl,-rpath,/opt/rocm/lib -o /tmp/cov_condition_device
 *   /tmp/cov_condition_device [numPoints = 4096] [lmax = 15]
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
extern int hipMemset(void *dst, int value, size_t bytes);
extern int hipDeviceSynchronize(void);

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s failed: %s (%s)\n", #call, bfhipErrorString(rc_), bfhipLastErrorMessage()); return 2; } } while (0)
#define HIP(call) do { if (call) { fprintf(stderr, "%s failed\n", #call); return 3; } } while (0)

#define NUM_OBS 32
#define NUM_DRAWS 256

static double misfit(double const *z, uint64_t const *obs, double const *y, double scale) {
  double s = 0;
  for (int a = 0; a < NUM_OBS; ++a) { double const d = z[obs[a]] * scale - y[a]; s += d * d; }
  return sqrt(s / NUM_OBS);
}

int main(int argc, char **argv) {
  uint64_t const numPoints = argc > 1 ? strtoull(argv[1], NULL, 10) : 4096;
  uint64_t const lmax = argc > 2 ? strtoull(argv[2], NULL, 10) : 15;
  uint64_t const seed = 2025, noiseSeed = 2026;
  if (numPoints < 64 || lmax < 1) { fprintf(stderr, "usage: %s [numPoints >= 64] [lmax >= 1]\n", argv[0]); return 1; }

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
  double *gam = malloc(n * sizeof *gam), *z = malloc(2 * m * sizeof *z), *mom = malloc(m * sizeof *mom);
  uint64_t *perm = malloc(m * sizeof *perm);
  if (!gam || !perm || !z || !mom) return 1;
  for (uint64_t j = 0; j < n; ++j) gam[j] = 1.0 / (1.0 + 0.01 * (double)j);
  for (uint64_t i = 0; i < m; ++i) perm[i] = m - 1 - i;
  void *dGam = NULL, *dPerm = NULL, *dZ = NULL, *dY = NULL, *dMean = NULL, *dSum = NULL, *dSumSq = NULL;
  HIP(hipMalloc(&dGam, n * 8)); HIP(hipMalloc(&dPerm, m * 8)); HIP(hipMalloc(&dZ, 2 * m * 8)); HIP(hipMalloc(&dY, NUM_OBS * 8));
  HIP(hipMalloc(&dMean, m * 8)); HIP(hipMalloc(&dSum, m * 8)); HIP(hipMalloc(&dSumSq, m * 8));
  HIP(hipMemcpy(dGam, gam, n * 8, 1)); HIP(hipMemcpy(dPerm, perm, m * 8, 1));

  /* ---- two prior draws: sample 0 is the truth that is observed, sample 1 an independent draw (block layout: z[i * 2 + s]) ---- */
  CHECK(bfhipCovDrawDevice(op, dGam, dPerm, seed, 0, 2, dZ, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(z, dZ, 2 * m * 8, 2));
  double ms = 0;
  for (uint64_t i = 0; i < m; ++i) ms += z[2 * i] * z[2 * i];
  ms /= (double)m;
  uint64_t obs[NUM_OBS];
  double y[NUM_OBS], noiseVar[NUM_OBS], z0[NUM_OBS], z1[NUM_OBS];
  uint64_t at[NUM_OBS];
  for (int a = 0; a < NUM_OBS; ++a) {
    obs[a] = ((2 * (uint64_t)a + 1) * m) / (2 * NUM_OBS);      /* distinct for m >= 64 */
    noiseVar[a] = 1e-4 * ms;
    y[a] = z[2 * obs[a]] + sqrt(noiseVar[a]) * bfhipNormalValue(noiseSeed + 1, (uint64_t)a);
    z0[a] = z[2 * obs[a]]; z1[a] = z[2 * obs[a] + 1]; at[a] = (uint64_t)a;
  }
  HIP(hipMemcpy(dY, y, sizeof y, 1));

  /* ---- factor once, then the mean and the moments of 256 conditioned draws ---- */
  BfhipCovCond *cond = NULL;
  CHECK(bfhipCovCondCreate(op, dGam, dPerm, obs, NUM_OBS, noiseVar, &cond, NULL));
  BfhipCovCondInfo info;
  memset(&info, 0, sizeof info);
  info.structSize = sizeof info;
  CHECK(bfhipCovCondGetInfo(cond, &info));
  printf("%u observations: %llu adjoint panel applies, pivots in [%.3e, %.3e], %.1f KB held; setup %.2f + %.2f + %.2f ms\n", info.numObs,
         (unsigned long long)info.setupApplies, info.minPivot, info.maxPivot, (double)info.factorBytes / 1e3, 1e3 * info.rowsSeconds, 1e3 * info.gramSeconds,
         1e3 * info.factorSeconds);
  CHECK(bfhipCovCondMeanDevice(cond, dY, dMean, NULL, NULL));
  HIP(hipMemset(dSum, 0, m * 8)); HIP(hipMemset(dSumSq, 0, m * 8));
  CHECK(bfhipCovCondMomentsDevice(cond, dY, seed + 7, noiseSeed, 0, NUM_DRAWS, 64, dSum, dSumSq, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(z, dMean, m * 8, 2)); HIP(hipMemcpy(mom, dSum, m * 8, 2));
  double const before = misfit(z1, at, y, 1.0), truth = misfit(z0, at, y, 1.0);
  double const after = misfit(z, obs, y, 1.0), afterDraws = misfit(mom, obs, y, 1.0 / NUM_DRAWS);
  HIP(hipMemcpy(mom, dSumSq, m * 8, 2));
  HIP(hipMemcpy(z + m, dSum, m * 8, 2));
  double varAll = 0, varObs = 0;
  for (uint64_t i = 0; i < m; ++i) { double const mu = z[m + i] / NUM_DRAWS; varAll += mom[i] / NUM_DRAWS - mu * mu; }
  for (int a = 0; a < NUM_OBS; ++a) { double const mu = z[m + obs[a]] / NUM_DRAWS; varObs += mom[obs[a]] / NUM_DRAWS - mu * mu; }
  printf("rms misfit at the %d observed points (noise sd %.3e, field rms %.3e):\n", NUM_OBS, sqrt(noiseVar[0]), sqrt(ms));
  printf("  the observed sample itself        %.6e\n", truth);
  printf("  an independent prior draw         %.6e   (before conditioning)\n", before);
  printf("  the posterior mean                %.6e   (after)\n", after);
  printf("  the mean of %d conditioned draws  %.6e\n", NUM_DRAWS, afterDraws);
  printf("pointwise variance of the conditioned draws: %.6e over all points, %.6e at the observed ones\n", varAll / (double)m, varObs / NUM_OBS);
  bfhipCovCondFree(&cond);
  hipFree(dGam); hipFree(dPerm); hipFree(dZ); hipFree(dY); hipFree(dMean); hipFree(dSum); hipFree(dSumSq);
  free(gam); free(perm); free(z); free(mom);
  bfhipFree(&op);
  if (!(after < before)) { fprintf(stderr, "conditioning did not reduce the misfit at the observed points\n"); return 5; }
  return 0;
}
