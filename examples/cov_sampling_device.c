/* examples/cov_sampling_device.c -- the sampling loop of the reference's covariance example (examples/covariance/lbo_cov.c:
 * draw numSamples samples z = P Phi GammaLam w, one after another, each from fresh normals) batched and resident on the
 * device, in plain C against include/bfhip*.h: no Python, no reference library.
 *
 * The operand is the benchmark's streamed butterfly (bench.py --workload streamer): the fac_streamer structure of the
 * N x J Laplace-Beltrami eigenvector matrix of the unit sphere, laid out by bfhipStreamerLayoutCreate under the rank
 * model, with synthetic values generated in HBM and stored in fp32.  The driver
 *   1. switches the real block kernels on (bfhipSetRealRhsBlocks(op, 2)),
 *   2. draws K samples with bfhipCovDrawDevice, 64 at a time (the normals never exist on the host),
 *   3. accumulates the pointwise sum and sum of squares of the same K samples with bfhipCovMomentsDevice (the samples are
 *      not stored) and checks them against the samples of step 2,
 *   4. prints the time per sample of both next to a loop of bfhipCovSampleDevice over vectors already on the device.
 *
 *   gcc -O2 -std=gnu11 -Wall -Werror -Iinclude examples/cov_sampling_device.c -Lbutterfly_amd/csrc -lbfhip -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/butterfly_amd/csrc -Wl,-rpath,/opt/rocm/lib -o /tmp/cov_sampling_device
 *   /tmp/cov_sampling_device [numPoints = 65536] [lmax = 63] [numSamples = 256]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "bfhip.h"
#include "bfhip_build.h"

/* the five HIP runtime calls the driver makes itself (no HIP headers needed) */
extern int hipMalloc(void **p, size_t bytes);
extern int hipFree(void *p);
extern int hipMemcpy(void *dst, void const *src, size_t bytes, int kind);   /* 1: H2D, 2: D2H */
extern int hipMemset(void *dst, int value, size_t bytes);
extern int hipDeviceSynchronize(void);

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s failed: %s (%s)\n", #call, bfhipErrorString(rc_), bfhipLastErrorMessage()); return 2; } } while (0)
#define HIP(call) do { if (call) { fprintf(stderr, "%s failed\n", #call); return 3; } } while (0)

static double now(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

int main(int argc, char **argv) {
  uint64_t const numPoints = argc > 1 ? strtoull(argv[1], NULL, 10) : 65536;
  uint64_t const lmax = argc > 2 ? strtoull(argv[2], NULL, 10) : 63;
  uint64_t const numSamples = argc > 3 ? strtoull(argv[3], NULL, 10) : 256;
  uint64_t const seed = 2025;
  if (numPoints < 64 || lmax < 1 || numSamples < 1) { fprintf(stderr, "usage: %s [numPoints >= 64] [lmax >= 1] [numSamples >= 1]\n", argv[0]); return 1; }

  /* ---- the operand: Fibonacci points on the sphere, eigenfunctions of degree <= lmax fed band by band -------- */
  double *pts = malloc(3 * numPoints * sizeof *pts);
  if (!pts) return 1;
  for (uint64_t i = 0; i < numPoints; ++i) {
    double const x = 1 - 2.0 * ((double)i + 0.5) / (double)numPoints, r = sqrt(1 - x * x), th = M_PI * (sqrt(5.0) - 1) * (double)i;
    pts[3 * i] = x; pts[3 * i + 1] = r * cos(th); pts[3 * i + 2] = r * sin(th);
  }
  uint32_t treeDepth = 0;
  CHECK(bfhipStreamerOctreeDepth(pts, numPoints, &treeDepth));
  uint32_t const colDepth = treeDepth > 3 ? treeDepth - 3 : 0;          /* lbo_cov.c:97-98 */
  double const wmax = sqrt((double)lmax * ((double)lmax + 1)) * 1.0001;
  uint64_t const numBands = 1ull << colDepth;
  uint64_t *bands = calloc(numBands, sizeof *bands);
  if (!bands) return 1;
  for (uint64_t l = 0;; ++l) {                                        /* degree l: 2l + 1 eigenfunctions at sqrt(l (l + 1)) (src/lbo.c:41-68) */
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
  opts.structSize = sizeof opts; opts.device = -1; opts.demoteToF32 = 1; opts.seed = seed; opts.maxRhs = 64;
  BfhipOperator *op = NULL;
  CHECK(bfhipCompileDesc(bfhipStreamerLayoutGetDesc(layout), &opts, &op));
  bfhipStreamerLayoutFree(&layout);
  free(bands); free(pts);
  uint64_t const m = bfhipGetNumRows(op), n = bfhipGetNumCols(op);
  printf("streamed butterfly: %llu rows x %llu columns (lmax = %llu), %.1f MB of fp32 leaves\n", (unsigned long long)m, (unsigned long long)n,
         (unsigned long long)lmax, (double)bfhipNumBytes(op) / 1e6);
  CHECK(bfhipSetRealRhsBlocks(op, 2));

  /* ---- GammaLam (a smooth spectrum) and the row permutation (the reversal) ---- */
  float *gam = malloc(n * sizeof *gam);
  uint64_t *perm = malloc(m * sizeof *perm);
  if (!gam || !perm) return 1;
  for (uint64_t j = 0; j < n; ++j) gam[j] = (float)(1.0 / (1.0 + 0.01 * (double)j));
  for (uint64_t i = 0; i < m; ++i) perm[i] = m - 1 - i;
  void *dGam = NULL, *dPerm = NULL, *dZ = NULL, *dSum = NULL, *dSumSq = NULL, *dW = NULL, *dZ1 = NULL;
  HIP(hipMalloc(&dGam, n * 4)); HIP(hipMalloc(&dPerm, m * 8)); HIP(hipMalloc(&dZ, m * numSamples * 4));
  HIP(hipMalloc(&dSum, m * 8)); HIP(hipMalloc(&dSumSq, m * 8)); HIP(hipMalloc(&dW, n * 4)); HIP(hipMalloc(&dZ1, m * 4));
  HIP(hipMemcpy(dGam, gam, n * 4, 1)); HIP(hipMemcpy(dPerm, perm, m * 8, 1));

  /* ---- (a) the loop as the reference writes it: one bfhipCovSampleDevice per sample, w already on the device ---- */
  CHECK(bfhipFillNormalDevice(dW, n, 0, BFHIP_F32, seed, NULL));
  CHECK(bfhipCovSampleDevice(op, dGam, dPerm, dW, dZ1, NULL));             /* warm-up */
  HIP(hipDeviceSynchronize());
  double t0 = now();
  for (uint64_t s = 0; s < numSamples; ++s) CHECK(bfhipCovSampleDevice(op, dGam, dPerm, dW, dZ1, NULL));
  HIP(hipDeviceSynchronize());
  double const msLoop = 1e3 * (now() - t0) / (double)numSamples;

  /* ---- (b) K samples drawn in blocks of 64, kept ---- */
  CHECK(bfhipCovDrawDevice(op, dGam, dPerm, seed, 0, numSamples < 64 ? numSamples : 64, dZ, NULL));   /* warm-up: grows the scratch */
  HIP(hipDeviceSynchronize());
  float *z = malloc(m * 64 * sizeof *z);
  double *ref = calloc(2 * m, sizeof *ref), *sum = malloc(2 * m * sizeof *sum);
  if (!z || !ref || !sum) return 1;
  t0 = now();
  for (uint64_t s0 = 0; s0 < numSamples; s0 += 64) {
    uint64_t const b = numSamples - s0 < 64 ? numSamples - s0 : 64;
    CHECK(bfhipCovDrawDevice(op, dGam, dPerm, seed, s0, b, (char *)dZ + s0 * m * 4, NULL));      /* block s0 / 64: [m x b], row-major */
  }
  HIP(hipDeviceSynchronize());
  double const msDraw = 1e3 * (now() - t0) / (double)numSamples;
  for (uint64_t s0 = 0; s0 < numSamples; s0 += 64) {                /* the moments of the stored samples, on the host */
    uint64_t const b = numSamples - s0 < 64 ? numSamples - s0 : 64;
    HIP(hipMemcpy(z, (char *)dZ + s0 * m * 4, m * b * 4, 2));
    for (uint64_t i = 0; i < m; ++i) for (uint64_t q = 0; q < b; ++q) { double const v = z[i * b + q]; ref[i] += v; ref[m + i] += v * v; }
  }

  /* ---- (c) the same K samples, never stored: pointwise sum and sum of squares ---- */
  HIP(hipMemset(dSum, 0, m * 8)); HIP(hipMemset(dSumSq, 0, m * 8));
  t0 = now();
  CHECK(bfhipCovMomentsDevice(op, dGam, dPerm, seed, 0, numSamples, 64, dSum, dSumSq, NULL));
  HIP(hipDeviceSynchronize());
  double const msMoments = 1e3 * (now() - t0) / (double)numSamples;
  HIP(hipMemcpy(sum, dSum, m * 8, 2)); HIP(hipMemcpy(sum + m, dSumSq, m * 8, 2));
  double worst = 0, meanVar = 0;
  for (uint64_t i = 0; i < m; ++i) {
    double const e1 = fabs(sum[i] - ref[i]) / (fabs(ref[i]) + 1e-300), e2 = fabs(sum[m + i] - ref[m + i]) / (ref[m + i] + 1e-300);
    /* (the sum of a row may cancel: its error is measured against the sum of squares' root instead when that is larger) */
    double const e1s = fabs(sum[i] - ref[i]) / (sqrt(ref[m + i] * (double)numSamples) + 1e-300);
    if ((e1 < e1s ? e1 : e1s) > worst) worst = e1 < e1s ? e1 : e1s;
    if (e2 > worst) worst = e2;
    double const mean = sum[i] / (double)numSamples;
    meanVar += sum[m + i] / (double)numSamples - mean * mean;
  }
  printf("loop of bfhipCovSampleDevice   %10.4f ms per sample\n", msLoop);
  printf("bfhipCovDrawDevice, 64 a call  %10.4f ms per sample\n", msDraw);
  printf("bfhipCovMomentsDevice          %10.4f ms per sample\n", msMoments);
  printf("pointwise variance over %llu samples: mean %.6e; moments vs the stored samples: worst relative difference %.2e\n",
         (unsigned long long)numSamples, meanVar / (double)m, worst);
  hipFree(dGam); hipFree(dPerm); hipFree(dZ); hipFree(dSum); hipFree(dSumSq); hipFree(dW); hipFree(dZ1);
  free(gam); free(perm); free(z); free(ref); free(sum);
  bfhipFree(&op);
  if (!(worst < 1e-10)) { fprintf(stderr, "the streamed moments differ from the stored samples'\n"); return 5; }
  return 0;
}
