/* bfhip_synth.h -- counter-based synthetic value stream shared by host and
 * device code.  Benchmark operands at N >= 262144 are "structure-exact,
 * value-random" (SURVEY.md section 8(d)): only block shapes come from the
 * reference's structure logic, values are this stream.  Every operation
 * below is exact in IEEE double (integer -> double below 2^53, scaling by a
 * power of two, a subtraction of two multiples of 2^-52 with |result| < 1),
 * so host and device produce bit-identical operands.  (The normal stream
 * at the end of the file goes through log / cos and is not: see there.)
 */
#ifndef BFHIP_SYNTH_H
#define BFHIP_SYNTH_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BFHIP_HD __host__ __device__ static inline
#else
#define BFHIP_HD static inline
#endif

BFHIP_HD uint64_t bfhip_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

/* uniform in [-1, 1) */
BFHIP_HD double bfhip_synth_value(uint64_t seed, uint64_t idx, int imag) {
  uint64_t z = bfhip_mix64(seed + 0x9e3779b97f4a7c15ULL * (2 * idx + (uint64_t)(imag != 0) + 1));
  return (double)(int64_t)(z >> 11) * 0x1.0p-52 - 1.0;
}

/* Standard normal number `idx` of the normal stream for `seed`: one value per index, a function of (seed, idx) alone, so any
 * split of an index range over calls, batches or devices draws the same numbers.  Box-Muller, cosine branch, over two
 * uniforms of the bfhip_mix64 stream at counter idx + 1, one per keyed stream (the keys are fixed here, for good):
 *   u1 = ((z1 >> 11) + 1) * 2^-53  in (0, 1]   (the logarithm is finite),   z1 = mix64((seed ^ BFHIP_NORMAL_KEY_U1) + golden * (idx + 1))
 *   u2 =  (z2 >> 11)      * 2^-53  in [0, 1),                               z2 = mix64((seed ^ BFHIP_NORMAL_KEY_U2) + golden * (idx + 1))
 *   value = sqrt(-2 ln u1) * cos(2 pi u2),   |value| <= sqrt(106 ln 2) < 8.6
 * The uniforms, -2 * ln and the argument 2 pi * u2 (one rounded product) are identical on host and device; `log`, `cos` and
 * hence the value are NOT bit-identical between the host's libm and the device's math library: they agree to the accuracy of
 * those two functions (a few ulp of double; the tests hold 8).  The device evaluates this very function in double for both
 * element types and rounds to float once for F32. */
#define BFHIP_NORMAL_KEY_U1 0xd1b54a32d192ed03ULL
#define BFHIP_NORMAL_KEY_U2 0x8cb92ba72f3d8dd7ULL
BFHIP_HD double bfhip_normal_value(uint64_t seed, uint64_t idx) {
  uint64_t const c = 0x9e3779b97f4a7c15ULL * (idx + 1);
  uint64_t const z1 = bfhip_mix64((seed ^ BFHIP_NORMAL_KEY_U1) + c), z2 = bfhip_mix64((seed ^ BFHIP_NORMAL_KEY_U2) + c);
  double const u1 = (double)((z1 >> 11) + 1) * 0x1.0p-53, u2 = (double)(z2 >> 11) * 0x1.0p-53;
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

#endif
