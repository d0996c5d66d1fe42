/* bfhip_cond.h -- struct BfhipCovCond, shared by the two host files that implement it: bfhip_cond.c (create, free, samples,
 * moments) and bfhip_condlik.c (log-likelihood with gradients, kriging variances), and the device entry points of the latter
 * (bfhip_condlik.hip).  Private to those files.
 */
#ifndef BFHIP_COND_H
#define BFHIP_COND_H

#include "bfhip_operator.h"
#include "../../include/bfhip.h"

typedef struct BfCondKey { uint64_t idx; uint32_t slot; } BfCondKey;      /* an index and the place it came from (condLookupSort) */

/* What the object needs from the field z = B w it conditions (B is m x n): the sizes, the element type of the blocks and four
 * calls.  Two backends fill it: the butterfly route (bfhip_cond.c: B = P A GammaLam of an operator) and the Chebyshev route
 * (bfhip_cheb.c: B = D p(S), m = n, float64, no permutation).
 *   panel   columns c0 .. c0 + p - 1 of the double matrix Bt [n x ld] = the rows of B at dRows[0 .. p), p <= 64, transposed
 *   wprime  where the packed block W' [n x b] of a pass starts (read at every pass: a scratch may have been grown since)
 *   field   the b columns of W' into the field block: dZ [m x b] packed (then `scatter` says whether the rows are permuted), or
 *           with dZ == NULL into scratch of the backend's, whose place *packed receives
 *   live    NULL, or the refusal of an object whose backend has changed under it (stale Chebyshev coefficients) */
typedef struct BfCondBackend {
  uint64_t n, m;
  uint32_t dtype;
  size_t elemSize;
  int columnWeights;             /* B = (...) GammaLam: the likelihood has a gradient in log gamma */
  int (*panel)(BfhipCovCond *c, uint64_t const *dRows, uint32_t p, double *Bt, uint32_t ld, uint32_t c0, void *stream);
  void *(*wprime)(BfhipCovCond *c);
  int (*field)(BfhipCovCond *c, uint32_t b, int scatter, void *dZ, void **packed, void *stream);
  int (*live)(BfhipCovCond const *c);
} BfCondBackend;

struct BfhipCovCond {
  BfCondBackend be;
  BfhipOperator *op;             /* butterfly route: referenced, like dGammaLam and dRowPerm */
  void const *dGammaLam;
  uint64_t const *dRowPerm;      /* NULL on the Chebyshev route */
  BfhipChebCov *cheb;            /* Chebyshev route: referenced */
  uint64_t chebGeneration;       /* the coefficients Bt was made with */
  void *dWp;                     /* Chebyshev route: the object's own W' block [n x 64], also the unit panel of a setup pass */
  int device;                    /* the backend's, kept so that Free reads nothing through op / cheb */
  uint32_t k;
  double *dBt;                   /* [n x k] */
  double *dL;                    /* [k x k]: G + D, then L */
  double *dNoiseVar, *dNoiseSd;  /* [k] each; NULL without noise */
  double *dR;                    /* [k x 64]: R, solved in place into alpha */
  double *dE;                    /* [k x 64]: the draw's noise block */
  void *dWn;                     /* [n x 64], the backend's dtype: the draw's normals */
  double *dPart;                 /* [chunks x k x 64]: partial sums of R */
  BfhipCovCondInfo info;
  /* bfhip_condlik.c: allocated by the first likelihood / variance call, not counted in info.factorBytes */
  double *dStrips;               /* [likSlots x k x 64]: the strips of the wide solve, one per workgroup */
  uint64_t likSlots;             /* strips dStrips holds */
  double *dLinv;                 /* [ceil(k / 64) x 64 x 64]: the inverses of the diagonal tiles of L */
  double *dColSq;                /* [n + k]: ||L^-1 b_j||^2, then ||L^-1 e_a||^2 */
  double *dVarBlk;               /* [n x 64]: a panel of rows of P A GammaLam, transposed (variance) */
  double *dVarPart;              /* [chunks x 64] partial sums of its columns' squares, then [64] ||L^-1 Bt^T r||^2, then [k] zeros */
  /* bfhip_cheb.c: the gradient in the density's parameters (Chebyshev route) */
  uint64_t *hObs;                /* host [k]: the observed vertices, kept by bfhipChebCovCondCreate (the unit panels are made again) */
  uint64_t *dGradRows;           /* [k]: the same on the device, uploaded by the first gradient call like everything below */
  double *dGradY;                /* [n x 64]: Y = X M[:, panel] */
  double *dGradM;                /* [k x 64] K^-1[:, panel] packed at the panel's width, then [k x 64] M[:, panel] */
  double *dGradPart;             /* [64 x chunks]: a panel's partial sums, one row per parameter */
};

/* releases what bfhip_condlik.c allocated (the device is drained by the caller) */
BF_HIDDEN void condLikRelease(BfhipCovCond *c);
/* the whole object (bfhip_cond.c; the device is drained by the caller) */
BF_HIDDEN void condRelease(BfhipCovCond *c);
/* the refusals the two constructors share that need the arguments alone, in this order: a repeated index, a bad noiseVar entry.
 * *keys as condLookupSort leaves them (free() them), NULL after a refusal */
BF_HIDDEN int condCheckObs(uint64_t const *obs, uint32_t k, double const *noiseVar, BfCondKey **keys);
/* the rest of a Create once c->be, c->k and c->device are set, the device is entered and the backend's scratch holds passes of 64
 * columns: the object's blocks, Bt by panels, G + D, its Cholesky factor; c->info (factorBytes is ADDED to).  The caller releases
 * c after a failure */
BF_HIDDEN int condSetup(BfhipCovCond *c, BfCondKey const *keys, uint64_t const *obs, double const *noiseVar, void *stream);

/* The rows i_t with dRowPerm[i_t] = idx[t], t < count (bfhip_cond.c): Create looks up its observed indices with it, the variance its
 * queries; `what` ("observed" / "query") is the word the refusals use.  In steps, because each caller has refusals and device work
 * of its own between them (Create validates its noise between the first two):
 *   condLookupSort   *keys = the indices sorted, each with the place it came from (free() it); a repeated index is refused
 *   condLookupRange  an index >= numRows is refused
 *   condLookupRows   dRows [count], allocated by the caller on the current device: dRowPerm inverted there (refused unless every
 *                    index is hit exactly once; drains `stream`), or idx itself without a permutation */
BF_HIDDEN int condLookupSort(uint64_t const *idx, uint32_t count, char const *what, BfCondKey **keys);
BF_HIDDEN int condLookupRange(BfCondKey const *keys, uint32_t count, char const *what, uint64_t numRows);
BF_HIDDEN int condLookupRows(BfCondKey const *keys, uint64_t const *idx, uint32_t count, char const *what, uint64_t const *dRowPerm, uint64_t numRows, void *dRows,
                             void *stream);
/* One panel of p <= 64 rows of P A GammaLam, transposed, into columns c0 .. c0 + p - 1 of Bt [n x k]: unit columns at dRows[0 .. p)
 * in the first half of the operator's covariance scratch (taken at 64 columns), A^T of them into the second, packed with GammaLam */
BF_HIDDEN int condAdjointPanel(BfhipOperator *op, void const *dGammaLam, uint64_t const *dRows, uint32_t p, double *Bt, uint32_t k, uint32_t c0, void *stream);

/* ---- the device entry points of bfhip_condlik.c, defined in bfhip_condlik.hip ---- */
#define BF_LIK_STRIP 64u             /* columns of a strip of the wide solve */
#define BF_LIK_NB 64u                /* its block rows: the diagonal tiles of L whose inverses are kept */
enum { BF_LIK_SRC_BT_ROWS = 0, BF_LIK_SRC_IDENTITY = 1, BF_LIK_SRC_BLOCK = 2 };
#ifdef __cplusplus
extern "C" {
#endif
/* Linv [ceil(k / 64)][64][64] = the inverses of the diagonal tiles of L (identity beyond row k) */
int bfdevLikInvDiag(double *Linv, double const *L, uint32_t k, void *stream);
/* out[s] = sum_a X[a, s]^2, L X = S, for the numCols columns of S [k x numCols] (never stored):
 *   BT_ROWS:  S[a, s] = src[s * k + a]  (src = Bt: its rows are the columns)
 *   IDENTITY: S = I (numCols = k; src unused)
 *   BLOCK:    S[a, s] = src[a * ld + s]
 * strips [slots x k x 64] is scratch: workgroup g owns strips[g] and the columns of strips g, g + slots, ... of S */
int bfdevLikStripSolve(double const *L, double const *Linv, uint32_t k, int kind, double const *src, uint64_t ld, uint64_t numCols, double *strips, uint64_t slots, double *out,
                       void *stream);
/* value[3] = { logLik, quad = sum_a y[a] alpha[a], logDet = 2 sum_a log L[a, a] } */
int bfdevLikValue(double *value, double const *L, uint32_t k, double const *y, double const *alpha, void *stream);
/* grad[j] = (sum_a Bt[j, a] alpha[a])^2 - colSq[j] */
int bfdevLikGradGamma(double *grad, double const *Bt, uint64_t n, uint32_t k, double const *alpha, double const *colSq, void *stream);
/* grad[a] = (alpha[a]^2 - colSq[a]) / 2 */
int bfdevLikGradNoise(double *grad, double const *alpha, double const *colSq, uint32_t k, void *stream);
/* part[c][s] = sum over the rows j of chunk c (BF_COND_CHUNK rows) of blk[j, s]^2, blk [n x p], p <= 64 */
int bfdevVarPriorPart(double *part, double const *blk, uint64_t n, uint32_t p, void *stream);
/* prior[s] = sum_c part[c][s] in chunk order (NULL: not stored), post[s] = that - solved[s] (NULL: not stored), s < p */
int bfdevVarAssemble(double *prior, double *post, double const *part, uint64_t chunks, double const *solved, uint32_t p, void *stream);

/* ---- the gradient in the density's parameters (bfhip_likgrad.hip; driven by bfhip_cheb.c), one panel of pc <= 64 observed
 * columns c0 .. c0 + pc - 1 at a time ---- */
/* E [k x pc] packed = the panel's columns of the identity */
int bfdevLikGradUnit(double *E, uint32_t k, uint32_t c0, uint32_t pc, void *stream);
/* Mp [k x 64]: Mp[a, c] = alpha[a] alpha[c0 + c] - Kinv[a, c] for c < pc (Kinv [k x pc] packed), zero beyond */
int bfdevLikGradM(double *Mp, double const *alpha, double const *Kinv, uint32_t k, uint32_t c0, uint32_t pc, void *stream);
/* Y [n x 64] = X [n x k] Mp [k x 64] on the FP64 matrix cores; columns >= pc of Mp are not read, those of Y are exact zeros */
int bfdevLikGradContract(double *Y, double const *X, uint64_t n, uint32_t k, double const *Mp, uint32_t pc, void *stream);
/* part[chunk] = sum over the rows r of the chunk (BF_COND_CHUNK rows) and c < pc of Y[r, c] Xp[r, c]; Y [n x 64], Xp [n x pc] packed */
int bfdevLikGradDot(double *part, double const *Y, double const *Xp, uint64_t n, uint32_t pc, void *stream);
/* grad[t] = (first ? 0 : grad[t]) + sum_chunk part[t * chunks + chunk] in chunk order, t < numParams */
int bfdevLikGradSum(double *grad, double const *part, uint64_t chunks, uint32_t numParams, int first, void *stream);
#ifdef __cplusplus
}
#endif

#endif
