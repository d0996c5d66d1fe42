/* bfhip_shim.c -- the BfMat vtable shim that makes the device operator a drop-in behind the reference's bfMatMul /
 * bfMatMulVec (reference src/mat.c:183-189; precedent for a foreign operator behind the vtable: BfMatFunc,
 * include/bf/mat_func.h:5-28, src/mat_func.c:59-82).
 */
#define _GNU_SOURCE
#include "bfhip_operator.h"
#include "../../include/bfhip_abi.h"

#include <dlfcn.h>
#include <stdlib.h>
#include <string.h>

/* =============================================================================
 * BfMat vtable shim
 * ============================================================================= */
typedef struct BfhipMat {
  BfAbiMat super;             /* must be first: this IS a BfMat */
  BfhipOperator *op;          /* the operator; with `sh`: this rank's share of it (shape queries go to `sh`) */
  int ownsOperator;
  int transposed;             /* bfMatTranspose has been applied an odd number of times: Mul / MulVec run the adjoint plan */
  struct BfhipSharded *sh;    /* bfhipShardedMatNew: applies are the sharded step (every rank's host calls with the same vectors) */
  int ownsSharded;
} BfhipMat;

/* rows / columns of the operator the object stands for (untransposed), and the host-vector apply behind every slot */
static uint64_t shimOpRows(BfhipMat const *s) { return s->sh ? bfhipShardedGetNumRows(s->sh) : bfhipGetNumRows(s->op); }
static uint64_t shimOpCols(BfhipMat const *s) { return s->sh ? bfhipShardedGetNumCols(s->sh) : bfhipGetNumCols(s->op); }
static int shimApplyHost(BfhipMat const *s, int transpose, void const *X, size_t ldx, size_t nrhs, void *Y, size_t ldy) {
  return s->sh ? bfhipShardedApplyHost(s->sh, transpose, X, ldx, nrhs, Y, ldy) : applyHost(s->op, transpose, X, ldx, nrhs, Y, ldy);
}

/* Failures surface the way the reference's own Mul failures do: the global error code is set
 * (bfSetError, src/error.c:20-24) and NULL is returned (the RAISE_ERROR / BF_ERROR_END idiom, e.g.
 * src/mat_product.c:404-405).  libbfhip does not link the reference; when the host process has
 * it loaded its bfSetError is found at run time.  Note that bfSetError asserts on a non-zero code
 * (src/error.c:21), so in a reference build with assertions a failed Mul is as fatal as the
 * reference's own BF_DIE() paths; bfhipSetErrorForwarding(0) keeps failures to NULL +
 * bfhipLastErrorMessage(). */
static int forwardErrors = 1;
void bfhipSetErrorForwarding(int on) { forwardErrors = on; }
static void shimRaise(int code) {
  if (!forwardErrors || !code) return;
  static void (*setError)(int);
  static int looked;
  if (!looked) { looked = 1; setError = (void (*)(int))dlsym(RTLD_DEFAULT, "bfSetError"); }
  if (setError) setError(code);
}
#define SHIM_FAIL(code, ...) do { shimRaise(bfhipFail((code), __VA_ARGS__)); return NULL; } while (0)

/* shape of what the object currently stands for: A, or A^T after bfMatTranspose (the reference's transposed product
 * answers with its reversed, transposed factors' shapes: src/mat_product.c:146-192, 409-420) */
static size_t shimGetNumRows(BfAbiMat const *m) { BfhipMat const *s = (BfhipMat const *)m; return s->transposed ? shimOpCols(s) : shimOpRows(s); }
static size_t shimGetNumCols(BfAbiMat const *m) { BfhipMat const *s = (BfhipMat const *)m; return s->transposed ? shimOpRows(s) : shimOpCols(s); }
static int shimGetType(BfAbiMat const *m) { (void)m; return BFABI_TYPE_MAT_FUNC; }
static size_t shimNumBytes(BfAbiMat const *m) { return bfhipNumBytes(((BfhipMat const *)m)->op); }
static void shimDelete(BfAbiMat **m) {
  if (!m || !*m) return;
  BfhipMat *s = (BfhipMat *)*m;
  /* a view never owns the operator (bfMatDenseRealDeinit skips the payload of a view the same way,
   * src/mat_dense_real.c:1667-1672) */
  if (s->ownsSharded && s->sh && !(s->super.props & BFABI_MAT_PROPS_VIEW)) bfhipShardedFree(&s->sh);
  if (s->ownsOperator && !(s->super.props & BFABI_MAT_PROPS_VIEW)) bfhipFree(&s->op);
  free(s);
  *m = NULL;
}
/* GetView: a shallow copy flagged VIEW, what every reference type returns (e.g.
 * bfMatDenseRealGetView, src/mat_dense_real.c:67-85).  bfMatBlockDenseGetBlockConst calls it on
 * every sub-block of a BlockDense on each Mul (src/mat_block_dense.c:1043-1061, via bfMatGet
 * with BF_POLICY_VIEW), so a shim placed INSIDE a reference container needs it. */
static BfAbiMat *shimGetView(BfAbiMat *m) {
  BfhipMat *v = malloc(sizeof *v);
  if (!v) SHIM_FAIL(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  *v = *(BfhipMat *)m;
  v->super.props |= BFABI_MAT_PROPS_VIEW;
  return &v->super;
}

/* Y = A X for a reference dense RHS; the result is allocated through the
 * RHS's own EmptyLike slot so the reference owns and frees it
 * (bfMatBlockCooMul does the same with ZerosLike, mat_block_coo.c:401). */
static void *shimMulImpl(void const *rhsV, BfhipMat const *self, int transpose) {
  BfAbiMat const *rhs = rhsV;
  BfhipOperator *op = self ? self->op : NULL;
  if (!op || !rhs || !rhs->vtbl) SHIM_FAIL(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operand");
  if (transpose && !op->hasTplan) SHIM_FAIL(BFABI_ERROR_NOT_IMPLEMENTED, "Mul on a transposed operator needs BFHIP_FLAG_ADJOINT");
  uint64_t const inLen = transpose ? shimOpRows(self) : shimOpCols(self), outLen = transpose ? shimOpCols(self) : shimOpRows(self);
  BfAbiGetTypeFn getType = (BfAbiGetTypeFn)rhs->vtbl->slot[BFABI_SLOT_GetType];
  if (!getType || getType(rhs) != BFABI_TYPE_MAT_DENSE_COMPLEX || op->srcDtype != BFHIP_C128)
    /* same restriction as bfMatDenseComplexMul's switch (mat_dense_complex.c:1036-1047) */
    SHIM_FAIL(BFABI_ERROR_NOT_IMPLEMENTED, "Mul needs a complex operator and a BfMatDenseComplex right-hand side");
  if (rhs->props & (BFABI_MAT_PROPS_TRANS | BFABI_MAT_PROPS_CONJ)) SHIM_FAIL(BFABI_ERROR_NOT_IMPLEMENTED, "transposed right-hand side");
  BfAbiMatDenseComplex const *x = (BfAbiMatDenseComplex const *)rhs;
  if (rhs->numRows != inLen)
    SHIM_FAIL(BFABI_ERROR_INCOMPATIBLE_SHAPES, "operator has %llu columns, right-hand side %llu rows", (unsigned long long)inLen, (unsigned long long)rhs->numRows);
  BfAbiLikeFn emptyLike = (BfAbiLikeFn)rhs->vtbl->slot[BFABI_SLOT_EmptyLike];
  if (!emptyLike) SHIM_FAIL(BFABI_ERROR_INVALID_ARGUMENTS, "right-hand side has no EmptyLike");
  /* a column-strided right-hand side (a view of every k-th column, a column range of a wider matrix:
   * bfMatDenseComplexGetColRange leaves colStride as it is, src/mat_dense_complex.c:648-672) is gathered into a packed
   * copy first -- cblas_zgemm in the reference cannot take it either (it passes ldb = rowStride and assumes unit column
   * stride, :1754), so this is more than the reference does, not less */
  /* A transposed COMPLEX object multiplies as its conjugate transpose, as in the reference: bfMatTranspose ends in
   * bfMatDenseComplexTranspose = bfMatConjTrans on every dense leaf (src/mat_dense_complex.c:1475-1478, src/mat.c:359-362) and
   * getCblasTranspose maps the flags to CblasConjTrans (:27-35).  A^H X = conj(A^T conj(X)): the right-hand side is
   * conjugated into the packed copy, the result in place. */
  void *packed = NULL;
  void const *xdata = x->data;
  size_t xld = x->rowStride;
  if (x->colStride != 1 || transpose) {
    if (x->colStride == 0) SHIM_FAIL(BFABI_ERROR_INVALID_ARGUMENTS, "right-hand side with colStride 0");
    size_t const nr = rhs->numRows, nc = rhs->numCols;
    packed = malloc((nr && nc ? nr * nc : 1) * 16);
    if (!packed) SHIM_FAIL(BFABI_ERROR_MEMORY_ERROR, "host OOM");
    for (size_t i = 0; i < nr; ++i)
      for (size_t q = 0; q < nc; ++q) {
        double const *e = (double const *)((char const *)x->data + (i * x->rowStride + q * x->colStride) * 16);
        double *d = (double *)((char *)packed + (i * nc + q) * 16);
        d[0] = e[0]; d[1] = transpose ? -e[1] : e[1];
      }
    xdata = packed; xld = nc;
  }
  BfAbiMat *res = emptyLike(rhs, outLen, rhs->numCols);
  if (!res) { free(packed); SHIM_FAIL(BFABI_ERROR_MEMORY_ERROR, "EmptyLike failed"); }
  BfAbiMatDenseComplex *y = (BfAbiMatDenseComplex *)res;
  int rc;
  if (y->colStride != 1) rc = bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "EmptyLike returned a result with colStride != 1");
  else rc = shimApplyHost(self, transpose, xdata, xld, rhs->numCols, y->data, y->rowStride);
  if (!rc && transpose)
    for (size_t i = 0; i < outLen; ++i)
      for (size_t q = 0; q < rhs->numCols; ++q) ((double *)y->data)[2 * (i * y->rowStride + q) + 1] *= -1.0;
  free(packed);
  if (rc) {
    BfAbiDeleteFn del = (BfAbiDeleteFn)res->vtbl->slot[BFABI_SLOT_Delete];
    if (del) del(&res);
    shimRaise(rc);
    return NULL;
  }
  return res;
}

void *bfhipMatMulFunc(void const *rhsV, void *opV) {
  BfhipMat tmp;
  memset(&tmp, 0, sizeof tmp);
  tmp.op = opV;
  return shimMulImpl(rhsV, &tmp, 0);
}

static BfAbiMat *shimMul(BfAbiMat const *lhs, BfAbiMat const *rhs) {
  return shimMulImpl(rhs, (BfhipMat const *)lhs, ((BfhipMat const *)lhs)->transposed);
}

/* bfMatRmul(A_hip, X) = X A (slot 44, src/mat.c:195-197; bfMatProductRmul walks the factors in order, src/mat_product.c:282-310, down
 * to bfMatDenseComplexRmul's one zgemm, src/mat_dense_complex.c:1075-1133 -- a dense complex `otherMat` only, :1125-1133).
 * X A = (A^T X^T)^T: the adjoint plan applied to the rows of X as right-hand sides.  X^T is gathered into a packed copy (any row /
 * column stride of X), the result is scattered into a matrix allocated through X's EmptyLike.  After bfMatTranspose the object
 * stands for A^H (shimMulImpl): X A^H = conj(conj(X) A^T) = conj((A conj(X)^T)^T), the FORWARD plan between two conjugations. */
static BfAbiMat *shimRmul(BfAbiMat const *lhs, BfAbiMat const *other) {
  BfhipMat const *self = (BfhipMat const *)lhs;
  BfhipOperator *op = self ? self->op : NULL;
  if (!op || !other || !other->vtbl) SHIM_FAIL(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operand");
  int const conj = self->transposed, transpose = !self->transposed;          /* which plan runs */
  if (transpose && !op->hasTplan) SHIM_FAIL(BFABI_ERROR_NOT_IMPLEMENTED, "Rmul needs an operator compiled with BFHIP_FLAG_ADJOINT");
  BfAbiGetTypeFn getType = (BfAbiGetTypeFn)other->vtbl->slot[BFABI_SLOT_GetType];
  if (!getType || getType(other) != BFABI_TYPE_MAT_DENSE_COMPLEX || op->srcDtype != BFHIP_C128)
    SHIM_FAIL(BFABI_ERROR_NOT_IMPLEMENTED, "Rmul needs a complex operator and a BfMatDenseComplex left operand");
  if (other->props & (BFABI_MAT_PROPS_TRANS | BFABI_MAT_PROPS_CONJ)) SHIM_FAIL(BFABI_ERROR_NOT_IMPLEMENTED, "transposed left operand");
  /* rows / columns of what the object stands for */
  uint64_t const rows = self->transposed ? shimOpCols(self) : shimOpRows(self), cols = self->transposed ? shimOpRows(self) : shimOpCols(self);
  size_t const m = other->numRows, k = other->numCols;
  if (k != rows) SHIM_FAIL(BFABI_ERROR_INCOMPATIBLE_SHAPES, "operator has %llu rows, left operand %llu columns", (unsigned long long)rows, (unsigned long long)k);
  BfAbiLikeFn emptyLike = (BfAbiLikeFn)other->vtbl->slot[BFABI_SLOT_EmptyLike];
  if (!emptyLike) SHIM_FAIL(BFABI_ERROR_INVALID_ARGUMENTS, "left operand has no EmptyLike");
  BfAbiMatDenseComplex const *x = (BfAbiMatDenseComplex const *)other;
  double *xt = malloc((k && m ? k * m : 1) * 16), *zt = malloc((cols && m ? cols * m : 1) * 16);
  if (!xt || !zt) { free(xt); free(zt); SHIM_FAIL(BFABI_ERROR_MEMORY_ERROR, "host OOM"); }
  for (size_t q = 0; q < m; ++q)
    for (size_t i = 0; i < k; ++i) {
      double const *e = (double const *)((char const *)x->data + (q * x->rowStride + i * x->colStride) * 16);
      xt[2 * (i * m + q)] = e[0]; xt[2 * (i * m + q) + 1] = conj ? -e[1] : e[1];
    }
  int rc = shimApplyHost(self, transpose, xt, m, m, zt, m);          /* (k x m) -> (cols x m) */
  free(xt);
  if (rc) { free(zt); shimRaise(rc); return NULL; }
  BfAbiMat *res = emptyLike(other, m, cols);
  if (!res) { free(zt); SHIM_FAIL(BFABI_ERROR_MEMORY_ERROR, "EmptyLike failed"); }
  BfAbiMatDenseComplex *y = (BfAbiMatDenseComplex *)res;
  for (size_t q = 0; q < m; ++q)
    for (size_t j = 0; j < cols; ++j) {
      double *d = (double *)((char *)y->data + (q * y->rowStride + j * y->colStride) * 16);
      d[0] = zt[2 * (j * m + q)]; d[1] = conj ? -zt[2 * (j * m + q) + 1] : zt[2 * (j * m + q) + 1];
    }
  free(zt);
  return res;
}

/* bfMatTranspose (slot 63, src/mat.c:271-273): in place, as bfMatProductTranspose reverses and transposes its factors
 * (src/mat_product.c:409-420).  The adjoint plan over the same packed leaves exists already (BFHIP_FLAG_ADJOINT), so the
 * object only changes which of its two plans Mul / MulVec / RmulVec run and what GetNumRows / GetNumCols answer; twice
 * is the identity.  For a REAL operator that is the transpose; a COMPLEX one multiplies as its conjugate transpose
 * afterwards, as the reference's does (its dense complex leaves transpose by bfMatConjTrans: shimMulImpl).  The slot returns nothing: without an
 * adjoint plan the reference's error state is raised (NOT_IMPLEMENTED) and the object is left as it was. */
static void shimTranspose(BfAbiMat *m) {
  BfhipMat *s = (BfhipMat *)m;
  if (!s->op->hasTplan) { shimRaise(bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "Transpose needs an operator compiled with BFHIP_FLAG_ADJOINT")); return; }
  s->transposed = !s->transposed;
  size_t const r = s->super.numRows;
  s->super.numRows = s->super.numCols;
  s->super.numCols = r;
}

/* y = A x (transpose == 0) or z = x^T A as a vector (bfMatRmulVec) for a reference BfVecReal; real
 * operators only: the block types reject complex vectors (mat_block_coo.c:438-444).  The result
 * is sized by the operator, as the reference's containers size theirs (bfVecRealNewWithValue(m, 0)
 * in src/mat_block_dense.c:574-590 and src/mat_block_coo.c:427-444; n for RmulVec, :696-712):
 * a malloc'd BfVecReal {vtbl, props NONE, size, stride 1, malloc'd data} carrying the ARGUMENT's
 * vtable, so that the reference's bfVecDelete -> bfVecRealDeinitAndDealloc frees data and struct with
 * free() (src/vec_real.c:661-676, src/mem.c:65-67).  Rectangular operators are the normal case:
 * cov_matvec applies the N x m operator Phi both ways (examples/covariance/lbo_cov.c:48-60). */
static BfAbiVec *shimApplyVec(BfAbiMat const *lhs, BfAbiVec const *vec, int rmul) {
  BfhipOperator *op = ((BfhipMat const *)lhs)->op;
  char const *const what = rmul ? "RmulVec" : "MulVec";
  int const transpose = rmul != ((BfhipMat const *)lhs)->transposed;          /* x^T (A^T) = (A x)^T */
  if (!vec || !vec->vtbl) SHIM_FAIL(BFABI_ERROR_INVALID_ARGUMENTS, "%s: NULL vector", what);
  BfAbiVecGetTypeFn getType = (BfAbiVecGetTypeFn)vec->vtbl->slot[BFABI_VSLOT_GetType];
  if (!getType || getType(vec) != BFABI_TYPE_VEC_REAL || op->srcDtype != BFHIP_F64)
    SHIM_FAIL(BFABI_ERROR_NOT_IMPLEMENTED, "%s needs a real operator and a BfVecReal", what);
  if (transpose && !op->hasTplan) SHIM_FAIL(BFABI_ERROR_NOT_IMPLEMENTED, "%s needs an operator compiled with BFHIP_FLAG_ADJOINT", what);
  BfhipMat const *self = (BfhipMat const *)lhs;
  uint64_t const inLen = transpose ? shimOpRows(self) : shimOpCols(self);
  uint64_t const outLen = transpose ? shimOpCols(self) : shimOpRows(self);
  if (vec->size != inLen)
    SHIM_FAIL(BFABI_ERROR_INCOMPATIBLE_SHAPES, "%s: operator expects %llu entries, vector has %llu", what, (unsigned long long)inLen, (unsigned long long)vec->size);
  BfAbiVecReal const *x = (BfAbiVecReal const *)vec;
  BfAbiVecReal *y = malloc(sizeof *y);
  double *data = malloc((outLen ? outLen : 1) * sizeof(double));
  if (!y || !data) { free(y); free(data); SHIM_FAIL(BFABI_ERROR_MEMORY_ERROR, "host OOM"); }
  y->super.vtbl = vec->vtbl;
  y->super.props = BFABI_VEC_PROPS_NONE;
  y->super.size = outLen;
  y->stride = 1;
  y->data = data;
  int rc = shimApplyHost(self, transpose, x->data, x->stride, 1, y->data, 1);
  if (rc) { free(data); free(y); shimRaise(rc); return NULL; }
  return &y->super;
}
static BfAbiVec *shimMulVec(BfAbiMat const *lhs, BfAbiVec const *vec) { return shimApplyVec(lhs, vec, 0); }
static BfAbiVec *shimRmulVec(BfAbiMat const *lhs, BfAbiVec const *vec) { return shimApplyVec(lhs, vec, 1); }

/* ToType (slot 54, bfMatToType) densifies through the extraction of bfhip_extract.c.  The slot is referenced weakly so that this
 * file still links without that one (the host sanitizer harness links the plan-side files alone: there the slot stays NULL). */
extern BfAbiMat *bfhipShimToType(BfAbiMat const *m, int type) __attribute__((weak));

static BfAbiMatVtable ShimVtable = {.slot = {
  [BFABI_SLOT_GetView] = (void *)shimGetView,
  [BFABI_SLOT_RmulVec] = (void *)shimRmulVec,
  [BFABI_SLOT_Delete] = (void *)shimDelete,
  [BFABI_SLOT_GetType] = (void *)shimGetType,
  [BFABI_SLOT_NumBytes] = (void *)shimNumBytes,
  [BFABI_SLOT_GetNumRows] = (void *)shimGetNumRows,
  [BFABI_SLOT_GetNumCols] = (void *)shimGetNumCols,
  [BFABI_SLOT_Mul] = (void *)shimMul,
  [BFABI_SLOT_Rmul] = (void *)shimRmul,
  [BFABI_SLOT_MulVec] = (void *)shimMulVec,
  [BFABI_SLOT_Transpose] = (void *)shimTranspose,
  [BFABI_SLOT_ToType] = (void *)bfhipShimToType,
}};

int bfhipShimGet(void const *mat, BfhipOperator **op, int *transposed, int *sharded) {
  BfhipMat const *s = mat;
  if (!s || s->super.vtbl != &ShimVtable) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "not a bfhipMatNew object");
  if (op) *op = s->op;
  if (transposed) *transposed = s->transposed;
  if (sharded) *sharded = s->sh != NULL;
  return 0;
}
void bfhipShimRaise(int code) { shimRaise(code); }

void *bfhipMatNew(BfhipOperator *op, int ownsOperator) {
  if (!op) { bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator"); return NULL; }
  BfhipMat *m = calloc(1, sizeof *m);
  if (!m) { bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); return NULL; }
  m->super.vtbl = &ShimVtable;
  m->super.props = BFABI_MAT_PROPS_NONE;
  m->super.numRows = op->plan.numRows;
  m->super.numCols = op->plan.numCols;
  m->op = op;
  m->ownsOperator = ownsOperator;
  return m;
}

/* the same object over a sharded operator: shapes are the whole operator's, applies are the sharded step */
void *bfhipShardedMatNew(struct BfhipSharded *sh, int ownsSharded) {
  if (!sh) { bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL sharded operator"); return NULL; }
  BfhipMat *m = calloc(1, sizeof *m);
  if (!m) { bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); return NULL; }
  m->super.vtbl = &ShimVtable;
  m->super.props = BFABI_MAT_PROPS_NONE;
  m->super.numRows = bfhipShardedGetNumRows(sh);
  m->super.numCols = bfhipShardedGetNumCols(sh);
  m->op = bfhipShardedOperator(sh);
  m->sh = sh;
  m->ownsSharded = ownsSharded;
  return m;
}
