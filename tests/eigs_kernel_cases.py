"""Designs, references and bounds for the eigensolver's kernels launched one at a time (bfhip_eigs.hip through bfdevEigsStep,
bfdevEigsGram, bfdevEigsRotate, bfdevEigsResidual, bfdevEigsStore and bfdevEigsChunkRows).  Builders
only: numpy, no GPU.  tests/test_eigs_kernels_cpu.py asserts what the designs claim (which branch each shape reaches, that
every omission a kernel could make breaks a bound by 1e3, that plain float64 passes every bound);
tests/test_gpu_eigs_kernels.py holds the device to the references built here.

Two kinds of input for every kernel:
  "int"    entries in [-3, 3], small integer scalars.  Every product and partial sum is an integer far below 2^53
           (int_worst_case), so the result is exact in any order of summation and the device has to return numpy's float64
           result bit for bit.  alpha > 0 in the step: then no sum of the kernel can end in -0.0 (alpha * (+0) = +0, and x + (+0)
           is never -0), and neither can the reference's, to which + 0.0 is added for that reason.
  "float"  standard normals (the step: the project's own folded matrices) against a numpy.longdouble reference, with the
           componentwise bounds of the operation count, u = 2^-53:
             Gram      |G - ref|_ij   <= (n + 2) u (|X|^T |Y|)_ij
             rotate    |out - ref|_ij <= (ld + 2) u (|X| |W|)_ij
             residual  |sumSq - ref|_c <= (n + 8) u ref_c            (d in long double, see Dense.residual_d; the kernel's fma rounds d once)
             step      |out - ref|_ic <= (nnz_i + 3) u (|alpha| sum_j |S_ij| |b1_jc| + |beta| |b1_ic| + |gamma| |b2_ic|)
             store     bit-equal to numpy's d[:, None] * X (one IEEE multiplication per element; without d a copy), so the
                       one design serves as both kinds.
           A bound of zero (the padding) asks for an exact zero.  References and bounds are formed in long double.

Blocks are [n, ld] with the first p columns in use and the padding columns zero, as the solver keeps them."""
import ctypes as C
import functools

import numpy as np

import cheb_cases as cc

LD = np.longdouble
U = 2.0 ** -53
SENTINEL = -7.25
GUARD_ROWS = 16                 # every block on the device is followed by this many rows of NaN (inputs) or SENTINEL (outputs)
TAIL = 64                       # ... and part, G, sumSq and dst by this many doubles of SENTINEL


# ---- the C side ------------------------------------------------------------------------------------------------------------------
class BfEigsStep(C.Structure):
    """BfEigsStep of bfhip_internal.h (tests/test_eigs_kernels_cpu.py holds it to a compiled probe)."""
    _fields_ = [("rowptr", C.c_void_p), ("colind", C.c_void_p), ("val", C.c_void_p), ("n", C.c_uint64), ("p", C.c_uint32), ("ld", C.c_uint32),
                ("b1", C.c_void_p), ("b2", C.c_void_p), ("out", C.c_void_p), ("alpha", C.c_double), ("beta", C.c_double), ("gamma", C.c_double)]


def bind(lib):
    """The launch functions' prototypes (bfhip_internal.h) on the loaded library."""
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    lib.bfdevEigsChunkRows.argtypes, lib.bfdevEigsChunkRows.restype = [u64, u32], u64
    for name, args in (("bfdevEigsStep", [C.POINTER(BfEigsStep), vp]), ("bfdevEigsGram", [vp, vp, u64, u32, vp, vp, vp]),
                       ("bfdevEigsRotate", [vp, vp, vp, u64, u32, vp]), ("bfdevEigsResidual", [vp, vp, vp, u64, u32, vp, vp, vp]),
                       ("bfdevEigsStore", [vp, u64, u32, u32, vp, vp, u64, vp])):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    return lib


def chunk_rows(n, ld):
    """bfdevEigsChunkRows restated: rows per chunk of the Gram and residual partials."""
    max_chunks = min(max((1 << 23) // (ld * ld), 64), 1024)
    rows = -(-n // max_chunks)
    return max(1024, -(-rows // 16) * 16)


def max_chunks(ld):
    return min(max((1 << 23) // (ld * ld), 64), 1024)


def chunks_of(n, ld):
    rows = chunk_rows(n, ld)
    return [(r0, min(r0 + rows, n)) for r0 in range(0, n, rows)]


CHUNK_TABLE = [((131072, 256), 1024), ((131073, 256), 1040), ((131089, 256), 1040), ((1048577, 16), 1040), ((4221, 144), 1024),
               ((1, 16), 1024), ((1024, 256), 1024), ((65536 + 1, 256), 1024), ((1 << 20, 16), 1024), ((1 << 24, 256), 131072),
               ((10 ** 6, 112), 1504), ((10 ** 6 + 1, 48), 1024)]


def tile_groups(ld):
    """The NT of bfEigsGramTiles / bfEigsRotateTiles per tile-column group of a block of ld columns."""
    tiles = ld // 16
    return [min(4, tiles - tj0) for tj0 in range(0, tiles, 4)]


def step_lanes(p):
    """(lanes per row, panels of columns) of bfdevEigsStep."""
    lg = 0
    while (1 << lg) < p and lg < 6:
        lg += 1
    return 1 << lg, -(-p // (1 << lg))


def ratio(got, ref, bound):
    """max |got - ref| / bound; inf where got is not finite or differs from ref at a bound of zero."""
    got = np.asarray(got)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got.astype(LD) - ref)
    nz = bound > 0
    if (err[~nz] != 0).any():
        return float("inf")
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def draw(rng, kind, shape):
    return rng.integers(-3, 4, size=shape).astype(np.float64) if kind == "int" else rng.standard_normal(shape)


# ---- Gram, rotation, residual ----------------------------------------------------------------------------------------------------
DENSE_LDS = (16, 48, 96, 112, 144, 256)
DENSE_NS = (1, 3, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049)
WANTED_GROUPS = {16: [1], 48: [3], 96: [4, 2], 112: [4, 3], 144: [4, 4, 1], 256: [4, 4, 4, 4]}
BIG = (131089, 256)             # chunks of 1040 rows, 127 of them, the last of 49


def dense_shapes():
    """(n, ld, p): every ld at n in {17, 1025, 2049}, every n at ld in {48, 112}; p = ld, ld - 15, ld, ld - 1 in turn."""
    out = []
    for ld in DENSE_LDS:
        for n in DENSE_NS:
            if n in (17, 1025, 2049) or ld in (48, 112):
                out.append((n, ld, (ld, ld - 15, ld, ld - 1)[len(out) % 4]))
    return out


def gram_xx_shapes():
    """One Gram(X, X) per ld, as orthonormalisation calls it: the 1025-row shape (two chunks, the second of one row)."""
    return [s for s in dense_shapes() if s[0] == 1025]


def shape_id(s):
    return "n%d-ld%d-p%d" % s


def two_prod(a, b):
    """(p, e) in float64 with a * b = p + e exactly (Veltkamp's split and Dekker's product; no fma in numpy)."""
    def split(x):
        c = 134217729.0 * x
        hi = c - (c - x)
        return hi, x - hi
    p = a * b
    (ah, al), (bh, bl) = split(a), split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def ld_mul(A, B):
    return np.ascontiguousarray(A, dtype=LD) @ np.ascontiguousarray(B, dtype=LD)


class Dense:
    """X, Y [n, ld], W [ld, ld], theta [ld] of one kind, zero outside the first p columns (W: rows too).  `live_tiles` are the
    16-column tiles that hold a column below p."""
    def __init__(self, n, ld, p, kind, operands_only=False):
        rng = np.random.default_rng([n, ld, p, int(kind == "int")])
        self.n, self.ld, self.p, self.kind = n, ld, p, kind
        self.X, self.Y = np.zeros((n, ld)), np.zeros((n, ld))
        self.X[:, :p], self.Y[:, :p] = draw(rng, kind, (n, p)), draw(rng, kind, (n, p))
        self.W, self.theta = np.zeros((ld, ld)), np.zeros(ld)
        if not operands_only:
            self.W[:p, :p], self.theta[:p] = draw(rng, kind, (p, p)), draw(rng, kind, p)
        self.live_tiles = range(-(-p // 16))

    # float64 evaluations: exact for "int" (the reference there), the yardstick of test_eigs_kernels_cpu.py for "float"
    def gram64(self, xx=False):
        return self.X.T @ (self.X if xx else self.Y) + 0.0

    def rotate64(self):
        return self.X @ self.W + 0.0

    def residual_d(self):
        """Y - X diag(theta) in long double to 2^-63 of each entry whatever cancels: theta X is split into a double and its
        exact error first (a long double product of two doubles would be rounded at 2^-64 of theta X, not of the difference)."""
        hi, lo = two_prod(self.theta, self.X)
        return (self.Y.astype(LD) - hi.astype(LD)) - lo.astype(LD)

    def residual64(self):
        """d rounded once, as the kernel's fma gives it, then squares summed in float64."""
        return (self.residual_d().astype(np.float64) ** 2).sum(axis=0)

    @functools.lru_cache(maxsize=None)
    def gram(self, xx=False):
        """(reference, bound) of G = X^T Y (xx: X^T X)."""
        Y = self.X if xx else self.Y
        if self.kind == "int":
            return self.gram64(xx).astype(LD), np.zeros((self.ld, self.ld), dtype=LD)
        return ld_mul(self.X.T, Y), (self.n + 2) * LD(U) * ld_mul(np.abs(self.X.T), np.abs(Y))

    @functools.lru_cache(maxsize=None)
    def rotate(self):
        if self.kind == "int":
            return self.rotate64().astype(LD), np.zeros((self.n, self.ld), dtype=LD)
        return ld_mul(self.X, self.W), (self.ld + 2) * LD(U) * ld_mul(np.abs(self.X), np.abs(self.W))

    @functools.lru_cache(maxsize=None)
    def residual(self):
        if self.kind == "int":
            return self.residual64().astype(LD), np.zeros(self.ld, dtype=LD)
        ref = (self.residual_d() ** 2).sum(axis=0)
        return ref, (self.n + 8) * LD(U) * ref


@functools.lru_cache(maxsize=None)
def dense(n, ld, p, kind):
    return Dense(n, ld, p, kind)


def int_worst_case(n, ld, nnz=0, scalars=(0, 0, 0)):
    """The largest absolute value any partial sum of an "int" design can take, per kernel."""
    a, b, g = (abs(s) for s in scalars)
    return dict(gram=9 * n, rotate=9 * ld, residual=(3 + 9) ** 2 * n, step=a * 9 * nnz + 3 * b + 3 * g)


# ---- store -----------------------------------------------------------------------------------------------------------------------
STORE_SHAPES = [(1, 16, 1, 1), (65, 48, 33, 40), (1025, 112, 97, 97), (70001, 256, 240, 241)]      # (n, ld, nev, ldu)
STORE_ONE_PASS = 65536 * 256            # elements the store's grid covers in one pass


def store_design(n, ld, nev, ldu):
    """(X [n, ld] normal in every column, d [n] in [0.5, 1.5))."""
    rng = np.random.default_rng([n, ld, nev, ldu])
    return rng.standard_normal((n, ld)), rng.random(n) + 0.5


# ---- step ------------------------------------------------------------------------------------------------------------------------
STEP_PS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 130, 256)       # 17: the one lane count (32) the others leave out
STEP_COLUMNWISE_PS = (3, 9, 65, 130)
STEP_MATRICES = ("mesh63", "wide_and_empty", "ladder259")
STEP_SCALARS = {"int": (2.0, -3.0, 1.0), "float": (1.7109375, -0.62, -0.3)}      # (alpha, beta, gamma)


def ladder259():
    """(rowptr, colind) of 259 rows, row i of i mod 20 nonzeros, columns increasing and distinct; the rows of one nonzero hold
    column 0 and column 258 in turn, the rows of two both."""
    n, rng = 259, np.random.default_rng(259)
    rowptr, colind = [0], []
    for i in range(n):
        k = i % 20
        cols = [(0, n - 1)[(i // 20) % 2]] if k == 1 else [0, n - 1] if k == 2 else sorted(rng.choice(n, size=k, replace=False).tolist())
        colind += cols
        rowptr.append(len(colind))
    return np.array(rowptr, dtype=np.uint64), np.array(colind, dtype=np.uint64)


class StepDesign:
    """One matrix and one kind: S in CSR, b1 and b2 [n, 256] (a launch at p columns takes the first p), the scalars, and the
    references of both forms of the launch for all 256 columns at once (column c's result does not depend on p)."""
    def __init__(self, name, kind):
        rng = np.random.default_rng([STEP_MATRICES.index(name), int(kind == "int")])
        self.name, self.kind = name, kind
        if name == "ladder259":
            self.rowptr, self.colind = ladder259()
            val = rng.standard_normal(len(self.colind))
        else:
            m = cc.catalogue()[name]
            self.rowptr, self.colind = m["rowptr"], m["colind"]
            val, _, _ = cc.fold(m["rowptr"], m["colind"], m["data"], m["mass"])
        if kind == "int":
            val = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=len(self.colind))
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.n = len(self.rowptr) - 1
        self.deg = np.diff(self.rowptr.astype(np.int64))
        self.b1, self.b2 = draw(rng, kind, (self.n, 256)), draw(rng, kind, (self.n, 256))
        self.alpha, self.beta, self.gamma = STEP_SCALARS[kind]

    def eval(self, dtype, with_b2, val=None):
        """alpha (S b1) + beta b1 [+ gamma b2] in `dtype`, row sums in CSR order."""
        ell = cc.Ell(self.rowptr, self.colind, self.val if val is None else val, dtype)
        out = dtype(self.alpha) * ell.mul(self.b1.astype(dtype)) + dtype(self.beta) * self.b1.astype(dtype)
        return out + dtype(self.gamma) * self.b2.astype(dtype) + dtype(0) if with_b2 else out + dtype(0)

    @functools.lru_cache(maxsize=None)
    def reference(self, with_b2):
        """(reference, bound), [n, 256] each."""
        if self.kind == "int":
            return self.eval(np.float64, with_b2).astype(LD), np.zeros((self.n, 256), dtype=LD)
        mag = abs(LD(self.alpha)) * cc.Ell(self.rowptr, self.colind, np.abs(self.val), LD).mul(np.abs(self.b1).astype(LD)) + abs(LD(self.beta)) * np.abs(self.b1).astype(LD)
        if with_b2:
            mag = mag + abs(LD(self.gamma)) * np.abs(self.b2).astype(LD)
        return self.eval(LD, with_b2), (self.deg[:, None] + 3) * LD(U) * mag

    def without_last_nonzero(self, row):
        val = self.val.copy()
        val[int(self.rowptr[row + 1]) - 1] = 0.0
        return val


@functools.lru_cache(maxsize=None)
def step_design(name, kind):
    return StepDesign(name, kind)
