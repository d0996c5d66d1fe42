"""Shared by tests/test_eigs_band_cpu.py and tests/test_gpu_eigs_band.py: the cases of the band entry
(bfhipChebCovEigsBandDevice), chains of successive bands on the matrices of tests/eigs_cases.py, and reference_band, the
algorithm in numpy float64: section 25's iteration with the block deflated against the locked vectors before every
orthonormalisation (X <- X - Q (Q^T X) twice, Q in panels of at most 256 columns one after the other, the rows summed in the
chunks of the device's partials) and min(locked lam) as one more point of the degree cap.  The truth is analytic for the grid
graph and numpy.linalg.eigh of the dense S elsewhere."""
import functools

import numpy as np

import eigs_cases as ec

TOL, MIN_GAP, MAX_REF_ITERS = ec.TOL, ec.MIN_GAP, ec.MAX_REF_ITERS
U53 = 2.0 ** -53
PANEL = 256

# (matrix, the bands' nev in order, guard (None: the default), degree (None: 20)).  Band k is deflated against all earlier ones.
#   graph4221 at (64, 13): 320 pairs in five bands, past the single call's 255, then a ragged sixth of 30: locked counts 64 ... 320,
#                          one panel up to 256, two at 320; degree 60 so that the cap with the locked eigenvalue decides.
#   graph4221 at (120, 10): p = 130 > 128, three bands.
#   two_grids: lambda = 0 twice, split across the first boundary: the first band takes one null vector, the second starts with the other.
#   path5: 2 locked, then nev = 3 = n - m without a guard: the exact branch, no filter.
#   mesh63: 8 + 8 at guard 1.        grid33: 33 + 21: the boundary at 53 pairs has a relative gap of 9.4e-6 (a nearly degenerate
#                          pair straddles it), below MIN_GAP; the one at 54 has 3.4e-3 and keeps that pair inside the band.
CHAINS = [
    ("graph4221", (64, 64, 64, 64, 64, 30), 13, 60),
    ("graph4221", (120, 120, 120), 10, 20),
    ("two_grids", (1, 16, 23), None, None),
    ("path5", (2, 3), (1, 0), None),
    ("mesh63", (8, 8), 1, 20),
    ("grid33", (33, 21), None, None),
]


def chain_id(chain):
    name, bands, guard, degree = chain
    return f"{name}-{'+'.join(str(b) for b in bands)}"


def guard_of(chain, k):
    g = chain[2]
    return g[k] if isinstance(g, tuple) else g


def block_columns(n, m, nev, guard):
    """p of a band call: section 25's rule with n - m in place of n."""
    return ec.block_columns(n - m, nev, guard)


def cross_chunk_rows(n, ld):
    """bfdevEigsCrossChunkRows restated: rows per chunk of the cross-Gram partials (chunks x mq16 x ld doubles, mq16 <= 256)."""
    max_chunks = min(max((1 << 23) // (256 * ld), 64), 1024)
    rows = -(-n // max_chunks)
    return max(1024, -(-rows // 16) * 16)


def cross_chunks_of(n, ld):
    rows = cross_chunk_rows(n, ld)
    return [(r0, min(r0 + rows, n)) for r0 in range(0, n, rows)]


def panels_of(m):
    return [(m0, min(m0 + PANEL, m)) for m0 in range(0, m, PANEL)]


# ---- the projection ------------------------------------------------------------------------------------------------------------
def project(X, Q, ld=None, skip_panel=None, skip_chunk=None, skip_last_column=False):
    """One pass X - Q (Q^T X): panel after panel, coefficients then update, the coefficients summed over the chunks of rows in
    order.  The skip_* arguments restate what a kernel could leave out (tests/test_eigs_band_cpu.py): one panel of Q, one chunk
    of rows of the coefficients, Q's last column."""
    n, m = Q.shape
    ld = -(-X.shape[1] // 16) * 16 if ld is None else ld
    X = X.copy()
    for k, (m0, m1) in enumerate(panels_of(m)):
        if k == skip_panel:
            continue
        if skip_last_column and m1 == m:
            m1 -= 1
        Qp = Q[:, m0:m1]
        C = np.zeros((m1 - m0, X.shape[1]))
        for j, (r0, r1) in enumerate(cross_chunks_of(n, ld)):
            if j != skip_chunk:
                C += Qp[r0:r1].T @ X[r0:r1]
        X -= Qp @ C
    return X


def project_twice(X, Q, passes=2, **skip):
    for _ in range(passes):
        X = project(X, Q, **skip)
    return X


def band_degree_cap(theta, lock_min, lam_max, degree):
    """ec.degree_cap with one more point: the interval and the normalisation come from the block's Ritz values alone, the ratio
    max / min of |rho_m| runs over them and over the smallest locked eigenvalue."""
    if lock_min is None:
        return ec.degree_cap(theta, lam_max, degree)
    a, a0, b = theta[-1], theta[0], lam_max
    e, c = (b - a) / 2, (b + a) / 2
    sigma1 = e / (a0 - c)
    tau, sigma = 2 / sigma1, sigma1
    pts = np.append(theta, lock_min)
    y0, y1 = np.ones_like(pts), sigma1 / e * (pts - c)
    best = 1
    for m in range(1, degree + 1):
        if m > 1:
            sn = 1 / (tau - sigma)
            y0, y1 = y1, 2 * sn / e * (pts - c) * y1 - sigma * sn * y0
            sigma = sn
        lo, hi = np.abs(y1).min(), np.abs(y1).max()
        if np.isfinite(hi) and hi < 2.0 ** 23 * lo:
            best = m
    return best


# ---- the algorithm in float64 --------------------------------------------------------------------------------------------------
def reference_band(mat, nev, Q=None, lam_locked=None, guard=None, degree=None, tol=TOL, max_iter=100, seed=0, passes=2, lock_cap=True):
    """dict(lam, U, residual, iterations, converged, max_degree, p): the band that follows the m = Q.shape[1] locked pairs.
    passes: projection passes before every orthonormalisation (2: the algorithm); lock_cap=False leaves the locked eigenvalue out
    of the degree cap (section 25's cap)."""
    n, lam_max = mat.n, mat.lam_max
    m = 0 if Q is None else Q.shape[1]
    p = block_columns(n, m, nev, guard)
    degree = 20 if degree is None else degree
    mul = mat.ell.mul
    lock_min = float(np.min(lam_locked[:m])) if m and lock_cap else None
    defl = (lambda X: project_twice(X, Q, passes)) if m else (lambda X: X)
    X = ec.normal_stream(seed, np.arange(n * p, dtype=np.uint64)).reshape(n, p)
    X, Y, theta, res = ec._rayleigh_ritz(mul, defl(X), n, p)
    its, max_degree = 0, 0
    while True:
        conv = 0
        while conv < nev and res[conv] <= tol * lam_max:
            conv += 1
        if conv == nev or its == max_iter:
            break
        if p < n - m:
            a, a0, b = theta[-1], theta[0], lam_max
            e, c = (b - a) / 2, (b + a) / 2
            sigma1 = e / (a0 - c)
            tau = 2 / sigma1
            deg = band_degree_cap(theta, lock_min, lam_max, degree)
            max_degree = max(max_degree, deg)
            prev, cur = X, sigma1 / e * (mul(X) - c * X)
            sigma = sigma1
            for _ in range(1, deg):
                sn = 1 / (tau - sigma)
                prev, cur = cur, 2 * sn / e * (mul(cur) - c * cur) - sigma * sn * prev
                sigma = sn
            X = cur
        its += 1
        X = defl(X)
        if ec._cholqr2(X, n, p) is None:
            return dict(converged=-1, iterations=its, p=p)
        X, Y, theta, res = ec._rayleigh_ritz(mul, X, n, p)
    return dict(lam=theta[:nev], U=X[:, :nev], residual=res[:nev], iterations=its, converged=conv, max_degree=max_degree, p=p)


@functools.lru_cache(maxsize=None)
def reference_chain(chain):
    """The chain run on the restatement's own bands: (lam_all, U_all, list of per-band dicts).  Computed once per process."""
    name, bands, _, degree = chain
    mat = ec.matrices()[name]
    total = sum(bands)
    U, lam, runs, m = np.zeros((mat.n, total)), np.zeros(total), [], 0
    for k, nev in enumerate(bands):
        r = reference_band(mat, nev, U[:, :m] if m else None, lam, guard_of(chain, k), degree)
        assert r["converged"] == nev, (chain_id(chain), k, r["converged"], r["iterations"])
        U[:, m:m + nev], lam[m:m + nev] = r["U"], r["lam"]
        runs.append(r)
        m += nev
    U.setflags(write=False); lam.setflags(write=False)
    return lam, U, runs


def truth_extent(lam, hi, lam_max):
    """The smallest count >= hi at which the true spectrum has a relative gap of MIN_GAP: hi itself at every boundary but the
    degenerate split of two_grids, where the band's vectors lie in the eigenspace that straddles the boundary."""
    while hi < len(lam) and (lam[hi] - lam[hi - 1]) / lam_max < MIN_GAP:
        hi += 1
    return hi


SPLIT = ("two_grids", 0)        # (matrix, band) whose upper boundary cuts the double eigenvalue 0


def orthonormality(U):
    return float(np.abs(U.T @ U - np.eye(U.shape[1])).max())


# ---- the two deflation kernels, launched alone (tests/test_gpu_eigs_band_kernels.py) -----------------------------------------
# Designs as in tests/eigs_kernel_cases.py: "int" entries in [-3, 3] (every partial sum an exact integer far below 2^53: bit for
# bit against numpy) and "float" standard normals against numpy.longdouble under componentwise bounds, u = 2^-53:
#     cross-Gram  |C - ref|_kj <= (n + 2) u (|Q|^T |X|)_kj          deflation  |out - ref|_ij <= (mq + 3) u (|X| + |Q| |C|)_ij
# Q lies in a flat buffer as the caller's layout allows: element (r, k) of the panel at base + r ldq + m0 + k, k < mq; everything
# else in the buffer is NaN (a column at or past mq that is read shows).  ldq kinds: mq, mq + 1, mq + 3 (rows overlap the offset:
# legal, the panel is what the kernel may read) and a multiple of 4 that holds m0 + mq; base offsets of 0 or 1 doubles, so that
# the deflation's 32-byte A-operand path (base + m0 32-byte aligned and ldq % 4 == 0) and its scalar path both run.
import eigs_kernel_cases as ek     # noqa: E402

K_MQS = (1, 15, 16, 17, 64, 100, 255, 256)
K_LDS = (16, 48, 112, 256)
K_NS = (1, 3, 15, 16, 17, 1023, 1024, 1025, 2049)
K_M0S = (0, 1, 4, 255)
WALK_MS = (257, 300)


def kernel_shapes():
    """(n, mq, ld, p, ldq, m0, base): every n twice, every mq at n = 17 and 1025, then the corners named below."""
    combos = []
    for k, n in enumerate(K_NS):
        combos += [(n, K_MQS[k % 8], K_LDS[k % 4]), (n, K_MQS[(k + 3) % 8], K_LDS[(k + 1) % 4])]
    for k, mq in enumerate(K_MQS):
        combos += [(1025, mq, K_LDS[(k + 2) % 4]), (17, mq, K_LDS[(k + 3) % 4])]
    combos += [(1025, 256, 256), (2049, 100, 112)]                 # two chunks at the widest block; three chunks, <4>,<3>
    out = []
    for i, (n, mq, ld) in enumerate(dict.fromkeys(combos)):
        p = ld if i % 2 == 0 else (ld - 15, ld - 1)[(i // 2) % 2]
        m0 = K_M0S[(3 * i + i // 4) % 4]
        ldq = (mq, mq + 1, mq + 3, -(-(m0 + mq) // 4) * 4 + 4)[i % 4]
        out.append((n, mq, ld, p, ldq, m0, (i // 8) % 2))
    # the vector path with a ragged last quad, and the same panel one double further on (8-byte alignment only)
    out += [(1025, 17, 48, 33, 24, 4, 0), (1025, 17, 48, 33, 24, 4, 1), (65, 255, 16, 16, 260, 0, 0), (17, 15, 112, 97, 16, 0, 0), (33, 100, 48, 48, 360, 255, 1)]
    return out


def kshape_id(s):
    return "n%d-mq%d-ld%d-p%d-ldq%d-m0_%d-b%d" % s


def vector_path(s):
    """True when bfdevEigsDeflate takes the 32-byte A-operand path (the buffer itself starts on a 32-byte boundary)."""
    n, mq, ld, p, ldq, m0, base = s
    return (base + m0) % 4 == 0 and ldq % 4 == 0


class BandDesign:
    """Q [n, mq], X [n, ld] (columns from p on zero), C [mq16, ld] (rows from mq on and columns from p on zero) of one kind."""
    def __init__(self, shape, kind):
        n, mq, ld, p, ldq, m0, base = shape
        rng = np.random.default_rng([n, mq, ld, p, int(kind == "int")])
        self.shape, self.kind, self.mq16 = shape, kind, -(-mq // 16) * 16
        self.Q = ek.draw(rng, kind, (n, mq))
        self.X, self.C = np.zeros((n, ld)), np.zeros((self.mq16, ld))
        self.X[:, :p], self.C[:mq, :p] = ek.draw(rng, kind, (n, p)), ek.draw(rng, kind, (mq, p))

    def flat_q(self):
        """(buffer, offset of element (0, 0) of the panel): NaN wherever the panel is not."""
        n, mq, ld, p, ldq, m0, base = self.shape
        size = base + (n - 1) * ldq + m0 + mq
        buf = np.full(size + ek.GUARD_ROWS * max(ldq, 1), np.nan)
        idx = base + m0 + np.arange(n)[:, None] * ldq + np.arange(mq)[None, :]
        buf[idx] = self.Q
        return buf, base

    @functools.lru_cache(maxsize=None)
    def cross(self):
        """(reference, bound) of C = Q^T X, [mq16, ld]."""
        n, mq = self.shape[0], self.shape[1]
        ref, bound = np.zeros((self.mq16, self.X.shape[1]), dtype=ek.LD), np.zeros((self.mq16, self.X.shape[1]), dtype=ek.LD)
        if self.kind == "int":
            ref[:mq] = self.Q.T @ self.X + 0.0
        else:
            ref[:mq] = ek.ld_mul(self.Q.T, self.X)
            bound[:mq] = (n + 2) * ek.LD(ek.U) * ek.ld_mul(np.abs(self.Q.T), np.abs(self.X))
        return ref, bound

    @functools.lru_cache(maxsize=None)
    def deflate(self):
        """(reference, bound) of X - Q C, [n, ld]."""
        mq = self.shape[1]
        if self.kind == "int":
            return (self.X - self.Q @ self.C[:mq] + 0.0).astype(ek.LD), np.zeros(self.X.shape, dtype=ek.LD)
        return (self.X.astype(ek.LD) - ek.ld_mul(self.Q, self.C[:mq]),
                (mq + 3) * ek.LD(ek.U) * (np.abs(self.X).astype(ek.LD) + ek.ld_mul(np.abs(self.Q), np.abs(self.C[:mq]))))


@functools.lru_cache(maxsize=None)
def band_design(shape, kind):
    return BandDesign(shape, kind)


def bind(lib):
    """The new launch functions' prototypes (bfhip_internal.h) on the loaded library."""
    import ctypes as C
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    lib.bfdevEigsCrossChunkRows.argtypes, lib.bfdevEigsCrossChunkRows.restype = [u64, u32], u64
    for name, args in (("bfdevEigsCrossGram", [vp, u64, u64, u32, vp, u64, u32, vp, vp, vp]), ("bfdevEigsDeflate", [vp, u64, u64, u32, vp, vp, u64, u32, vp]),
                       ("bfdevEigsProject", [vp, u64, u64, vp, u64, u32, vp, vp, vp])):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    return lib
