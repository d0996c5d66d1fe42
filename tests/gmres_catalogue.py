"""Test infrastructure: designed GMRES cases that reach the edges of the device Krylov kernels (bfhip_gmres.hip,
bfGmres*Kernel) and of their driver (bfhip_gmres.c, bfGmresRun).

The kernels split each column of length n into nb = min(ceil(n / 256), 1024) row blocks of ceil(n / nb) rows
(`bfRowRange`): n < 256 and n % 256 != 0 leave a ragged last block, n = 262145 hits the cap with 257 rows per block and three
empty trailing blocks.  CGS2 reduces the dots of V_0..V_j in groups of 8 (`bfGmresDotsKernel`): caps of 1, 7, 8, 9, 16 and 17
vectors cross the group edges.  Right-hand sides reach the driver's special columns: zero, an eigenvector (GMRES converges at
its first step), x0 exact, scaled by 2^k, and 2^-600 next to 2^+600.

`names()` lists the cases without building anything; `case(name)` builds one (cached).  Every case carries what
gmres_highprec.Problem needs (the Desc the device compiles, ||A||, kappa) and an fp64 matvec for the restatement."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from butterfly_amd import helm2_structure as hs
import gmres_highprec as gh

ORTHS = ("mgs", "cgs2")
SCALE_BASES = ("dense257_k3_m17", "normal300_kappa10_m17_x0", "blockdiag65537_k2_m8")   # the 2^k equivariance test's cases
KINDS = ("zero", "eigen", "x0exact", "scaled")


def row_blocks(n):
    """(nb, rows per block, [(r0, r1)] per block) as bfRowRange splits a column of length n."""
    nb = min(max((n + 255) // 256, 1), 1024)
    per = -(-n // nb)
    return nb, per, [(min(b * per, n), min(b * per + per, n)) for b in range(nb)]


@dataclass
class Operator:
    desc: object
    vals: dict
    norm_a: float
    kappa: float
    mv64: object                 # fp64 matvec of n x k arrays
    dense: np.ndarray | None = None


@dataclass
class Case:
    name: str
    op: str                      # operator key (operators are shared between cases)
    B: np.ndarray
    X0: np.ndarray | None
    m: int
    tol: float
    kinds: tuple = ()
    zero_cols: tuple = ()        # columns whose initial residual is exactly zero
    precond: str | None = None   # None, "dense" (block inverse of the dense system) or "block_jacobi" (device-built)
    iters: int | None = None     # the number of Arnoldi steps the case must report, where it is known
    extra: dict = field(default_factory=dict)

    @property
    def n(self):
        return self.B.shape[0]


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _unitary(rng, n):
    q, r = np.linalg.qr(_crandn(rng, n, n))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def _leaf(M):
    d = hs.Desc(dtype=0)
    d.root = d.add(hs.NODE_DENSE, M.shape[0], M.shape[1])
    return d, {d.root: np.ascontiguousarray(M, dtype=np.complex128)}


def _dense_op(M, norm_a, kappa):
    d, v = _leaf(M)
    return Operator(d, v, norm_a, kappa, lambda x, M=M: M @ x, M)


@functools.lru_cache(maxsize=None)
def operator(key):
    kind, arg = key.split(":")
    if kind == "dense":                     # Q diag(sigma) W^H, sigma from 1 down to 0.1: ||A|| = 1, kappa = 10
        n = int(arg)
        rng = np.random.default_rng(100 + n)
        sig = np.geomspace(1.0, 0.1, n) if n > 1 else np.ones(1)
        M = (_unitary(rng, n) * sig) @ _unitary(rng, n).conj().T
        return _dense_op(M, 1.0, 10.0 if n > 1 else 1.0)
    if kind == "normal":                    # Q diag(lambda) Q^H, |lambda| from 1 to kappa, arguments all round the circle
        kappa = float(arg)
        n = 300
        rng = np.random.default_rng(7)
        lam = np.geomspace(1.0, kappa, n) * np.exp(1j * rng.uniform(-np.pi, np.pi, n))
        Q = _unitary(rng, n)
        op = _dense_op((Q * lam) @ Q.conj().T, kappa, kappa)
        op.extra = {"Q": Q, "lam": lam}
        return op
    if kind == "diag":                      # small Gaussian integers: every product and sum of the apply is exact
        n = int(arg)
        d = np.array([(1 + i % 4) * (1j if i % 3 == 0 else 1) for i in range(n)], dtype=np.complex128)
        return _dense_op(np.diag(d), 4.0, 4.0)
    if kind == "cI":
        n = int(arg)
        return _dense_op(3.0 * np.eye(n, dtype=np.complex128), 3.0, 1.0)
    if kind == "blockdiag":                 # random unitary 16 x 16 blocks and a ragged 1 x 1 last block: ||A|| = kappa = 1
        n = int(arg)
        rng = np.random.default_rng(n)
        nfull = n // 16
        q, r = np.linalg.qr(_crandn(rng, nfull, 16, 16))
        d = np.diagonal(r, axis1=1, axis2=2)
        blocks = q * (d / np.abs(d))[:, None, :]
        last = n - 16 * nfull
        tail = np.eye(last, dtype=np.complex128) * np.exp(2j)
        d = hs.Desc(dtype=0)
        vals, ch = {}, []
        for b in range(nfull):
            leaf = d.add(hs.NODE_DENSE, 16, 16)
            vals[leaf] = blocks[b]
            ch.append((leaf, 16 * b, 16 * b))
        if last:
            leaf = d.add(hs.NODE_DENSE, last, last)
            vals[leaf] = tail
            ch.append((leaf, 16 * nfull, 16 * nfull))
        d.root = d.add(hs.NODE_BLOCK, n, n, ch, hs.BF_TYPE_BLOCK_DIAG)
        sv = np.linalg.svd(blocks, compute_uv=False)
        smax, smin = max(sv.max(), 1.0), min(sv.min(), 1.0)

        def mv(x):
            x = np.asarray(x)
            y = np.empty_like(x)
            y[:16 * nfull] = np.einsum("bij,bjk->bik", blocks, x[:16 * nfull].reshape(nfull, 16, -1)).reshape(16 * nfull, -1)
            y[16 * nfull:] = np.exp(2j) * x[16 * nfull:]
            return y
        return Operator(d, vals, smax, smax / smin, mv)
    if kind == "bie":
        import bie
        n = int(arg)
        desc, root, vals, dense = bie.second_kind_case(n, 128)
        desc.root = root
        sv = np.linalg.svd(dense, compute_uv=False)
        return Operator(desc, vals, sv[0], sv[0] / sv[-1], lambda x, M=dense: M @ x, dense)
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def dense_block_inverse(key, nblocks=16):
    """P = blockdiag(A_bb^-1) over nblocks equal diagonal blocks of the operator's dense matrix; (P, ||P A||, kappa(P A))."""
    A = operator(key).dense
    n = A.shape[0]
    P = np.zeros_like(A)
    for i in range(nblocks):
        sl = slice(i * n // nblocks, (i + 1) * n // nblocks)
        P[sl, sl] = np.linalg.inv(A[sl, sl])
    sv = np.linalg.svd(P @ A, compute_uv=False)
    return P, sv[0], sv[0] / sv[-1]


def _specs():
    """name -> builder; nothing is computed until a case is asked for."""
    S = {}

    def add(name, fn):
        S[name] = fn

    def rand(n, k, seed):
        return _crandn(np.random.default_rng(seed), n, k)

    # dense leaves at every row-block shape near 256: n < 256, n % 256 != 0, one full block, one row over
    for n, k, m, x0 in ((1, 1, 1, False), (2, 2, 7, True), (3, 3, 8, False), (255, 8, 9, False), (256, 2, 16, True),
                        (257, 3, 17, False), (1000, 1, 8, True), (257, 8, 1, False)):
        add(f"dense{n}_k{k}_m{m}" + ("_x0" if x0 else ""),
            lambda n=n, k=k, m=m, x0=x0: Case("", f"dense:{n}", rand(n, k, n + k), rand(n, k, 3 * n) if x0 else None, m, 1e-30))

    def zero_col():
        B = rand(257, 3, 5)
        B[:, 1] = 0
        return Case("", "dense:257", B, None, 17, 1e-30, kinds=("zero",), zero_cols=(1,))
    add("dense257_zero_column", zero_col)

    def zero_col_x0():
        B = rand(256, 2, 6)
        B[:, 0] = 0
        X0 = rand(256, 2, 7)
        X0[:, 0] = 0
        return Case("", "dense:256", B, X0, 8, 1e-30, kinds=("zero",), zero_cols=(0,))
    add("dense256_zero_column_x0", zero_col_x0)

    for kexp in (-600, -300, 300, 600):
        add(f"dense257_scaled_2^{kexp}",
            lambda kexp=kexp: Case("", "dense:257", np.ldexp(rand(257, 2, 9).real, kexp) + 1j * np.ldexp(rand(257, 2, 9).imag, kexp),
                                   None, 8, 1e-30, kinds=("scaled",)))

    def mixed():
        B = rand(257, 2, 10)
        B[:, 0] = np.ldexp(B[:, 0].real, -600) + 1j * np.ldexp(B[:, 0].imag, -600)
        B[:, 1] = np.ldexp(B[:, 1].real, 600) + 1j * np.ldexp(B[:, 1].imag, 600)
        return Case("", "dense:257", B, None, 8, 1e-30, kinds=("scaled",))
    add("dense257_mixed_2^-600_2^600", mixed)

    # normal matrices of designed condition
    for kap, k, m, x0 in (("1", 3, 16, False), ("10", 2, 17, True), ("1000", 1, 16, False)):
        add(f"normal300_kappa{kap}_m{m}" + ("_x0" if x0 else ""),
            lambda kap=kap, k=k, m=m, x0=x0: Case("", f"normal:{kap}", rand(300, k, 11), rand(300, k, 12) if x0 else None, m, 1e-30))

    def eigen():                            # b = an eigenvector: the first step's estimate is at rounding level
        Q = operator("normal:10").extra["Q"]
        B = np.stack([Q[:, 5] * (1 + 1j), rand(300, 1, 13)[:, 0]], axis=1)
        return Case("", "normal:10", B, None, 20, 1e-10, kinds=("eigen",))
    add("normal300_eigenvector", eigen)

    def eigen_alone():
        Q = operator("normal:10").extra["Q"]
        return Case("", "normal:10", (Q[:, 7] * 2j)[:, None], None, 20, 1e-10, kinds=("eigen",), iters=1)
    add("normal300_eigenvector_alone", eigen_alone)

    # exact breakdown: a diagonal operator and 3 I with unit-vector right-hand sides
    def diag_breakdown():
        B = rand(257, 3, 14)
        B[:, 0] = 0
        B[5, 0] = 3
        B[:, 2] = 0
        return Case("", "diag:257", B, None, 9, 1e-30, kinds=("eigen", "zero"), zero_cols=(2,))
    add("diag257_breakdown_and_zero", diag_breakdown)

    def diag_x0_exact():
        rng = np.random.default_rng(15)
        X0 = rng.integers(-4, 5, (257, 2)) + 1j * rng.integers(-4, 5, (257, 2))
        D = np.diag(operator("diag:257").dense)
        B = rand(257, 2, 16)
        B[:, 0] = D * X0[:, 0]                                 # Gaussian integers: exact, so r0 = 0 exactly
        return Case("", "diag:257", B, X0.astype(np.complex128), 8, 1e-30, kinds=("x0exact",), zero_cols=(0,))
    add("diag257_x0_exact", diag_x0_exact)

    def ci_tol0():
        B = np.zeros((255, 2), dtype=np.complex128)
        B[0, 0] = 2
        B[7, 1] = 1j
        return Case("", "cI:255", B, None, 7, 0.0, kinds=("eigen",), iters=1)
    add("cI255_exact_breakdown_tol0", ci_tol0)
    add("cI255_random", lambda: Case("", "cI:255", rand(255, 2, 17), None, 8, 1e-10, kinds=("eigen",), iters=1))

    # block-diagonal operators: many row blocks, the nb cap
    add("blockdiag65537_k2_m8", lambda: Case("", "blockdiag:65537", rand(65537, 2, 18), None, 8, 1e-30))
    add("blockdiag262145_k1_m9", lambda: Case("", "blockdiag:262145", rand(262145, 1, 19), None, 9, 1e-30))

    # the second-kind BIE system of tests/bie.py, to convergence, plain and left-preconditioned
    add("bie2048_k2", lambda: Case("", "bie:2048", rand(2048, 2, 20), None, 80, 1e-10))
    add("bie2048_k1_x0", lambda: Case("", "bie:2048", rand(2048, 1, 21), 0.5 * rand(2048, 1, 22), 80, 1e-10))
    add("bie2048_dense_block_inverse", lambda: Case("", "bie:2048", rand(2048, 2, 23), None, 80, 1e-10, precond="dense"))
    add("bie2048_block_jacobi", lambda: Case("", "bie:2048", rand(2048, 1, 24), None, 80, 1e-10, precond="block_jacobi"))
    return S


SPECS = _specs()


def names():
    return list(SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = SPECS[name]()
    c.name = name
    return c


def problem(c, P=None):
    """gmres_highprec.Problem of a case; P: the preconditioner matrix ("dense" cases build their own; "block_jacobi" cases
    take the device's, extracted by the caller)."""
    op = operator(c.op)
    if c.precond == "dense":
        P, na, ka = dense_block_inverse(c.op)
        return gh.Problem(op.desc, op.vals, na, ka, P)
    if c.precond == "block_jacobi":
        assert P is not None
        sv = np.linalg.svd(P @ op.dense, compute_uv=False)
        return gh.Problem(op.desc, op.vals, sv[0], sv[0] / sv[-1], P)
    return gh.Problem(op.desc, op.vals, op.norm_a, op.kappa)
