"""Test infrastructure: designed cases for the mixed-precision GMRES refinement (bfhip_refine.c; in bfhip_gmres.hip
bfRefineDemote/Promote/Scale/UpdateKernel and, through the true residual, bfGmresResidual/ScaleKernel).

The operators are tests/gmres_catalogue.py's (`operator(key)`: designed ||A|| and kappa).  The system operator is the complex128
compile of `desc`/`vals`, the inner one the demote_to_f32 compile of the same (or, for the two stagnation cases, of `low`, a
different matrix of the same size).

Every case has tol 1e-12, the default inner tolerance and max_outer 10.  The spectra of these operators surround the origin, so
GMRES needs close to n vectors whatever kappa is: the cases that are to converge allow FULL = 304 inner vectors (n <= 300), and
with them each outer step gains about six digits.  dense:1000 and the block-diagonal operators (whose spectrum covers the unit
circle) would need far longer bases: their cases take the exact inverse as the inner left preconditioner, so that the row-block
shapes (`gmres_catalogue.row_blocks`) are held to convergence too.  `blockdiag65537_k2` without it stagnates at its first step.

`converges` marks the cases whose restatement reaches tol (tests/test_refine_highprec_cpu.py confirms each); the others are
held to the invariants of tests/refine_highprec.py only, never to a count.  The one-element-per-thread kernels run
n * nrhs elements: 1, 4, 9 and 2040 (below 256 or no multiple of it), 512 (a multiple), 262145 = 1024 * 256 + 1 (one over)."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import gmres_catalogue as cat
import gmres_highprec as gh

ORTHS = cat.ORTHS
SCALE_EXPONENTS = (-600, -300, 300, 600)
FULL = 304                   # inner vectors that span the whole space of the n <= 300 operators
SCALE_BASES = ("dense257_k2", "normal300_k2", "blockdiag65537_k2")      # the 2^k equivariance test's cases (no x0)

# (outer, inner) counts of the restatement (`restated`) on the cases that converge; tests/test_refine_highprec_cpu.py holds the
# restatement to them, the GPU tests allow the device one outer step more (as tests/test_gpu_gmres_refine.py does)
RESTATED = {
    "dense1_k1": (2, 2), "dense2_k2": (2, 4), "dense3_k3": (2, 6), "dense255_k8": (2, 510), "dense1000_k1_inv": (2, 2), "blockdiag65537_k2_inv": (2, 2), "dense256_k2": (2, 512), "dense257_k3": (2, 514),
    "dense257_k3_x0": (2, 514), "diag257_x0_exact": (2, 16), "dense256_zero_b_x0": (2, 512), "dense257_zero_first": (2, 514),
    "dense257_zero_middle": (2, 514), "dense257_zero_last": (2, 514), "dense257_k2": (2, 514), "dense257_scaled_2^-600": (2, 514),
    "dense257_scaled_2^-300": (2, 514), "dense257_scaled_2^300": (2, 514), "dense257_scaled_2^600": (2, 514),
    "dense257_mixed_2^-600_2^600": (2, 514), "normal300_k2": (2, 600), "normal300_eigenvector_and_random": (2, 600),
    "diag257_unit_vector_and_random": (2, 16), "normal300_precond_c128": (3, 834), "normal300_precond_c64": (3, 834),
}

# history[1] of the restatement where the inner operator is another matrix and the first step is the last.  The device's X_1 is
# not returned when it is worse than x0, so its history[1] is held to this figure: both solve A_low d = r^ to inner_tol, their
# corrections differ by at most 2 inner_tol ||A_low^-1|| and the residuals by ||A|| times that (`history1_tolerance`)
HISTORY1 = {"normal300_wrong_inner_operator": 0.8226892675942502, "normal300_unrelated_inner_operator": 21.43397506767038}


@dataclass
class Case:
    name: str
    op: str                      # gmres_catalogue operator key of the system
    B: np.ndarray
    X0: np.ndarray | None = None
    low: str | None = None       # operator key of the inner operator, where it is not the system's
    tol: float = 1e-12
    inner_tol: float = 0.0       # 0: the library default, refine_ref.INNER_TOL_DEFAULT
    max_outer: int = 10
    max_inner: int = 100
    precond: str | None = None   # None; "c128" or "c64": gmres_catalogue.dense_block_inverse(op) compiled as such; "inverse": the
                                 # exact inverse (complex128)
    zero_cols: tuple = ()        # columns whose initial residual is exactly zero
    converges: bool = True
    slow: bool = False           # the plan emulator needs too long: left to the GPU; there one orthogonalisation, no re-runs

    @property
    def n(self):
        return self.B.shape[0]

    @property
    def low_key(self):
        return self.low or self.op


def ldexp(Z, k):
    return np.ldexp(Z.real, k) + 1j * np.ldexp(Z.imag, k)


def _rand(n, k, seed):
    return cat._crandn(np.random.default_rng(seed), n, k)


def _specs():
    S = {}

    def add(name, fn):
        S[name] = fn

    # row-block shapes: n < 256, n % 256 != 0, one full block, one row over, and the many-block operators
    for n, k in ((1, 1), (2, 2), (3, 3), (255, 8), (256, 2), (257, 3)):
        add(f"dense{n}_k{k}", lambda n=n, k=k: Case("", f"dense:{n}", _rand(n, k, 1000 + n + k), max_inner=FULL))
    # the shapes of many row blocks converge with the exact inverse as the inner preconditioner: a wrong scale, update, demote or
    # promote at nb = 4, 257 (ragged) or 1024 (empty blocks) then misses tol, which no check could see on a stagnating solve
    add("dense1000_k1_inv", lambda: Case("", "dense:1000", _rand(1000, 1, 2001), max_inner=16, precond="inverse"))
    add("blockdiag65537_k2_inv", lambda: Case("", "blockdiag:65537", _rand(65537, 2, 18), max_inner=8, precond="inverse"))
    add("blockdiag262145_k1_inv", lambda: Case("", "blockdiag:262145", _rand(262145, 1, 19), max_inner=8, precond="inverse", slow=True))
    add("blockdiag65537_k2", lambda: Case("", "blockdiag:65537", _rand(65537, 2, 18), max_inner=8, converges=False))

    # x0: random; exact in one column; x0 != 0 under b_p = 0 (the residual is then ||A x_p||, not a ratio)
    add("dense257_k3_x0", lambda: Case("", "dense:257", _rand(257, 3, 31), _rand(257, 3, 32), max_inner=FULL))

    def diag_x0_exact():
        c = cat.case("diag257_x0_exact")                      # Gaussian integers: r0 = 0 exactly in column 0, column 1 random
        return Case("", c.op, c.B, c.X0, zero_cols=(0,))
    add("diag257_x0_exact", diag_x0_exact)

    def zero_b_x0():
        B = _rand(256, 2, 33)
        B[:, 0] = 0
        return Case("", "dense:256", B, _rand(256, 2, 34), max_inner=FULL)
    add("dense256_zero_b_x0", zero_b_x0)

    # a zero column of b among live ones
    for p, where in enumerate(("first", "middle", "last")):
        def zero(p=p):
            B = _rand(257, 3, 40 + p)
            B[:, p] = 0
            return Case("", "dense:257", B, zero_cols=(p,), max_inner=FULL)
        add(f"dense257_zero_{where}", zero)

    # b scaled by 2^k, and 2^-600 next to 2^+600
    add("dense257_k2", lambda: Case("", "dense:257", _rand(257, 2, 9), max_inner=FULL))
    for k in SCALE_EXPONENTS:
        add(f"dense257_scaled_2^{k}", lambda k=k: Case("", "dense:257", ldexp(_rand(257, 2, 9), k), max_inner=FULL))

    def mixed():
        B = _rand(257, 2, 9)
        B[:, 0], B[:, 1] = ldexp(B[:, 0], -600), ldexp(B[:, 1], 600)
        return Case("", "dense:257", B, max_inner=FULL)
    add("dense257_mixed_2^-600_2^600", mixed)

    # uneven columns: an eigenvector (its correction is one Krylov vector, though the complex64 operator leaves it as far from
    # done after one step as the random column beside it), and a unit vector on a diagonal operator, which one step finishes
    add("normal300_k2", lambda: Case("", "normal:10", _rand(300, 2, 11), max_inner=FULL))

    def uneven():
        Q = cat.operator("normal:10").extra["Q"]
        return Case("", "normal:10", np.stack([Q[:, 5] * (1 + 1j), _rand(300, 1, 13)[:, 0]], axis=1), max_inner=FULL)
    add("normal300_eigenvector_and_random", uneven)

    def unit_vector():                         # b_0 = 3 e_5 on the diagonal operator: e_5 and A e_5 are exact in complex64, so
        B = _rand(257, 2, 14)                   # column 0 is done after the first step while column 1 needs the second
        B[:, 0] = 0
        B[5, 0] = 3
        return Case("", "diag:257", B)
    add("diag257_unit_vector_and_random", unit_vector)

    # a capped inner solve: more outer steps, or stagnation
    for m in (1, 3):
        add(f"dense257_max_inner{m}", lambda m=m: Case("", "dense:257", _rand(257, 2, 50 + m), max_inner=m, converges=False))

    # the inner operator is another matrix: a step makes things worse and the best iterate must come back
    # (normal:1000 shares its eigenvectors and phases with normal:10: its steps still gain a little and stop at the first
    # that does not halve; the unrelated dense:300 makes the first step worse than x0)
    add("normal300_wrong_inner_operator", lambda: Case("", "normal:10", _rand(300, 2, 60), low="normal:1000", max_inner=FULL, converges=False))
    add("normal300_unrelated_inner_operator", lambda: Case("", "normal:10", _rand(300, 2, 61), low="dense:300", max_inner=FULL, converges=False))

    # inner left preconditioner, complex128 and complex64
    for kind in ("c128", "c64"):
        add(f"normal300_precond_{kind}", lambda kind=kind: Case("", "normal:10", _rand(300, 2, 70), precond=kind, max_inner=FULL))
    return S


SPECS = _specs()


def names():
    return list(SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = SPECS[name]()
    c.name = name
    return c


def problem(c):
    """The plain problem A x = b in long double: refinement reports true, unpreconditioned residuals."""
    return _problem(c.op)


@functools.lru_cache(maxsize=None)
def _problem(key):
    op = cat.operator(key)
    return gh.Problem(op.desc, op.vals, op.norm_a, op.kappa)


def history1_tolerance(c):
    import refine_ref
    a, low = cat.operator(c.op), cat.operator(c.low_key)
    return 2 * (c.inner_tol or refine_ref.INNER_TOL_DEFAULT) * a.norm_a * low.kappa / low.norm_a


def precond_desc(key, kind="c128", nblocks=16):
    """(desc, vals, apply) of a case's inner preconditioner as a tree of dense leaves, `apply` its fp64 action.  "inverse": the
    exact inverse (one dense leaf, or the conjugate transposes of the unitary blocks); else
    gmres_catalogue.dense_block_inverse(key)."""
    from butterfly_amd import helm2_structure as hs
    op = cat.operator(key)
    d = hs.Desc(dtype=0)
    if kind == "inverse" and op.dense is not None:
        P = np.linalg.inv(op.dense)
        d.root = d.add(hs.NODE_DENSE, *P.shape)
        return d, {d.root: np.ascontiguousarray(P)}, (lambda v: P @ v)
    if kind == "inverse":
        blocks = [np.ascontiguousarray(np.linalg.inv(op.vals[k])) for k in sorted(op.vals)]
    else:
        P = cat.dense_block_inverse(key, nblocks)[0]
        n = P.shape[0]
        blocks = [np.ascontiguousarray(P[i * n // nblocks:(i + 1) * n // nblocks, i * n // nblocks:(i + 1) * n // nblocks])
                  for i in range(nblocks)]
    pv, ch, r0 = {}, [], 0
    for blk in blocks:
        leaf = d.add(hs.NODE_DENSE, *blk.shape)
        pv[leaf] = blk
        ch.append((leaf, r0, r0))
        r0 += blk.shape[0]
    d.root = d.add(hs.NODE_BLOCK, r0, r0, ch, hs.BF_TYPE_BLOCK_DIAG)

    def apply(v):
        out, r = np.empty_like(v), 0
        lead = next((i for i, b in enumerate(blocks) if b.shape != blocks[0].shape), len(blocks))
        same = blocks[:lead]                                   # the leading run of equal blocks in one einsum, the rest one by one
        m = blocks[0].shape[0]
        out[:m * len(same)] = np.einsum("bij,bjk->bik", np.stack(same), v[:m * len(same)].reshape(len(same), m, -1)).reshape(m * len(same), -1)
        r = m * len(same)
        for b in blocks[len(same):]:
            out[r:r + b.shape[0]] = b @ v[r:r + b.shape[0]]
            r += b.shape[0]
        return out
    return d, pv, apply


# ---- the restatement (tests/refine_ref.py) of a case, without a GPU: the plan emulator's complex64 model of the plan-only
# compile of the inner operator (and of a complex64 preconditioner), the fp64 matvec as the system
@functools.lru_cache(maxsize=None)
def _low_model(key):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    import refine_ref
    op = cat.operator(key)
    low = HipOperator.from_desc(op.desc, op.vals, flags=_capi.FLAG_PLAN_ONLY, max_rhs=8, demote_to_f32=True)
    return refine_ref.c64_model(low), low          # the operator is kept alive with its model


@functools.lru_cache(maxsize=None)
def _msolve(key, kind):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    import refine_ref
    d, pv, apply = precond_desc(key, kind)
    if kind != "c64":
        return apply, None
    pre = HipOperator.from_desc(d, pv, flags=_capi.FLAG_PLAN_ONLY, max_rhs=8, demote_to_f32=True)
    return refine_ref.c64_model(pre), pre


def low_model(key):
    return _low_model(key)[0]


def restated(c, **kw):
    """((X, num_outer, num_inner, residual, history), [X_1..X_k]) of refine_ref.solve_refine on case c; **kw: its mutants."""
    import refine_ref
    msolve = _msolve(c.op, c.precond)[0] if c.precond else None
    with np.errstate(all="ignore"):
        X, k, inner, hist, its = refine_ref.solve_refine(cat.operator(c.op).mv64, low_model(c.low_key), c.B, X0=c.X0, tol=c.tol,
                                                         inner_tol=c.inner_tol or refine_ref.INNER_TOL_DEFAULT, max_outer=c.max_outer,
                                                         max_inner=c.max_inner, msolve=msolve, return_iterates=True, **kw)
    return (X, k, inner, min(hist) if kw.get("keep_best", True) else hist[-1], hist), its


@functools.lru_cache(maxsize=None)
def solution(name):
    import refine_highprec as rh
    c = case(name)
    return rh.solution(problem(c), cat.operator(c.op), c.B)
