"""Designed cases for the conditioning kernels (bfhip_cond.hip, bfhip_condlik.hip; DESIGN.md sections 20 and 21) at the
shapes the first tests leave out: more than one chunk of BF_COND_CHUNK = 1024 columns, more than one workgroup of the Cholesky
panel kernel (k >= 161), k past 256 and 512, cond(K) up to 1e10, and the documented maximum k = 2048.  Builders only: numpy
(and the CPU oracle for the dense form of a random graph), no GPU.  tests/test_cov_cond_cases_cpu.py asserts what each builder
claims; tests/test_gpu_cov_cond_shapes.py holds the device to the references built here.

A. chunk_operands(): three operands whose n spans 3, exactly 1 and 1 + one row chunks.  chunk_sensitivity() is the condition
   every such case has to meet on the reference alone: leaving one chunk out of G, or out of B^T W, moves alpha by at least
   1e3 tolerances, so a kernel that drops or misplaces a chunk cannot pass.
B. spectrum_case(): Phi = U diag(s) V^T, gamma = 1, noiseVar = delta: K = P U diag(s^2 + delta) U^T P^T has the spectrum that was
   asked for, log-spaced from 1 down to 1 / kappa.  host_float64() is the same operation in plain float64, the yardstick of the
   device's forward error.
C. integer_case(): Phi = L0 = 2 I + three entries of +-1 per row within 40 columns left of the diagonal, observed in row order.
   G = L0 L0^T has integer entries <= 7 and L0 is its Cholesky factor: every product, root and quotient of the Gram kernel, the
   factorization and both substitutions is exact in double in any order of summation, so the device has to return the integers
   that went in, bit for bit."""
import numpy as np

import randgraph
from butterfly_amd.helm2_structure import NODE_DENSE, Desc
from test_cov_likelihood_cpu import LikReference
from test_gpu_cov_condition import LD, Oracle, Reference, cholesky_ld, col_errs, input_of, permute_rows, solve_ld, tol_of

CHUNK = 1024                       # BF_COND_CHUNK (bfhip_operator.h)
RHO = 0.01
A_KS, A_QS, NQUERY = (33, 130), (1, 70), 70
GRAPH_CHUNK_NORMS = (8.80, 8.78, 1.69)
ONE_ROW_GAMMA = 8.0                # gamma[1024] of the n = 1025 operand, see chunk_operands()
SPECTRUM_CASES = ((161, 200, 1e10), (300, 333, 1e6), (513, 1100, 1e2), (513, 1100, 1e10))     # (k, n, kappa)
INTEGER_KS = (97, 2048)


def dense_leaf(phi):
    """A one-leaf operand: the adjoint apply of a unit column to it is exact, so the device's B is the observed rows of phi."""
    d = Desc(dtype=1)
    node = d.add(NODE_DENSE, phi.shape[0], phi.shape[1])
    d.root = node
    return d, {node: np.ascontiguousarray(phi, dtype=np.float64)}


def chunk_slices(n):
    return [slice(j0, min(j0 + CHUNK, n)) for j0 in range(0, n, CHUNK)]


def inverse_perm(perm):
    rev = np.empty(len(perm), dtype=np.int64); rev[perm] = np.arange(len(perm))
    return rev


# ---------------------------------------------------------------------------
# A. more than one chunk of n
# ---------------------------------------------------------------------------
class ChunkOperand:
    """One operand of part A with its weights, permutation and W block; refs[demote, k] are built on demand, once."""
    def __init__(self, name, desc, vals, gam, seed, demotes, blocks):
        from oracle import bfref
        self.name, self.desc, self.vals, self.demotes, self.blocks = name, desc, vals, demotes, blocks
        self.m, self.n = desc.rows[desc.root], desc.cols[desc.root]
        self.A = bfref.from_desc(desc, vals)
        rng = np.random.default_rng(seed)
        self.gam = gam
        self.row_perm = rng.permutation(self.m)
        self.rev = inverse_perm(self.row_perm)
        self.W = rng.standard_normal((self.n, max(A_QS)))
        self.phi = Oracle(self.A, self.gam, self.row_perm).rapply(np.eye(self.m)).T.copy()      # dense Phi [m x n], from the oracle
        self._cases = {}

    def oracle(self, demote):
        return Oracle(self.A, input_of(self.gam, demote), self.row_perm)

    def rows(self, demote):
        """P Phi Gamma in long double, [m x n]: row o is r_o."""
        return permute_rows(self.phi.astype(LD) * input_of(self.gam, demote).astype(LD), self.row_perm)

    def case(self, demote, k):
        """(Reference, LikReference, 70 query indices) of k observations: noise, y and E as in tests/test_gpu_cov_condition.py."""
        if (demote, k) not in self._cases:
            krng = np.random.default_rng(1000 + k)
            obs = krng.choice(self.m, size=k, replace=False)
            ref = Reference(self.phi[self.rev[obs], :].T, input_of(self.gam, demote), obs, RHO, krng, phi=self.phi, row_perm=self.row_perm)
            ref.y = np.asarray(ref.Bt.T @ krng.standard_normal(self.n) + np.sqrt(ref.noise) * krng.standard_normal(k), dtype=np.float64)
            ref.E = np.sqrt(ref.noise)[:, None] * krng.standard_normal((k, max(A_QS)))
            ref.lam_min = float(np.linalg.eigvalsh(ref.A.astype(np.float64))[0])
            rest = np.setdiff1d(np.arange(self.m), obs[:8])
            query = np.concatenate([obs[:8], krng.permutation(rest)])[:NQUERY]          # 8 observed points lead; at k = 130 most of the rest are observed too
            self._cases[demote, k] = ref, LikReference(ref.Bt, ref.noise, ref.y), query
        return self._cases[demote, k]


def chunk_operands():
    """The three operands of part A, by name.
    graph:    the random graph of seed 79, 157 x 2085: chunks of 1024, 1024 and 37 columns; F64 and F32, block switches off and on.
              The last chunk holds 1.69^2 / (8.80^2 + 8.78^2 + 1.69^2) = 1.8 % of ||Phi||_F^2: with gamma in [0.1, 1.1) throughout,
              leaving it out of G moves alpha by 1.9e-2 at k = 33, short of the 2e-2 that F32 (tolerance 2e-5) needs.  gamma is
              therefore tripled on the last chunk, which gives it nine times the share.
    one:      a dense leaf, 140 x 1024, entries N(0, 1 / n): exactly one chunk, the j0 + CHUNK < n edge.
    one_row:  a dense leaf, 140 x 1025: the second chunk is the single column 1024.  With gamma in [0.1, 1.1) the first chunk gives G
              a diagonal of about sum_j gamma_j^2 / n = 0.44; gamma[1024] = 8 makes the last column's rank-one term 64 / 1025 z z^T =
              0.06 z z^T (z the N(0, 1) draws of that column), a seventh of that, and its share of B^T W of the same order."""
    desc, vals = randgraph.random_operand(np.random.default_rng(79), depth=4, size_hint=120, cplx=False, m=157, n=2085)
    gam = np.random.default_rng(7901).random(2085) + 0.1
    gam[2 * CHUNK:] *= 3.0
    ops = {"graph": ChunkOperand("graph", desc, vals, gam, 7900, (False, True), (False, True))}
    for name, n in (("one", 1024), ("one_row", 1025)):
        rng = np.random.default_rng(8000 + n)
        desc, vals = dense_leaf(rng.standard_normal((140, n)) / np.sqrt(n))
        gam = rng.random(n) + 0.1
        if n > CHUNK:
            gam[CHUNK] = ONE_ROW_GAMMA
        ops[name] = ChunkOperand(name, desc, vals, gam, 8100 + n, (False,), (False,))
    return ops


def chunk_sensitivity(ref, W, E):
    """{(chunk, "G" | "BtW"): the smallest relative l2 change, over the columns, of the reference alpha when that chunk's rows of Bt
    are left out of G = Bt^T Bt, or out of Bt^T W}.  Long double throughout; G + D stays positive definite without a chunk."""
    R = ref.residual(ref.y, W, E)
    alpha = solve_ld(ref.L, R)
    out = {}
    for c, sl in enumerate(chunk_slices(ref.Bt.shape[0])):
        Bc = ref.Bt[sl]
        out[c, "G"] = float(col_errs(solve_ld(cholesky_ld(ref.A - Bc.T @ Bc), R), alpha).min())
        out[c, "BtW"] = float(col_errs(solve_ld(ref.L, R + Bc.T @ W[sl].astype(LD)), alpha).min())
    return out


def assert_every_chunk_matters(op, demote, k, q):
    """The condition of part A, on the reference alone: every chunk, left out of either sum, moves every column of alpha by at
    least 1e3 times the tolerance the device is held to."""
    ref, _, _ = op.case(demote, k)
    need = 1e3 * tol_of(demote)
    sens = chunk_sensitivity(ref, input_of(op.W[:, :q], demote), ref.E[:, :q])
    print(f"{op.name} demote={demote} k={k} q={q}: cond(G + D) = {ref.kappa:.3e}; alpha moves by at least "
          + ", ".join(f"{what}[{c}] {v:.2e}" for (c, what), v in sens.items()) + f" (needed {need:.0e})")
    assert ref.kappa <= ref.kappa_bound
    assert len(sens) == 2 * ((op.n + CHUNK - 1) // CHUNK)
    assert min(sens.values()) >= need
    return sens


def variance_reference(rows, ref, query):
    """(prior, posterior) variances at the output indices `query` in long double: p = ||r||^2, v = p - ||L^-1 Bt^T r||^2."""
    from test_cov_likelihood_cpu import forward_ld
    r = rows[query, :]
    p = (r ** 2).sum(axis=1)
    return p, p - (forward_ld(ref.L, ref.Bt.T @ r.T) ** 2).sum(axis=0)


# ---------------------------------------------------------------------------
# B. designed spectra
# ---------------------------------------------------------------------------
class SpectrumReference(Reference):
    """tests/test_gpu_cov_condition.py's Reference with the noise given, not drawn: Bt [n x k] (gamma = 1), noiseVar = delta."""
    def __init__(self, Bt, delta, obs, phi, row_perm, y):
        k = len(obs)
        self.k, self.obs, self.y = k, obs, y
        self.Bt = Bt.astype(LD)
        self.noise = np.full(k, delta, dtype=np.float64)
        self.lik = LikReference(self.Bt, self.noise, y)                  # the one long-double factorization of the case
        self.A, self.L = self.lik.K, self.lik.L
        ev = np.linalg.eigvalsh(self.A.astype(np.float64))
        self.lam_min, self.lam_max = float(ev[0]), float(ev[-1])
        self.kappa = self.lam_max / self.lam_min
        self.phi, self.gam, self.row_perm = phi, np.ones(phi.shape[1]), row_perm


def haar(rng, n, k):
    """n x k with orthonormal columns, Haar distributed: Q of a Gaussian matrix with the signs of R's diagonal made positive."""
    q, r = np.linalg.qr(rng.standard_normal((n, k)))
    return q * np.sign(np.diag(r))


def solve_f64(l, r):
    """(L L^T)^-1 R in plain float64: forward, then backward substitution, row by row."""
    k = l.shape[0]
    x = np.array(r, dtype=np.float64)
    for c in range(k):
        x[c] = (x[c] - l[c, :c] @ x[:c]) / l[c, c]
    for c in range(k - 1, -1, -1):
        x[c] = (x[c] - l[c + 1:, c] @ x[c + 1:]) / l[c, c]
    return x


def host_float64(Bt, noise, y, W, E):
    """What the device computes, in plain float64 on the host: (alpha [k x q], (logLik, quad, logDet))."""
    Bt = np.asarray(Bt, dtype=np.float64)
    k = Bt.shape[1]
    l = np.linalg.cholesky(Bt.T @ Bt + np.diag(noise))
    alpha = solve_f64(l, y[:, None] - Bt.T @ W - E)
    quad = float(y @ solve_f64(l, y))
    logdet = float(2 * np.log(np.diag(l)).sum())
    return alpha, np.array([-quad / 2 - logdet / 2 - k / 2 * np.log(2 * np.pi), quad, logdet])


class SpectrumCase:
    """m = k rows, all observed in a random order through a random row permutation; the eigenvalues of K = G + delta I are
    lam[i] = kappa^(-i / (k - 1)) by design, delta = 1 / (2 kappa), s_i^2 = lam[i] - delta.  q = 3 columns: y, W and E are all
    N(0, 1), so the residual block y 1^T - B W - E is N(0, 1)-sized data through both chunks of n."""
    def __init__(self, k, n, kappa, with_reference=True):
        rng = np.random.default_rng([k, n, int(round(np.log10(kappa)))])
        self.k, self.n, self.kappa, self.q = k, n, kappa, 3
        self.lam = kappa ** (-np.arange(k) / (k - 1.0))
        self.delta = 0.5 / kappa
        self.phi = (haar(rng, k, k) * np.sqrt(self.lam - self.delta)) @ haar(rng, n, k).T          # [k x n], rounded to double
        self.row_perm = rng.permutation(k)
        self.obs = rng.permutation(k)
        self.y, self.W, self.E = rng.standard_normal(k), rng.standard_normal((n, self.q)), rng.standard_normal((k, self.q))
        self.Bt = np.ascontiguousarray(self.phi[inverse_perm(self.row_perm)[self.obs], :].T)       # [n x k]: column a is the row observed as obs[a]
        if with_reference:
            self.ref = SpectrumReference(self.Bt, self.delta, self.obs, self.phi, self.row_perm, self.y)
            self.alpha, _ = self.ref.posterior(self.y, self.W, self.E)
            self.values = np.array([self.ref.lik.loglik, self.ref.lik.quad, self.ref.lik.logdet], dtype=LD)
            self.alpha64, self.values64 = host_float64(self.Bt, self.ref.noise, self.y, self.W, self.E)

    def measured_kappa(self):
        """cond(K) of the matrix the reference factors: K formed in long double from the rounded Phi, eigenvalues in float64."""
        Bt = self.Bt.astype(LD)
        ev = np.linalg.eigvalsh((Bt.T @ Bt + self.delta * np.eye(self.k, dtype=LD)).astype(np.float64))
        return float(ev[-1] / ev[0])


# ---------------------------------------------------------------------------
# C. exact integers at the maximum k
# ---------------------------------------------------------------------------
class IntegerCase:
    """k = m = n.  Observation a is row a of L0 (obs[a] = row_perm[a]), so B = L0 and chol(G) = L0; the output is permuted at random.
    x0 in [-8, 8] with y = G x0; W [n x 70] in [-4, 4], X [k x 70] in [-8, 8] and E[:, s] = y - B W[:, s] - G X[:, s]: all integers
    below 2^53 by a wide margin, held in float64 (and exact in float32 where the operator is demoted)."""
    def __init__(self, k):
        rng = np.random.default_rng(3000 + k)
        self.k = self.n = k
        L0 = 2 * np.eye(k, dtype=np.int64)
        for i in range(1, k):
            lo = max(0, i - 40)
            cols = rng.choice(np.arange(lo, i), size=min(3, i - lo), replace=False)
            L0[i, cols] = rng.choice([-1, 1], size=len(cols))
        def mul(a, b):                # integers far below 2^53: the float64 product is exact, and quick at k = 2048
            return np.rint(a.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)
        self.L0 = L0
        self.G = mul(L0, L0.T)
        self.row_perm = rng.permutation(k)
        self.obs = self.row_perm.copy()
        self.x0 = rng.integers(-8, 9, size=k)
        self.y = mul(self.G, self.x0)
        self.W = rng.integers(-4, 5, size=(k, 70))
        self.X = rng.integers(-8, 9, size=(k, 70))
        self.E = self.y[:, None] - mul(L0, self.W) - mul(self.G, self.X)
        self.quad = int(self.x0 @ self.y)
        self.query = rng.permutation(k)[:70]
        self.prior = np.diag(self.G)[inverse_perm(self.row_perm)[self.query]]     # ||row of P L0 at index o||^2 = G[i, i], row_perm[i] = o

    def operand(self):
        return dense_leaf(self.L0.astype(np.float64))


def cholesky_f64_right_looking(a):
    """Lower Cholesky factor in plain float64, right-looking (the order of the device's diagonal-tile kernel)."""
    a = np.array(a, dtype=np.float64)
    k = a.shape[0]
    for c in range(k):
        a[c, c] = np.sqrt(a[c, c])
        a[c + 1:, c] /= a[c, c]
        a[c + 1:, c + 1:] -= np.outer(a[c + 1:, c], a[c + 1:, c])
    return np.tril(a)
