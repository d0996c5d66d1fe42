"""Log-likelihood with gradients and kriging variances of a conditioned field, the part that needs
no GPU: the exported symbols, the size of BfhipCovCondLikOptions, the argument checks that need only the arguments (reached
with a stand-in object pointer that is never dereferenced, as in tests/test_cov_condition_cpu.py), and the reference
formulas themselves, which tests/test_gpu_cov_likelihood.py holds the device to: they are checked here in long double
against central differences and against the homogeneity identity, so the specification is pinned without a GPU.

The two checks that read the object (a workspace below one strip needs numObs, a query index out of range needs numRows)
cannot be reached here: an object only comes out of bfhipCovCondCreate, which a plan-only operator refuses.  They are
exercised on the device, in tests/test_gpu_cov_likelihood.py::test_refusals_on_the_device."""
import ctypes as C
import os
import subprocess

import numpy as np

from butterfly_amd import _capi
from butterfly_amd.operator import CovCondition
from test_gpu_cov_condition import cholesky_ld, solve_ld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, RANGE = 1, 5
LD = np.longdouble
PI_LD = 4 * np.arctan(LD(1))


def forward_ld(l, r):
    """L^-1 R in long double."""
    x = np.array(r, dtype=LD)
    for c in range(l.shape[0]):
        x[c] = (x[c] - l[c, :c] @ x[:c]) / l[c, c]
    return x


class LikReference:
    """Everything the likelihood entry returns, in long double, from Bt [n x k] (rows already scaled by gamma), the noise
    variances and y: value = (logLik, quad, logDet), g = d logLik / d log gamma, h = d logLik / d noiseVar."""
    def __init__(self, Bt, noise, y):
        Bt, d, y = np.asarray(Bt, dtype=LD), np.asarray(noise, dtype=LD), np.asarray(y, dtype=LD)
        k = Bt.shape[1]
        self.K = Bt.T @ Bt + np.diag(d)
        self.L = cholesky_ld(self.K)
        self.alpha = solve_ld(self.L, y)
        self.quad = y @ self.alpha
        self.logdet = 2 * np.log(np.diag(self.L)).sum()
        self.loglik = -self.quad / 2 - self.logdet / 2 - LD(k) / 2 * np.log(2 * PI_LD)
        self.u = Bt @ self.alpha
        self.bnorm2 = (Bt ** 2).sum(axis=1)                                   # ||b_j||^2
        self.g = self.u ** 2 - (forward_ld(self.L, Bt.T) ** 2).sum(axis=0)
        self.h = (self.alpha ** 2 - (forward_ld(self.L, np.eye(k, dtype=LD)) ** 2).sum(axis=0)) / 2
        self.k, self.d = k, d


def test_the_new_symbols_are_exported():
    lib = _capi.load()
    for name in ("bfhipCovCondLogLikelihoodDevice", "bfhipCovCondVarianceDevice"):
        assert hasattr(lib, name), name
    for name in ("log_likelihood", "variance"):
        assert callable(getattr(CovCondition, name)), name


def test_options_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bfhip.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(BfhipCovCondLikOptions), '
                   'offsetof(BfhipCovCondLikOptions, workspaceBytes), sizeof(BfhipCovCondInfo));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_ws, info = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(_capi.BfhipCovCondLikOptions) == 16
    assert off_ws == _capi.BfhipCovCondLikOptions.workspaceBytes.offset == 8
    assert info == 64                                     # the info struct did not grow


def test_argument_checks_read_nothing_through_the_object():
    """No pointer below is ever dereferenced, the stand-in object least of all: every call ends in a check that needs only
    the arguments.  (0x1000 stands for "not NULL".)  The order is the header's: NULLs, the query set, structSize."""
    lib = _capi.load()
    p = C.c_void_p(0x1000)
    lik, var = lib.bfhipCovCondLogLikelihoodDevice, lib.bfhipCovCondVarianceDevice
    msg = lib.bfhipLastErrorMessage
    good = _capi.BfhipCovCondLikOptions(16, 0, 0)
    assert lik(None, p, p, None, None, None, None) == INVALID and b"NULL" in msg()
    assert lik(p, None, p, p, p, C.byref(good), None) == INVALID and b"NULL" in msg()
    assert lik(p, p, None, p, p, C.byref(good), None) == INVALID and b"NULL" in msg()
    for size in (0, 8, 15, 17, 24):
        bad = _capi.BfhipCovCondLikOptions(size, 0, 1 << 30)
        assert lik(p, p, p, None, None, C.byref(bad), None) == INVALID and b"structSize" in msg(), size
    # a NULL wins over a bad structSize
    bad = _capi.BfhipCovCondLikOptions(8, 0, 0)
    assert lik(p, None, p, None, None, C.byref(bad), None) == INVALID and b"NULL" in msg()

    q = np.array([3, 7, 11], dtype=np.uint64)
    rep = np.array([3, 7, 3, 10 ** 12], dtype=np.uint64)   # repeated, and far outside any operator: the repetition is found first
    assert var(None, q.ctypes.data, 3, p, p, None) == INVALID and b"NULL" in msg()
    assert var(p, None, 3, p, p, None) == INVALID and b"NULL" in msg()
    assert var(p, None, 0, None, None, None) == INVALID and b"NULL" in msg()
    assert var(p, q.ctypes.data, 0, p, p, None) == INVALID and b"numQuery" in msg()
    assert var(p, q.ctypes.data, 0, None, None, None) == INVALID and b"numQuery" in msg()
    assert var(p, q.ctypes.data, 3, None, None, None) == INVALID and b"both" in msg()
    assert var(p, rep.ctypes.data, 4, None, None, None) == INVALID and b"both" in msg()
    assert var(p, rep.ctypes.data, 4, p, None, None) == INVALID and b"repeated" in msg()
    assert var(p, rep.ctypes.data, 4, None, p, None) == INVALID and b"repeated" in msg()


def test_reference_formulas_in_long_double():
    """12 observations of 9 weights (G alone is singular).  Central differences of the reference logLik in log gamma_j and in
    noiseVar[a], step 1e-6, agree with the reference gradients to 1e-6 relative, entry by entry; and
    sum_j g_j / 2 + sum_a h_a d_a = (quad - k) / 2 to 1e-15 relative."""
    rng = np.random.default_rng(2111)
    k, n, step = 12, 9, LD(1e-6)
    B = rng.standard_normal((k, n)).astype(LD)             # unscaled observed rows Phi[i_a, :]
    gam = (rng.random(n) + 0.1).astype(LD)
    d = (0.05 + rng.random(k)).astype(LD)
    y = rng.standard_normal(k).astype(LD)

    def lik(log_gam, noise):
        return LikReference((B * np.exp(log_gam)).T, noise, y).loglik

    ref = LikReference((B * gam).T, d, y)
    lg = np.log(gam)
    worst_g = worst_h = 0.0
    for j in range(n):
        e = np.zeros(n, dtype=LD); e[j] = step
        fd = (lik(lg + e, d) - lik(lg - e, d)) / (2 * step)
        worst_g = max(worst_g, float(abs(fd - ref.g[j]) / abs(ref.g[j])))
    for a in range(k):
        e = np.zeros(k, dtype=LD); e[a] = step
        fd = (lik(lg, d + e) - lik(lg, d - e)) / (2 * step)
        worst_h = max(worst_h, float(abs(fd - ref.h[a]) / abs(ref.h[a])))
    lhs, rhs = ref.g.sum() / 2 + ref.h @ d, (ref.quad - k) / 2
    hom = float(abs(lhs - rhs) / abs(rhs))
    print(f"central differences vs reference gradients, max relative: log gamma {worst_g:.3e}, noise {worst_h:.3e}; homogeneity {hom:.3e}")
    assert worst_g <= 1e-6 and worst_h <= 1e-6
    assert hom <= 1e-15
