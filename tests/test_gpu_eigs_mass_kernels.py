"""The mass step of the consistent-mass eigensolver (bfEigsMassStepKernel, bfhip_eigs_mass.hip), one launch
at a time through bfdevEigsMassStep, and bfdevEigsMassSolve on the sphere's B.  The matrices, b1 and b2 are the step designs of
tests/eigs_kernel_cases.py (imported, not edited) with their values in the place of the mass; w is drawn here.

  out = alpha (B b1) + beta b1 + gamma b2 + delta w
  "int"    entries in [-3, 3] and integer scalars: bit-equal to numpy's float64 result.
  "float"  against numpy.longdouble within (nnz_i + 4) u (|alpha| sum_j |B_ij| |b1_jc| + |beta| |b1_ic| + |gamma| |b2_ic| + |delta| |w_ic|),
           u = 2^-53: nnz_i fmas of the row sum, the scaling by alpha and three more fmas.
Per p: out of place, out == b2 (equal bits), a repeat into fresh outputs (equal bytes), sentinels in the columns p .. ld - 1 and in
16 rows past the end, and for p in {3, 9, 65, 130} every column against the one-column launch at ld = 16, bit for bit.  The
forms with NULL terms (B X alone; delta w alone, the mass solve's first step) ride along; bfdevEigsDualProduct (S X and B X from
one gather) is held to the two single launches bit for bit.  One test needs no GPU: on the
references alone, leaving out the w term or a row's last nonzero breaks the bound by 1e3 at least."""
import ctypes as C
import functools

import numpy as np
import pytest

import eigs_kernel_cases as ek

LD, U = ek.LD, ek.U
NAN, SENT = float("nan"), ek.SENTINEL
SCALARS = {"int": (2.0, -3.0, 1.0, -2.0), "float": (1.7109375, -0.62, -0.3, 0.8125)}        # (alpha, beta, gamma, delta)


class BfEigsMassStep(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("colind", C.c_void_p), ("val", C.c_void_p), ("n", C.c_uint64), ("p", C.c_uint32), ("ld", C.c_uint32),
                ("b1", C.c_void_p), ("b2", C.c_void_p), ("w", C.c_void_p), ("out", C.c_void_p), ("alpha", C.c_double), ("beta", C.c_double),
                ("gamma", C.c_double), ("delta", C.c_double)]


class BfEigsMassSolve(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("colind", C.c_void_p), ("val", C.c_void_p), ("n", C.c_uint64), ("p", C.c_uint32), ("ld", C.c_uint32),
                ("t", C.c_void_p), ("z", C.c_void_p), ("work", C.c_void_p), ("lo", C.c_double), ("hi", C.c_double), ("steps", C.c_uint32),
                ("reserved", C.c_uint32)]


class MassDesign:
    """A step design of eigs_kernel_cases plus w [n, 256] and delta, and the references for all 256 columns at once."""
    def __init__(self, name, kind):
        self.s = ek.step_design(name, kind)
        rng = np.random.default_rng([7, ek.STEP_MATRICES.index(name), int(kind == "int")])
        self.kind, self.n = kind, self.s.n
        self.w = ek.draw(rng, kind, (self.n, 256))
        self.scalars = SCALARS[kind]

    def _terms(self, dtype, val=None):
        s = self.s
        a, b, g, d = (dtype(x) for x in self.scalars)
        ell = ek.cc.Ell(s.rowptr, s.colind, s.val if val is None else val, dtype)
        return a * ell.mul(s.b1.astype(dtype)), b * s.b1.astype(dtype), g * s.b2.astype(dtype), d * self.w.astype(dtype)

    def eval(self, dtype, with_w=True, val=None):
        t = self._terms(dtype, val)
        out = t[0] + t[1] + t[2]
        return out + t[3] + dtype(0) if with_w else out + dtype(0)

    @functools.lru_cache(maxsize=None)
    def reference(self):
        if self.kind == "int":
            return self.eval(np.float64).astype(LD), np.zeros((self.n, 256), dtype=LD)
        s = self.s
        a, b, g, d = (abs(LD(x)) for x in self.scalars)
        mag = a * ek.cc.Ell(s.rowptr, s.colind, np.abs(s.val), LD).mul(np.abs(s.b1).astype(LD)) + b * np.abs(s.b1).astype(LD) \
            + g * np.abs(s.b2).astype(LD) + d * np.abs(self.w).astype(LD)
        return self.eval(LD), (s.deg[:, None] + 4) * LD(U) * mag


@functools.lru_cache(maxsize=None)
def design(name, kind):
    return MassDesign(name, kind)


def test_the_bound_notices_a_missing_w_term_and_a_missing_last_nonzero():
    """No GPU: what the kernel could leave out must break the bound by 1e3 on these designs."""
    for name in ek.STEP_MATRICES:
        m = design(name, "float")
        ref, bound = m.reference()
        assert ek.ratio(m.eval(np.float64), ref, bound) <= 1                     # plain float64 passes
        no_w = ek.ratio(m.eval(np.float64, with_w=False), ref, bound)
        row = int(np.argmax(m.s.deg))
        short = ek.ratio(m.eval(np.float64, val=m.s.without_last_nonzero(row)), ref, bound)
        print(f"{name}: without w {no_w:.1e} x the bound, without the last nonzero of row {row} {short:.1e} x")
        assert no_w >= 1e3 and short >= 1e3
        mi = design(name, "int")
        assert not np.array_equal(mi.eval(np.float64, with_w=False), mi.eval(np.float64))


@pytest.fixture(scope="module")
def dev():
    from test_gpu_eigs_kernels import Device
    d = Device()
    vp = C.c_void_p
    d.lib.bfdevEigsMassStep.argtypes, d.lib.bfdevEigsMassStep.restype = [C.POINTER(BfEigsMassStep), vp], C.c_int
    d.lib.bfdevEigsMassSolve.argtypes, d.lib.bfdevEigsMassSolve.restype = [C.POINTER(BfEigsMassSolve), vp], C.c_int
    return d


@pytest.fixture(scope="module")
def csr(dev):
    made = {}

    def get(name, kind):
        if (name, kind) not in made:
            s = ek.step_design(name, kind)
            made[name, kind] = (dev.ints(s.rowptr, np.int64), dev.ints(s.colind, np.int32), dev.block(s.val))
        return made[name, kind]
    return get


def mass_step(dev, mat, n, p, ld, b1, b2, w, out, scalars):
    ptr = lambda t: t.data_ptr() if t is not None else None
    a = BfEigsMassStep(mat[0].data_ptr(), mat[1].data_ptr(), mat[2].data_ptr(), n, p, ld, ptr(b1), ptr(b2), ptr(w), out.data_ptr(), *scalars)
    assert dev.lib.bfdevEigsMassStep(C.byref(a), dev.stream) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ek.STEP_MATRICES)
@pytest.mark.parametrize("p", ek.STEP_PS)
def test_mass_step(dev, csr, name, p):
    from test_gpu_eigs_kernels import held, padded, same_bytes
    ld = -(-p // 16) * 16
    for kind in ("int", "float"):
        m = design(name, kind)
        s, n, scal, mat = m.s, m.n, m.scalars, csr(name, kind)
        b1, b2, w = dev.block(padded(s.b1, p, ld)), dev.block(padded(s.b2, p, ld)), dev.block(padded(m.w, p, ld))

        def launch(form):
            out = dev.out_block(n, ld)
            if form == "inplace":
                out[:n, :p] = b2[:n, :p]
            if form == "bx":
                mass_step(dev, mat, n, p, ld, b1, None, None, out, (scal[0], 0.0, 0.0, 0.0))
            elif form == "first":
                mass_step(dev, mat, n, p, ld, None, None, w, out, (0.0, 0.0, 0.0, scal[3]))
            else:
                mass_step(dev, mat, n, p, ld, b1, out if form == "inplace" else b2, w, out, scal)
            dev.sync()
            o = out.cpu().numpy()
            assert (o[n:] == SENT).all() and (o[:n, p:] == SENT).all()            # rows from n on and columns from p on: never written
            return o[:n, :p]

        tag = f"mass step {name} p={p}"
        ref, bound = m.reference()
        o = launch("full")
        held(tag, o, (ref[:, :p], bound[:, :p]), kind)
        if kind == "float":
            assert same_bytes(o, launch("full"))
        assert same_bytes(o, launch("inplace"))
        # the forms with NULL terms: alpha B b1 is the step design's reference without beta and gamma; delta w is one product
        if kind == "int":
            bx = launch("bx")
            want = scal[0] * ek.cc.Ell(s.rowptr, s.colind, s.val, np.float64).mul(s.b1[:, :p].copy()) + 0.0
            assert same_bytes(bx + 0.0, want)
        else:
            assert same_bytes(launch("first") + 0.0, scal[3] * m.w[:, :p] + 0.0)
        if kind == "float" and p in ek.STEP_COLUMNWISE_PS:
            B1 = dev.torch.zeros((p, n + ek.GUARD_ROWS, 16), dtype=dev.torch.float64, device=dev.dev)
            B1[:, n:] = NAN
            B2, W, O = B1.clone(), B1.clone(), dev.torch.full_like(B1, SENT)
            B1[:, :n, 0], B2[:, :n, 0], W[:, :n, 0] = b1[:n, :p].T, b2[:n, :p].T, w[:n, :p].T
            for c in range(p):
                mass_step(dev, mat, n, 1, 16, B1[c], B2[c], W[c], O[c], scal)
            dev.sync()
            O = O.cpu().numpy()
            assert (O[:, n:] == SENT).all() and (O[:, :n, 1:] == SENT).all()
            diff = np.count_nonzero(O[:, :n, 0].T != o)
            print(f"{tag}: column by column, {diff} entries differ")
            assert same_bytes(O[:, :n, 0].T, o)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ek.STEP_MATRICES)
def test_dual_product_equals_the_two_single_launches(dev, csr, name):
    """Y = S b1 and T = B b1 from one gather (bfdevEigsDualProduct, Rayleigh-Ritz): each output bit-equal to its own launch
    (bfdevEigsStep with alpha = 1 and the mass step with alpha = 1), with a second value array drawn here in the place of B."""
    from test_gpu_eigs_kernels import padded, same_bytes
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    dev.lib.bfdevEigsDualProduct.argtypes, dev.lib.bfdevEigsDualProduct.restype = [vp, vp, vp, vp, u64, u32, u32, vp, vp, vp, vp], C.c_int
    for kind in ("int", "float"):
        m = design(name, kind)
        s, n, mat = m.s, m.n, csr(name, kind)
        rng = np.random.default_rng([11, ek.STEP_MATRICES.index(name), int(kind == "int")])
        val_b = dev.block(ek.draw(rng, kind, len(s.val)))
        for p in (1, 3, 8, 9, 17, 64, 65, 130):
            ld = -(-p // 16) * 16
            b1 = dev.block(padded(s.b1, p, ld))
            o_s, o_b, y, t = (dev.out_block(n, ld) for _ in range(4))
            dev.step(mat, n, p, ld, b1, None, o_s, (1.0, 0.0, 0.0))
            mass_step(dev, (mat[0], mat[1], val_b), n, p, ld, b1, None, None, o_b, (1.0, 0.0, 0.0, 0.0))
            assert dev.lib.bfdevEigsDualProduct(mat[0].data_ptr(), mat[1].data_ptr(), mat[2].data_ptr(), val_b.data_ptr(), n, p, ld, b1.data_ptr(),
                                                y.data_ptr(), t.data_ptr(), dev.stream) == 0
            dev.sync()
            y, t, o_s, o_b = (x.cpu().numpy() for x in (y, t, o_s, o_b))
            for o in (y, t):
                assert (o[n:] == SENT).all() and (o[:n, p:] == SENT).all()
            assert same_bytes(y[:n, :p] + 0.0, o_s[:n, :p] + 0.0) and same_bytes(t[:n, :p] + 0.0, o_b[:n, :p] + 0.0)
            if kind == "int":
                want = ek.cc.Ell(s.rowptr, s.colind, s.val, np.float64).mul(s.b1[:, :p].copy()) + 0.0
                assert same_bytes(y[:n, :p] + 0.0, want)


@pytest.mark.gpu
def test_mass_solve_meets_the_chebyshev_bound_on_the_sphere(dev):
    import consistent_eigs_cases as kc
    from test_gpu_eigs_kernels import same_bytes
    s = kc.pencils()["sphere"]
    n, p, ld = s.n, 4, 16
    B = s.dense()[1]
    t = np.zeros((n, ld))
    t[:, :p] = np.random.default_rng(0).standard_normal((n, p))
    z = np.linalg.solve(B, t[:, :p])
    zn = np.linalg.norm(z)
    mat = (dev.ints(s.rowptr, np.int64), dev.ints(s.colind, np.int32), dev.block(s.bval))
    dT = dev.block(t)
    for k in (8, 16, 24, 30):
        outs = []
        for _ in range(2):
            dZ, dW = dev.out_block(n, ld), dev.out_block(n, ld)
            a = BfEigsMassSolve(mat[0].data_ptr(), mat[1].data_ptr(), mat[2].data_ptr(), n, p, ld, dT.data_ptr(), dZ.data_ptr(), dW.data_ptr(), 0.25, 1.0, k, 0)
            assert dev.lib.bfdevEigsMassSolve(C.byref(a), dev.stream) == 0
            dev.sync()
            o, wk = dZ.cpu().numpy(), dW.cpu().numpy()
            assert (o[n:] == SENT).all() and (o[:n, p:] == SENT).all() and (wk[n:] == SENT).all() and (wk[:n, p:] == SENT).all()
            outs.append(o[:n, :p])
        err = np.linalg.norm(outs[0] - z)
        ref = np.linalg.norm(kc.mass_solve(s.b_ell.mul, t[:, :p], 0.25, 1.0, k) - z)
        print(f"mass solve k = {k}: error {err / zn:.3e} of ||z|| (allowed {4 * 3.0 ** -k + 64 * U:.3e}; the restatement's {ref / zn:.3e})")
        assert err <= (4 * 3.0 ** -k + 64 * U) * zn
        assert same_bytes(outs[0], outs[1])
        if k == 30:
            assert err <= 1e-13 * zn
