"""Matrix-free Chebyshev covariance on the device: bfChebStepKernel and the five entries over it.

Reference: the reference's own forward recurrence (examples/covariance/cheb_cov.c: chebmul) in numpy.longdouble on the
same folded S (tests/cheb_cases.py); the project compiles no binary of the reference.  Per column
    ||x_dev - x_ld||_2 <= 8 * max(e_ref, 2^-53) * sum_k |c_k| * ||w||_2
where e_ref is that column's error of the forward recurrence run in float64, normalised the same way: the device
(Clenshaw, fma, another summation order) may be at most 8 times worse than the reference's algorithm in the reference's
precision.  Sample: the same with max d; matvec: with (sum |c_k|)^2 and max d^2.  Every matrix is symmetric positive
semidefinite and lamMax an upper bound of its spectrum, so |T_k| <= 1 and the normalisation is the natural one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cheb_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = (1, 2, 3, 8, 64, 129)
QS = (1, 2, 3, 17, 64, 70)       # 3, 17: lanes past the row's end; 64: a wavefront per row; 70: a second panel
MAXQ = max(QS)
COLS = (0, 1, 2, 16, 63, 64, 69)   # the columns held against the q = 1 results: first and last of every q and of both panels
MATRICES = ("mesh63", "n1", "path5", "wide_and_empty", "dense48", "mesh4099")
FLOOR = 2.0 ** -53


def col_norms(X):
    return np.sqrt((np.asarray(X, dtype=cc.LD) ** 2).sum(axis=0)).astype(np.float64)


class Case:
    """One matrix: the folded S restated on the host, the device object, inputs, and references per order (computed once)."""
    def __init__(self, name, spec):
        from butterfly_amd import ChebCovariance, cheb_fit, matern_density
        self.name, self.spec = name, spec
        self.n = len(spec["rowptr"]) - 1
        self.val, self.d, self.gersh = cc.fold(spec["rowptr"], spec["colind"], spec["data"], spec["mass"])
        self.lam_max = spec["lam_max"] if spec["lam_max"] is not None else self.gersh
        self.ell = {dt: cc.Ell(spec["rowptr"], spec["colind"], self.val, dt) for dt in (cc.LD, np.float64)}
        self.obj = ChebCovariance.from_csr(spec["rowptr"], spec["colind"], spec["data"], spec["mass"], lam_max=spec["lam_max"], device=0)
        rng = np.random.default_rng(len(name) + self.n)
        self.W = rng.standard_normal((self.n, MAXQ))
        # columns the references are computed for: all of them, on the large mesh (long double is slow) those of COLS
        self.rcols = np.arange(MAXQ) if self.n <= 1000 else np.array(COLS)
        self.density = matern_density(0.9, 1.5)
        self.coefs = {order: cheb_fit(self.density, order, 0.0, self.lam_max) for order in ORDERS}
        self._ref = {}

    def ref(self, order, kind="apply"):
        """(x_ld, e_ref per column, normalisation per column) of `kind` at `order` for the columns rcols of W."""
        key = (order, kind)
        if key not in self._ref:
            c = self.coefs[order]
            out = {}
            for dt in (cc.LD, np.float64):
                d = self.d.astype(dt)[:, None]
                x = self.W[:, self.rcols].astype(dt)
                if kind == "matvec":
                    x = cc.forward_recurrence(self.ell[dt], self.lam_max, c, d * x)
                x = cc.forward_recurrence(self.ell[dt], self.lam_max, c, x)
                out[dt] = d * x if kind != "apply" else x
            s = np.abs(c).sum()
            norm = {"apply": s, "sample": s * self.d.max(), "matvec": s * s * self.d.max() ** 2}[kind] * col_norms(self.W[:, self.rcols])
            e_ref = col_norms(out[np.float64].astype(cc.LD) - out[cc.LD]) / norm
            self._ref[key] = (out[cc.LD], e_ref, norm)
        return self._ref[key]

    def run(self, kind, order, q, cols=None):
        import torch
        self.obj.set_coefficients(self.coefs[order])
        W = self.W[:, :q] if cols is None else self.W[:, cols]
        fn = {"apply": self.obj.apply_block_device, "sample": self.obj.sample_block_device, "matvec": self.obj.matvec_block_device}[kind]
        z = fn(torch.from_numpy(np.ascontiguousarray(W)).to("cuda:0"))
        return z.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    import torch
    assert torch.cuda.is_available()
    made = {}
    cat = cc.catalogue()

    def get(name):
        if name not in made:
            made[name] = Case(name, cat[name])
        return made[name]
    yield get
    for c in made.values():
        c.obj.close()


def check_columns(case, kind, order, X, q):
    x_ld, e_ref, norm = case.ref(order, kind)
    k = int((case.rcols < q).sum())                 # rcols is increasing: its first k entries are the columns of this block
    err = col_norms(X[:, case.rcols[:k]].astype(cc.LD) - x_ld[:, :k]) / norm[:k]
    bound = 8 * np.maximum(e_ref[:k], FLOOR)
    print(f"{case.name} {kind} order {order} q {q}: device {err.max():.2e}, forward recurrence in float64 {e_ref[:k].max():.2e}")
    assert np.isfinite(X).all() and (err <= bound).all(), (case.name, kind, order, q, float((err / bound).max()))
    return err


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", MATRICES)
def test_apply_matches_the_long_double_forward_recurrence_and_columns_do_not_depend_on_q(cases, name, order):
    case = cases(name)
    info = case.obj.info()
    assert info["n"] == case.n and info["nnz"] == len(case.val) and info["lamMax"] == case.lam_max      # the fold and the bound, bit for bit
    single = {j: case.run("apply", order, 1, cols=[j])[:, 0] for j in COLS}
    for q in QS:
        X = case.run("apply", order, q)
        assert X.shape == (case.n, q)
        check_columns(case, "apply", order, X, q)
        for j in COLS:
            if j < q:
                assert np.array_equal(X[:, j], single[j]), (name, order, q, j)
    assert case.obj.info()["order"] == order and case.obj.info()["errorEstimate"] == abs(case.coefs[order][-1])


@pytest.mark.parametrize("order", ORDERS)
def test_the_dense_case_matches_the_spectral_truth(cases, order):
    """Z against Q g(Lambda) Q^T W: the interpolation error max |g - p| over the 48 eigenvalues (long double) times ||w||,
    plus the rounding bound of the accuracy test."""
    case = cases("dense48")
    Q, lam = case.spec["Q"].astype(cc.LD), case.spec["lam"].astype(cc.LD)
    c = case.coefs[order].astype(cc.LD)
    t = 2 * lam / cc.LD(case.lam_max) - 1
    p = (c[:, None] * np.cos(np.arange(order, dtype=cc.LD)[:, None] * np.arccos(t)[None, :])).sum(axis=0)
    kap, nu = cc.LD(0.9), cc.LD(1.5)
    g = np.abs(1 + kap * kap * lam) ** (-nu / 4 - cc.LD(0.5))
    assert np.abs(g.astype(np.float64) - case.density(case.spec["lam"])).max() <= 4 * 2.0 ** -52
    interp = float(np.abs(g - p).max())
    truth = (Q * g) @ (Q.T @ case.W.astype(cc.LD))
    _, e_ref, norm = case.ref(order)
    for q in (1, MAXQ):
        X = case.run("apply", order, q)
        err = col_norms(X.astype(cc.LD) - truth[:, :q])
        bound = interp * col_norms(case.W)[:q] + 8 * np.maximum(e_ref[:q], FLOOR) * norm[:q]
        print(f"dense48 order {order} q {q}: max |g - p| {interp:.2e}, device vs truth {(err / col_norms(case.W)[:q]).max():.2e}")
        assert (err <= bound).all(), float((err / bound).max())


# every order on the two small matrices with a mass; one short and one long recurrence on the large mesh
@pytest.mark.parametrize("name,order", [(m, o) for m in ("mesh63", "wide_and_empty") for o in ORDERS] + [("mesh4099", 2), ("mesh4099", 64)])
def test_sample_and_matvec_match_the_sequence_with_d_applied_separately(cases, name, order):
    case = cases(name)
    for kind in ("sample", "matvec"):
        single = {j: case.run(kind, order, 1, cols=[j])[:, 0] for j in (0, 2, 69)}
        for q in (3, MAXQ):
            Z = case.run(kind, order, q)
            check_columns(case, kind, order, Z, q)
            for j in (0, 2, 69):
                if j < q:
                    assert np.array_equal(Z[:, j], single[j]), (name, kind, order, q, j)
    # symmetry of C = D p(S)^2 D: u^T (C v) = v^T (C u); each product is within its bound of the exact one
    Z = case.run("matvec", order, MAXQ)
    _, e_ref, norm = case.ref(order, "matvec")
    assert tuple(case.rcols[:2]) == (0, 1)
    u, v, Cu, Cv = case.W[:, 0].astype(cc.LD), case.W[:, 1].astype(cc.LD), Z[:, 0].astype(cc.LD), Z[:, 1].astype(cc.LD)
    nu, nv = float(np.sqrt((u * u).sum())), float(np.sqrt((v * v).sum()))
    bound = 8 * max(e_ref[0], FLOOR) * norm[0] * nv + 8 * max(e_ref[1], FLOOR) * norm[1] * nu
    assert abs(float(u @ Cv - v @ Cu)) <= bound


def test_runs_are_bit_identical_and_workspace_growth_changes_nothing():
    import torch
    from butterfly_amd import ChebCovariance, cheb_fit, matern_density
    spec = cc.catalogue()["mesh63"]
    rng = np.random.default_rng(5)
    W = torch.from_numpy(rng.standard_normal((63, MAXQ))).to("cuda:0")
    obj = ChebCovariance.from_csr(spec["rowptr"], spec["colind"], spec["data"], spec["mass"], device=0)
    try:
        with pytest.raises(Exception) as ei:                       # no coefficients yet
            obj.apply_block_device(W[:, :3].contiguous())
        assert getattr(ei.value, "code", None) == 1
        lam_max = obj.info()["lamMax"]
        obj.set_coefficients(cheb_fit(matern_density(0.9, 1.5), 64, 0.0, lam_max))
        assert obj.info()["workspaceBytes"] == 0
        small = W[:, :3].contiguous()
        first = {k: getattr(obj, k + "_block_device")(small).cpu().numpy() for k in ("apply", "sample", "matvec")}
        ws = obj.info()["workspaceBytes"]
        assert ws == 3 * 63 * 3 * 8
        wide = {k: getattr(obj, k + "_block_device")(W).cpu().numpy() for k in ("apply", "sample", "matvec")}
        assert obj.info()["workspaceBytes"] == 3 * 63 * MAXQ * 8
        for k in first:
            again = getattr(obj, k + "_block_device")(small).cpu().numpy()
            assert np.array_equal(again, first[k]) and np.array_equal(wide[k][:, :3], first[k]), k
            assert np.array_equal(getattr(obj, k + "_block_device")(W).cpu().numpy(), wide[k]), k
        # in-place use and a bad q are refused
        lib = obj._lib
        p = C.c_void_p(W.data_ptr())
        assert lib.bfhipChebCovApplyBlockDevice(obj.handle, p, 3, p, None) == 1
        assert lib.bfhipChebCovSampleBlockDevice(obj.handle, p, 0, C.c_void_p(small.data_ptr()), None) == 1
        assert lib.bfhipChebCovMatvecBlockDevice(obj.handle, p, 65536, C.c_void_p(small.data_ptr()), None) == 1
        assert lib.bfhipChebCovDrawDevice(obj.handle, 1, 0, 0, p, None) == 1
        assert lib.bfhipChebCovMomentsDevice(obj.handle, 1, 0, 10, 65, p, None, None) == 1
        assert lib.bfhipChebCovMomentsDevice(obj.handle, 1, 0, 0, 64, p, None, None) == 1
        assert lib.bfhipChebCovMomentsDevice(obj.handle, 1, 0, 10, 64, None, None, None) == 1
        torch.cuda.synchronize()
    finally:
        obj.close()


def test_draw_equals_the_sample_of_device_normals_and_moments_equal_the_stored_draws():
    import torch
    from butterfly_amd import ChebCovariance, _capi, matern_density
    verts, faces = cc.jittered_grid_mesh()
    obj = ChebCovariance.from_trimesh(verts, faces, device=0)
    try:
        n, seed, first, K = 63, 99, 5, 150
        obj.set_density(matern_density(0.9, 1.5), 8)
        lib = _capi.load()
        stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        draws = []
        for s0, q in ((0, 64), (64, 64), (128, 22)):
            Z = obj.draw_device(seed, first + s0, q)
            W = torch.empty((q, n), dtype=torch.float64, device="cuda:0")      # row s = the normals of sample first + s0 + s
            with torch.cuda.device(0):
                for s in range(q):
                    assert lib.bfhipFillNormalDevice(C.c_void_p(W[s].data_ptr()), n, (first + s0 + s) * n, _capi.BFHIP_F64, seed, stream) == 0
            Zw = obj.sample_block_device(W.t().contiguous())
            assert torch.equal(Z, Zw), (s0, q)
            draws.append(Z.cpu().numpy())
        Zall = np.concatenate(draws, axis=1)
        assert Zall.shape == (n, K) and np.isfinite(Zall).all() and Zall.std() > 0
        base1, base2 = np.linspace(-1, 1, n), np.linspace(2, 3, n)
        s1, s2 = torch.from_numpy(base1.copy()).to("cuda:0"), torch.from_numpy(base2.copy()).to("cuda:0")
        obj.moments_device(seed, first, K, 64, s1, s2)                         # 64 + 64 + 22, += into non-zero buffers
        want1, want2 = Zall.astype(cc.LD).sum(axis=1), (Zall.astype(cc.LD) ** 2).sum(axis=1)
        b1, b2 = K * 2.0 ** -52 * (np.abs(Zall).sum(axis=1) + np.abs(base1)), K * 2.0 ** -52 * ((Zall ** 2).sum(axis=1) + np.abs(base2))
        got1, got2 = s1.cpu().numpy(), s2.cpu().numpy()
        assert (np.abs(got1.astype(cc.LD) - base1 - want1) <= b1).all() and (np.abs(got2.astype(cc.LD) - base2 - want2) <= b2).all()
        only1, only2 = torch.zeros(n, dtype=torch.float64, device="cuda:0"), torch.zeros(n, dtype=torch.float64, device="cuda:0")
        obj.moments_device(seed, first, K, 64, only1, None)                    # either output may be NULL
        obj.moments_device(seed, first, K, 64, None, only2)
        assert (np.abs(only1.cpu().numpy().astype(cc.LD) - want1) <= b1).all() and (np.abs(only2.cpu().numpy().astype(cc.LD) - want2) <= b2).all()
        again = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        obj.moments_device(seed, first, K, 64, again, None)
        assert torch.equal(again, only1)
    finally:
        obj.close()


def test_the_c_example_builds_with_werror_and_exits_zero(tmp_path):
    lib = os.path.join(ROOT, "butterfly_amd", "csrc")
    exe = str(tmp_path / "cheb_cov_device")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cheb_cov_device.c"), "-L", lib, "-lbfhip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-lm", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe, "24", "48", "64"], capture_output=True, text=True, timeout=120)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0
    assert "covariance column" in p.stdout
