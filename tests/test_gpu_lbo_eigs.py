"""The device eigensolver (bfhipChebCovEigsDevice) on the cases of tests/eigs_cases.py.  Per case, from
ONE pair of calls: the return code, residuals recomputed in numpy float64, eigenvalues index by index against the truth
(Kahan's matching for an orthonormal block), the subspace (Davis-Kahan), orthonormality against the float64 restatement of
the algorithm, and bitwise equal repeats.  Across the cases: a ragged ldu, a live conditioning object, the iteration limit,
the degree cap, the spectral covariance from the returned pairs against the Chebyshev one on one mesh, and the C example.
The truth is analytic for the grid graph and numpy.linalg.eigh of the dense S elsewhere (n <= 1089)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cheb_cases as cc
import eigs_cases as ec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNTIME_ERROR = 2
U53 = 2.0 ** -53


def call(obj, nev, guard=None, degree=None, tol=None, max_iter=None, seed=0, flags=0, ldu=None, fill=0.0):
    """bfhipChebCovEigsDevice through ctypes: (rc, lam, residual, the whole [n, ldu] block as numpy, info dict)."""
    import torch
    from butterfly_amd import _capi
    lib = _capi.load()
    opt = _capi.BfhipEigsOptions()
    opt.structSize = C.sizeof(opt)
    opt.guard, opt.degree, opt.maxIter = guard or 0, degree or 0, max_iter or 0
    opt.tol, opt.seed = tol or 0.0, seed
    opt.flags = flags | (_capi.EIGS_NO_GUARD if guard == 0 else 0)
    info = _capi.BfhipEigsInfo()
    info.structSize = C.sizeof(info)
    ldu = nev if ldu is None else ldu
    lam, res = np.full(nev, np.nan), np.full(nev, np.nan)
    dU = torch.full((obj.n, ldu), fill, dtype=torch.float64, device="cuda:0")
    rc = lib.bfhipChebCovEigsDevice(obj.handle, C.byref(opt), nev, lam.ctypes.data, res.ctypes.data, C.c_void_p(dU.data_ptr()), ldu,
                                    C.byref(info), C.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    return rc, lam, res, dU.cpu().numpy(), info.as_dict()


@pytest.fixture(scope="module")
def objects():
    import torch
    from butterfly_amd import ChebCovariance
    assert torch.cuda.is_available()
    mats, made = ec.matrices(), {}

    def get(name):
        if name not in made:
            m = mats[name]
            made[name] = (m, ChebCovariance.from_csr(m.rowptr, m.colind, m.data, m.mass, device=0))
        return made[name]
    yield get
    for _, o in made.values():
        o.close()


@pytest.fixture(scope="module")
def runs(objects):
    """Per case, computed once: two plain calls, one mass-normalised call, the restatement and the truth."""
    from butterfly_amd import _capi
    made = {}

    def get(case):
        if case not in made:
            name, nev, guard, degree = case
            m, obj = objects(name)
            a = call(obj, nev, guard, degree)
            b = call(obj, nev, guard, degree)
            phi = call(obj, nev, guard, degree, flags=_capi.EIGS_MASS_NORMALISED)
            ref = ec.reference_eigs(m, nev, guard, degree)
            lam, V = m.truth(min(m.n, nev + 1))
            made[case] = dict(m=m, a=a, b=b, phi=phi, ref=ref, lam=lam, V=V[:, :nev])
        return made[case]
    return get


@pytest.mark.parametrize("case", ec.CASES, ids=ec.case_id)
def test_pairs_residuals_values_subspace_orthonormality_and_repeats(runs, case):
    name, nev, guard, degree = case
    r = runs(case)
    m, (rc, theta, res, U, info) = r["m"], r["a"]
    p, lam_max, lam = info["blockColumns"], m.lam_max, r["lam"]
    tag = ec.case_id(case)
    # 1. the call
    assert rc == 0 and info["converged"] == nev and p == ec.block_columns(m.n, nev, guard) and info["lamMax"] == lam_max
    assert np.isfinite(U).all() and np.isfinite(theta).all() and (np.diff(theta) >= 0).all()
    assert info["operatorColumns"] >= p and info["workspaceBytes"] > 0 and info["maxDegreeUsed"] <= (degree or 20)
    print(f"{tag}: p {p}, {info['iterations']} iterations (restatement {r['ref']['iterations']}), largest degree {info['maxDegreeUsed']}, "
          f"max residual / lamMax {info['maxResidual']:.2e}")
    # 2. residuals recomputed in float64
    R = m.ell.mul(U) - U * theta
    rj = np.linalg.norm(R, axis=0)
    rounding = (m.max_row_nnz + 4) * U53 * lam_max
    print(f"{tag}: recomputed residuals up to {rj.max():.2e} (allowed {ec.TOL * lam_max + rounding:.2e}); reported ones differ by {np.abs(res - rj).max():.2e} (allowed {rounding:.2e})")
    assert (rj <= ec.TOL * lam_max + rounding).all()
    assert (np.abs(res - rj) <= rounding).all()
    assert info["maxResidual"] == res.max() / lam_max
    # 3. eigenvalues, index by index
    RF = np.linalg.norm(R)
    err = np.abs(theta - lam[:nev])
    print(f"{tag}: eigenvalue error {err.max():.2e} (allowed {RF + 2 * p * U53 * lam_max:.2e})")
    assert (err <= RF + 2 * p * U53 * lam_max).all()
    # 4. the subspace
    if nev < m.n:
        delta = lam[nev] - theta.max()
        assert delta > 0
        out = np.linalg.norm(U - r["V"] @ (r["V"].T @ U))
        print(f"{tag}: ||(I - P) U||_F {out:.2e} (allowed {RF / delta + p * 2 * U53:.2e})")
        assert out <= RF / delta + p * 2 * U53
    # 5. orthonormality, against the restatement's
    e_ref = np.abs(r["ref"]["U"].T @ r["ref"]["U"] - np.eye(nev)).max()
    bound = 8 * max(e_ref, p * U53)
    e_dev = np.abs(U.T @ U - np.eye(nev)).max()
    rc2, theta2, _, Phi, _ = r["phi"]
    mass = np.ones(m.n) if m.mass is None else m.mass
    e_phi = np.abs(Phi.T @ (mass[:, None] * Phi) - np.eye(nev)).max()
    print(f"{tag}: ||U^T U - I||_max {e_dev:.2e}, ||Phi^T M Phi - I||_max {e_phi:.2e}, restatement {e_ref:.2e} (allowed {bound:.2e})")
    assert e_dev <= bound and e_phi <= bound
    assert rc2 == 0 and (theta2 == theta).all() and (Phi == m.d[:, None] * U).all()          # the flag scales the store by d, nothing else
    # 6. repeats
    rcb, thetab, resb, Ub, infob = r["b"]
    assert rcb == 0 and theta.tobytes() == thetab.tobytes() and res.tobytes() == resb.tobytes() and U.tobytes() == Ub.tobytes()
    assert infob == info


def test_a_ragged_ldu_leaves_the_padding_untouched(objects, runs):
    case = ("graph4221", 17, 3, None)
    m, obj = objects("graph4221")
    rc, theta, res, U, _ = call(obj, 17, 3, ldu=23, fill=-7.25)
    assert rc == 0 and U.shape == (4221, 23)
    assert (U[:, 17:] == -7.25).all()
    _, theta0, res0, U0, _ = runs(case)["a"]
    assert (U[:, :17] == U0).all() and (theta == theta0).all() and (res == res0).all()


def test_a_live_conditioning_object_is_not_disturbed(objects):
    import torch
    from butterfly_amd import matern_density
    m, obj = objects("two_grids")
    obj.set_density(matern_density(0.9, 1.5), 24)
    gen = np.random.default_rng(5)
    obs = gen.choice(m.n, 40, replace=False).astype(np.uint64)
    cond = obj.condition(obs, np.full(40, 0.05))
    y = torch.from_numpy(gen.standard_normal(40)).to("cuda:0")
    before = cond.mean(y).cpu().numpy()
    work = obj.info()["workspaceBytes"]
    rc, *_ = call(obj, 16, 8)
    assert rc == 0
    after = cond.mean(y).cpu().numpy()
    cond.close()
    assert before.tobytes() == after.tobytes() and obj.info()["workspaceBytes"] == work and obj.info()["order"] == 24


def test_the_iteration_limit_is_a_runtime_error_with_finite_outputs(objects):
    from butterfly_amd import _capi
    m, obj = objects("graph4221")
    rc, theta, res, U, info = call(obj, 64, 13, max_iter=1)
    msg = _capi.load().bfhipLastErrorMessage().decode()
    print(msg)
    assert rc == RUNTIME_ERROR and info["iterations"] == 1 and info["converged"] < 64
    assert f"{info['converged']} of 64" in msg
    assert np.isfinite(theta).all() and np.isfinite(res).all() and np.isfinite(U).all()
    assert np.abs(U.T @ U - np.eye(64)).max() <= 8 * 77 * U53                                   # the best pairs found are still an orthonormal block


def test_the_degree_cap_acts_on_the_63_vertex_mesh(runs):
    r = runs(("mesh63", 8, 8, 20))
    print(f"largest degree used {r['a'][4]['maxDegreeUsed']} (restatement {r['ref']['max_degree']})")
    assert 2 <= r["a"][4]["maxDegreeUsed"] < 20


def test_the_spectral_covariance_from_the_pairs_matches_the_chebyshev_one(objects):
    """C = D g(S)^2 D on the 1089-vertex grid, two ways: D p(S)^2 D V by the recurrence (order 256) and D U g(Theta)^2 U^T D V
    from the returned pairs, for a Gaussian g that is below 2^-40 g(0) beyond lambda_nev.  Exactly, the two differ by
    D (p(S)^2 - g(S)^2) D V + D (g(S)^2 restricted to the spectrum from lambda_nev on) D V, so per column by at most
    (max |p^2 - g^2| + max_{lambda >= lambda_nev} g^2) max d^2 ||V_j||; the device adds the bound of tests/test_gpu_cheb_cov.py
    (8 x the float64 forward recurrence's own error against long double, or 8 x 2^-53, in units of (sum |c_k|)^2 max d^2 ||V_j||)."""
    import torch
    from butterfly_amd import _capi, cheb_fit
    nev, q, order = 33, 17, 256
    m, obj = objects("grid33")
    lib = _capi.load()
    lam_all, _ = m.truth(m.n)
    kappa = 40 * np.log(2.0) / lam_all[nev] ** 2
    g = lambda lam: np.exp(-kappa * lam * lam)
    assert g(lam_all[nev]) <= 2.0 ** -40
    coef = cheb_fit(g, order, 0.0, m.lam_max)
    obj.set_coefficients(coef)
    pv = np.array([lib.bfhipChebEval(order, 0.0, m.lam_max, coef.ctypes.data, float(x)) for x in lam_all])
    gv = g(lam_all)
    model = np.abs(pv ** 2 - gv ** 2).max() + (gv[nev:] ** 2).max()
    V = np.random.default_rng(33).standard_normal((m.n, q))
    dV = torch.from_numpy(V).to("cuda:0")
    Zc = obj.matvec_block_device(dV)
    lam, U, info = obj.eigs(nev, guard=16, tol=1e-12)
    assert info["code"] == 0 and info["converged"] == nev
    d = torch.from_numpy(m.d).to("cuda:0")[:, None]
    g2 = torch.from_numpy(g(lam) ** 2).to("cuda:0")[:, None]
    Zs = d * (U @ (g2 * (U.T @ (d * dV))))
    diff = np.linalg.norm((Zc - Zs).cpu().numpy(), axis=0)
    # the device bound of section 22 for this matvec: the float64 forward recurrence against long double, applied twice
    refs = {}
    for dt in (cc.LD, np.float64):
        ell = cc.Ell(m.rowptr, m.colind, m.val, dt)
        dd = m.d.astype(dt)[:, None]
        x = cc.forward_recurrence(ell, m.lam_max, coef, dd * V.astype(dt))
        refs[dt] = dd * cc.forward_recurrence(ell, m.lam_max, coef, x)
    vn = np.linalg.norm(V, axis=0)
    norm = np.abs(coef).sum() ** 2 * m.d.max() ** 2 * vn
    e_ref = np.sqrt(((refs[np.float64].astype(cc.LD) - refs[cc.LD]) ** 2).sum(axis=0)).astype(np.float64) / norm
    bound = model * m.d.max() ** 2 * vn + 8 * np.maximum(e_ref, U53) * norm
    print(f"max |p^2 - g^2| + tail {model:.2e}; difference per column up to {diff.max():.2e} (allowed {bound.min():.2e} .. {bound.max():.2e}); "
          f"||Z|| about {np.linalg.norm(Zc.cpu().numpy(), axis=0).mean():.2e}")
    assert (diff <= bound).all(), float((diff / bound).max())


def test_the_c_example_builds_with_werror_and_exits_zero(tmp_path):
    lib = os.path.join(ROOT, "butterfly_amd", "csrc")
    exe = str(tmp_path / "lbo_eigs_device")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "lbo_eigs_device.c"), "-L", lib, "-lbfhip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-lm", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0
    assert "l(l+1)" in p.stdout
