"""The consistent-mass pencil on the device (BFHIP_EIGS_CONSISTENT_MASS) on the cases of
tests/consistent_eigs_cases.py.  The reference's sphere in one call of 81 pairs and by bands (49 locked, then 32) against the
reference's own fixture (tests/golden/sphere_phi_500x32.npz: eigenvalues, and the two clusters' spans); the small and designed
cases against a dense generalised eigensolve in numpy; the lumped calls bit for bit before and after a mass is set; a live
conditioning object; the C example.

The rules (u = 2^-53, lamMaxG = lamMax / lo, p the block's columns, B = D M D):
  eigenvalues   |theta_j - lam_j| <= 2 res_j + 64 u lamMaxG on the sphere (the issue's rule: 2 = 1 / sqrt(lo) turns the 2-norm residual
                into the B^-1 norm the pencil's perturbation bound wants); on the small cases, which hold multiple eigenvalues,
                the block form 2 ||R||_F + 64 u lamMaxG (Kahan's matching for a B-orthonormal block).
  residuals     recomputed in float64 on the host, S u - theta B u with u = Phi / d: <= tol lamMaxG + (nnz_row + 4) u lamMaxG, the
                rounding term of tests/test_gpu_lbo_eigs.py with this pencil's bound (||u||_2 <= 2, |S| <= lamMax, theta |B| <= lamMaxG).
  B-orthonormality  within 8 max(the float64 restatement's, p u), section 25's rule.
  clusters      the M-norm of a fixture vector minus its M-projection onto the device's cluster span
                <= 2 ||R_cluster||_F / delta + 2e-11 (consistent_eigs_cases.cluster_bound).
The outer iterations are capped at twice what the restatement took (consistent_eigs_cases.MEASURED_ITERS)."""
import os
import subprocess

import numpy as np
import pytest

import cheb_cases as cc
import consistent_eigs_cases as kc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def objects():
    import torch
    from butterfly_amd import ChebCovariance
    assert torch.cuda.is_available()
    pens, made = kc.pencils(), {}

    def get(name):
        if name not in made:
            pen = pens[name]
            obj = ChebCovariance.from_csr(pen.rowptr, pen.colind, pen.data, pen.mass, device=0)
            if pen.bounds is None:
                obj.set_consistent_mass(pen.mdata)
            else:
                obj.set_consistent_mass(pen.mdata, *pen.bounds)
            made[name] = (pen, obj)
        return made[name]
    yield get
    for _, o in made.values():
        o.close()


def recomputed(pen, theta, U):
    """(R, its column norms) of S U - B U diag(theta) in float64, and the rounding allowance."""
    R = pen.s_ell.mul(U) - pen.b_ell.mul(U) * theta
    nnz_row = int(np.diff(pen.rowptr.astype(np.int64)).max())
    return R, np.linalg.norm(R, axis=0), (nnz_row + 4) * U53 * pen.lam_max_g


def b_gram_error(pen, U):
    return float(np.abs(U.T @ pen.b_ell.mul(U) - np.eye(U.shape[1])).max())


# ---------------------------------------------------------------------------
# the reference's sphere
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_call(objects):
    pen, obj = objects("sphere")
    tol, cap = 1e-12, 2 * kc.MEASURED_ITERS["sphere-81@1e-12"]
    runs = [obj.eigs(kc.SPHERE_NEV, tol=tol, max_iter=cap, mass_normalised=True, consistent_mass=True, raise_on_limit=False) for _ in range(2)]
    ref = kc.reference_eigs_consistent(pen, kc.SPHERE_NEV, tol=tol, max_iter=cap)
    return pen, tol, [(lam, Phi.cpu().numpy(), info) for lam, Phi, info in runs], ref


def test_the_sphere_in_one_call_reproduces_the_reference_fixture(sphere_call):
    pen, tol, runs, ref = sphere_call
    _, _, lam_fix, phi_fix = kc.sphere_fixture()
    theta, Phi, info = runs[0]
    res, p = info["residual"], info["blockColumns"]
    assert info["code"] == 0 and info["converged"] == 81 and info["lamMax"] == pen.lam_max_g and p == 101
    print(f"sphere: p {p}, {info['iterations']} iterations (restatement {ref['iterations']}), largest degree {info['maxDegreeUsed']}, "
          f"max residual / lamMaxG {info['maxResidual']:.2e}, {info['operatorColumns']} operator columns, {info['workspaceBytes']} workspace bytes")
    assert info["workspaceBytes"] >= 5 * pen.n * 112 * 8
    # eigenvalues 49 .. 80 against the fixture
    err = np.abs(theta[49:] - lam_fix)
    allowed = 2 * res[49:] + 64 * U53 * pen.lam_max_g
    print(f"sphere: eigenvalue error up to {err.max():.2e} (smallest allowance {allowed.min():.2e}); relative {np.abs(theta[49:] / lam_fix - 1).max():.2e}")
    assert (err <= allowed).all()
    # residuals recomputed on the host
    U = Phi / pen.d[:, None]
    R, rj, rounding = recomputed(pen, theta, U)
    print(f"sphere: recomputed residuals up to {rj.max():.2e} (allowed {tol * pen.lam_max_g + rounding:.2e}); reported ones differ by {np.abs(res - rj).max():.2e}")
    assert (rj <= tol * pen.lam_max_g + rounding).all() and (np.abs(res - rj) <= rounding).all()
    # Phi^T M Phi = I
    M = cc.csr_to_dense(pen.rowptr, pen.colind, pen.mdata, pen.n)
    Phi_ref = pen.d[:, None] * ref["U"]
    e_ref = np.abs(Phi_ref.T @ M @ Phi_ref - np.eye(81)).max()
    e_dev = np.abs(Phi.T @ M @ Phi - np.eye(81)).max()
    print(f"sphere: ||Phi^T M Phi - I||_max {e_dev:.2e}, restatement {e_ref:.2e} (allowed {8 * max(e_ref, p * U53):.2e})")
    assert e_dev <= 8 * max(e_ref, p * U53)
    # the clusters l = 7 and l = 8 against the fixture's vectors
    lam_true, _ = pen.truth()
    for a, b in kc.SPHERE_CLUSTERS:
        dist = kc.cluster_distance(lambda V: M @ V, phi_fix[:, a - 49:b - 49], Phi[:, a:b])
        bound = kc.cluster_bound(rj, lam_true, a, b)
        print(f"sphere: cluster {a}..{b - 1}: M-distance of the fixture's vectors from the device's span {dist:.2e} (allowed {bound:.2e})")
        assert dist <= bound
    # two calls, equal bits
    theta2, Phi2, info2 = runs[1]
    assert theta.tobytes() == theta2.tobytes() and Phi.tobytes() == Phi2.tobytes() and res.tobytes() == info2["residual"].tobytes()


def test_the_sphere_by_bands_after_49_locked_pairs(objects):
    import torch
    pen, obj = objects("sphere")
    _, _, lam_fix, _ = kc.sphere_fixture()
    lam_true, U_true = pen.truth(49)
    all_u = torch.zeros((pen.n, 81), dtype=torch.float64, device="cuda:0")
    lam_all = np.zeros(81)
    lam0, _, info0 = obj.eigs_band(49, None, out=all_u[:, :49], consistent_mass=True)
    lam_all[:49] = lam0
    cap = 2 * kc.MEASURED_ITERS["sphere-band-32"]
    lam1, _, info1 = obj.eigs_band(32, (all_u, lam_all, 49), out=all_u[:, 49:], consistent_mass=True, max_iter=cap, raise_on_limit=False)
    assert info1["code"] == 0 and info1["converged"] == 32 and info1["blockColumns"] == 40
    ref = kc.reference_eigs_consistent(pen, 32, locked=(U_true, lam_true), max_iter=cap)
    print(f"band: {info0['iterations']} iterations for the 49, {info1['iterations']} for the band of 32 (restatement {ref['iterations']})")
    err = np.abs(lam1 - lam_fix)
    assert (err <= 2 * info1["residual"] + 64 * U53 * pen.lam_max_g).all()
    U = all_u.cpu().numpy()
    full_ref = np.concatenate([U_true, ref["U"]], axis=1)
    e_ref, e_dev = b_gram_error(pen, full_ref), b_gram_error(pen, U)
    print(f"band: eigenvalue error {err.max():.2e}; ||U^T B U - I||_max over 81 columns {e_dev:.2e}, restatement {e_ref:.2e}")
    assert e_dev <= 8 * max(e_ref, 81 * U53)                  # 81: the columns the Gram matrix runs over
    _, rj, rounding = recomputed(pen, lam1, U[:, 49:])
    assert (rj <= kc.TOL * pen.lam_max_g + rounding).all()


def test_eigs_bands_runs_the_consistent_pencil_into_one_array(objects):
    pen, obj = objects("sphere")
    lam, U, infos = obj.eigs_bands(81, band=32, consistent_mass=True)
    lam_true, _ = pen.truth(81)
    U = U.cpu().numpy()
    assert [i["code"] for i in infos] == [0, 0, 0] and U.shape == (500, 81)
    R, rj, rounding = recomputed(pen, lam, U)
    assert (rj <= kc.TOL * pen.lam_max_g + rounding).all()
    assert (np.abs(lam - lam_true) <= 2 * np.linalg.norm(R) + 64 * U53 * pen.lam_max_g).all()
    # the restatement band by band, as eigs_bands runs them: 32, 32, 17
    Q, lam_q = np.zeros((pen.n, 0)), np.zeros(0)
    for nev in (32, 32, 17):
        r = kc.reference_eigs_consistent(pen, nev, locked=(Q, lam_q) if Q.shape[1] else None)
        Q, lam_q = np.concatenate([Q, r["U"]], axis=1), np.concatenate([lam_q, r["lam"]])
    e_ref, e = b_gram_error(pen, Q), b_gram_error(pen, U)
    print(f"eigs_bands: iterations {[i['iterations'] for i in infos]}, ||U^T B U - I||_max {e:.2e}, restatement {e_ref:.2e}")
    assert e <= 8 * max(e_ref, 81 * U53)


# ---------------------------------------------------------------------------
# small and designed cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.SMALL_CASES, ids=kc.case_id)
def test_small_cases_against_the_dense_truth(objects, case):
    name, nev, guard, _ = case
    pen, obj = objects(name)
    tag = kc.case_id(case)
    cap = max(2 * kc.MEASURED_ITERS[tag], 1)
    runs = [obj.eigs(nev, guard=guard, max_iter=cap, consistent_mass=True, raise_on_limit=False) for _ in range(2)]
    theta, U, info = runs[0][0], runs[0][1].cpu().numpy(), runs[0][2]
    ref = kc.reference_eigs_consistent(pen, nev, guard, max_iter=cap)
    p = info["blockColumns"]
    print(f"{tag}: p {p}, {info['iterations']} iterations (restatement {ref['iterations']}), largest degree {info['maxDegreeUsed']}, "
          f"max residual / lamMaxG {info['maxResidual']:.2e}, lamMaxG {info['lamMax']:.6g}")
    assert info["code"] == 0 and info["converged"] == nev and p == ref["p"]
    assert abs(info["lamMax"] / pen.lam_max_g - 1) <= 4 * U53
    lam, _ = pen.truth(nev)
    R, rj, rounding = recomputed(pen, theta, U)
    assert (rj <= kc.TOL * pen.lam_max_g + rounding).all() and (np.abs(info["residual"] - rj) <= rounding).all()
    err = np.abs(theta - lam)
    print(f"{tag}: eigenvalue error {err.max():.2e} (allowed {2 * np.linalg.norm(R) + 64 * U53 * pen.lam_max_g:.2e})")
    assert (err <= 2 * np.linalg.norm(R) + 64 * U53 * pen.lam_max_g).all()
    e_ref, e_dev = b_gram_error(pen, ref["U"]), b_gram_error(pen, U)
    print(f"{tag}: ||U^T B U - I||_max {e_dev:.2e}, restatement {e_ref:.2e} (allowed {8 * max(e_ref, p * U53):.2e})")
    assert e_dev <= 8 * max(e_ref, p * U53)
    if p == pen.n:
        assert info["iterations"] == 0 and info["maxDegreeUsed"] == 0           # the first Rayleigh-Ritz step is exact: no filter
    assert runs[1][0].tobytes() == theta.tobytes() and runs[1][1].cpu().numpy().tobytes() == U.tobytes()


# ---------------------------------------------------------------------------
# nothing else changes
# ---------------------------------------------------------------------------
def test_the_lumped_calls_keep_their_bits_with_a_mass_set():
    from butterfly_amd import ChebCovariance
    pen = kc.pencils()["two_grids"]
    obj = ChebCovariance.from_csr(pen.rowptr, pen.colind, pen.data, pen.mass, device=0)

    def lumped():
        lam, U, info = obj.eigs(16, guard=8)
        lam_b, U_b, info_b = obj.eigs_band(8, (U, lam), guard=8)
        return (lam.tobytes(), U.cpu().numpy().tobytes(), info["residual"].tobytes(), info["workspaceBytes"], info["operatorColumns"],
                lam_b.tobytes(), U_b.cpu().numpy().tobytes(), info_b["residual"].tobytes(), info_b["workspaceBytes"])

    before = lumped()
    obj.set_consistent_mass(pen.mdata)
    after_set = lumped()
    lam_c, _, info_c = obj.eigs(16, guard=8, consistent_mass=True)
    after_call = lumped()
    obj.set_consistent_mass(pen.mdata)                      # a second call replaces the array
    lam_c2, _, _ = obj.eigs(16, guard=8, consistent_mass=True)
    obj.close()
    assert before == after_set == after_call
    assert lam_c.tobytes() == lam_c2.tobytes() and info_c["workspaceBytes"] > before[3]
    assert abs(lam_c[5] / np.frombuffer(before[0])[5] - 1) > 1e-3             # the other pencil has other numbers (0.4 % at least here)


def test_a_live_conditioning_object_survives_a_consistent_call(objects):
    import torch
    from butterfly_amd import matern_density
    pen, obj = objects("two_grids")
    obj.set_density(matern_density(0.9, 1.5), 24)
    gen = np.random.default_rng(5)
    obs = gen.choice(pen.n, 40, replace=False).astype(np.uint64)
    cond = obj.condition(obs, np.full(40, 0.05))
    y = torch.from_numpy(gen.standard_normal(40)).to("cuda:0")
    before = cond.mean(y).cpu().numpy()
    work = obj.info()["workspaceBytes"]
    _, _, info = obj.eigs(16, guard=8, consistent_mass=True)
    obj.set_consistent_mass(pen.mdata)
    after = cond.mean(y).cpu().numpy()
    cond.close()
    assert info["code"] == 0
    assert before.tobytes() == after.tobytes() and obj.info()["workspaceBytes"] == work and obj.info()["order"] == 24


def test_the_flag_is_refused_without_a_mass_and_mass_steps_above_64():
    from butterfly_amd import ChebCovariance
    pen = kc.pencils()["mesh63"]
    obj = ChebCovariance.from_csr(pen.rowptr, pen.colind, pen.data, pen.mass, device=0)
    with pytest.raises(Exception, match="no consistent mass"):
        obj.eigs(8, consistent_mass=True)
    obj.set_consistent_mass(pen.mdata)
    with pytest.raises(Exception, match="massSteps"):
        obj.eigs(8, consistent_mass=True, mass_steps=65)
    lam, _, info = obj.eigs(8, consistent_mass=True, mass_steps=64)
    obj.close()
    assert info["code"] == 0 and np.abs(lam - pen.truth(8)[0]).max() <= 1e-9 * pen.lam_max_g


def test_the_c_example_builds_with_werror_and_exits_zero(tmp_path):
    lib = os.path.join(ROOT, "butterfly_amd", "csrc")
    exe = str(tmp_path / "lbo_consistent_device")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "lbo_consistent_device.c"), "-L", lib, "-lbfhip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-lm", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout[-6000:], p.stderr[-2000:])
    assert p.returncode == 0
    assert "l(l+1)" in p.stdout and "consistent mass" in p.stdout
