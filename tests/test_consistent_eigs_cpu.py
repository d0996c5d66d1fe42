"""The consistent-mass pencil of the device eigensolver (BFHIP_EIGS_CONSISTENT_MASS), the part that needs
no GPU: the exported names and the struct's layout against a compiled C program, the P1 mass assembler against a numpy
assembly, the dense generalised spectrum of the reference's sphere against its own fixture (tests/golden/sphere_phi_500x32.npz),
every refusal before a device is touched, the float64 restatement of the algorithm on every case of
tests/consistent_eigs_cases.py, and the new host code under AddressSanitizer and UBSan (tests/native/fem_mass_check.c, a
program of its own)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cheb_cases as cc
import consistent_eigs_cases as kc
from butterfly_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "butterfly_amd", "csrc")
INVALID = 1

MEASURED_ITERS = kc.MEASURED_ITERS


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("cons_sz")
    src = d / "sz.c"
    names = ("n", "nnz", "hRowptr", "hColind", "hD", "dMass", "massLo", "massHi", "massOps")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bfhip_internal.h"\nint main(void){printf("%zu %zu %zu %zu %zu %u", '
                   'sizeof(BfhipEigsOptions), offsetof(BfhipEigsOptions, tol), offsetof(BfhipEigsOptions, flags), offsetof(BfhipEigsOptions, massSteps), '
                   'sizeof(struct BfhipChebCov), BFHIP_EIGS_CONSISTENT_MASS);'
                   + "".join('printf(" %%zu", offsetof(struct BfhipChebCov, %s));' % n for n in names) + 'printf("\\n");return 0;}\n')
    exe = d / "sz"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src), "-o", str(exe)])
    v = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    return dict(options=v[:4], obj_size=v[4], flag=v[5], off=dict(zip(names, v[6:])))


def test_the_new_names_are_exported_and_the_options_keep_their_layout(layout):
    from butterfly_amd import ChebCovariance, trimesh_lbo_fem_mass
    lib = _capi.load()
    for name in ("bfhipTrimeshLboFemMass", "bfhipChebCovSetConsistentMass", "bfdevEigsMassStep", "bfdevEigsMassSolve", "bfEigsMassFold"):
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    assert "#define BFHIP_EIGS_CONSISTENT_MASS 4u" in hdr and _capi.EIGS_CONSISTENT_MASS == 4 == layout["flag"]
    assert "bfhipTrimeshLboFemMass(" in hdr and "bfhipChebCovSetConsistentMass(" in hdr and "bfEigsMassFold" not in hdr
    O = _capi.BfhipEigsOptions
    assert layout["options"] == [C.sizeof(O), O.tol.offset, O.flags.offset, O.massSteps.offset] == [40, 16, 32, 36]     # 36: where `reserved` was
    assert callable(ChebCovariance.set_consistent_mass) and callable(trimesh_lbo_fem_mass)
    import inspect
    for fn in (ChebCovariance.eigs, ChebCovariance.eigs_band, ChebCovariance.eigs_bands):
        assert {"consistent_mass", "mass_steps"} <= set(inspect.signature(fn).parameters)
    assert "consistent_mass" in inspect.signature(ChebCovariance.from_trimesh).parameters


def test_the_mass_assembler_against_numpy_on_the_jittered_grid():
    from butterfly_amd import trimesh_lbo_fem, trimesh_lbo_fem_mass
    verts, faces = cc.jittered_grid_mesh()
    rowptr, colind, _, lumped = trimesh_lbo_fem(verts, faces)
    md = trimesh_lbo_fem_mass(verts, faces, rowptr, colind)
    M_ref, lumped_ref, area = kc.mass_dense(verts, faces)
    M = cc.csr_to_dense(rowptr, colind, md, len(verts))
    scale = np.abs(M_ref).max()
    assert np.abs(M - M_ref).max() <= 16 * kc.U53 * scale and (M_ref[M == 0] == 0).all()
    assert np.abs(M - M.T).max() <= 4 * kc.U53 * scale
    assert np.abs(M.sum(1) - lumped).max() <= 32 * kc.U53 * lumped.max() and np.abs(lumped - lumped_ref).max() <= 32 * kc.U53 * lumped.max()
    assert np.abs(np.diag(M) - lumped / 2).max() <= 32 * kc.U53 * lumped.max()
    assert abs(M.sum() - area) <= 256 * kc.U53 * area
    d = 1 / np.sqrt(lumped)
    ev = np.linalg.eigvalsh(d[:, None] * M * d[None, :])
    print(f"spectrum of D M D on the 7 x 9 grid: [{ev[0]:.4f}, {ev[-1]:.4f}]")
    assert 0.25 - 1e-14 <= ev[0] and ev[-1] <= 1 + 1e-14


def test_the_dense_spectrum_of_the_sphere_is_the_reference_fixture():
    s = kc.pencils()["sphere"]
    _, _, lam_fix, phi_fix = kc.sphere_fixture()
    assert s.n == 500 and s.bounds is None
    lam, U = s.truth()
    assert (lam < 50).sum() == 49 and ((lam >= 50) & (lam <= 100)).sum() == 32
    rel = np.abs(lam[49:81] / lam_fix - 1).max()
    M = cc.csr_to_dense(s.rowptr, s.colind, s.mdata, s.n)
    orth = np.abs(phi_fix.T @ M @ phi_fix - np.eye(32)).max()
    print(f"eigenvalues 49..80 against the fixture: {rel:.2e} relative; fixture Phi^T M Phi - I: {orth:.2e}")
    assert rel <= 1e-13 and orth <= 1e-13
    # the lumped pencil has other numbers: a test against the fixture fails without the feature
    lumped = np.linalg.eigvalsh(s.dense()[0])[49:81]
    assert np.abs(lumped / lam_fix - 1).max() > 0.2
    # the band splits at its largest gap into the l = 7 and l = 8 clusters
    gaps = np.diff(lam[49:81])
    assert int(gaps.argmax()) == 14 and gaps.max() > 10
    ev = np.linalg.eigvalsh(s.dense()[1])
    print(f"spectrum of B on the sphere: [{ev[0]:.4f}, {ev[-1]:.4f}]")
    assert 0.25 <= ev[0] and ev[-1] <= 1 + 1e-14


def _stand_in(layout, pen=None, mass_set=False):
    """A zeroed object with n (and, with a pencil, nnz and the host copies of the pattern and of d) set; device 0 is never entered."""
    buf = (C.c_char * layout["obj_size"])()
    off = layout["off"]
    keep = []
    if pen is None:
        C.c_uint64.from_buffer(buf, off["n"]).value = 100
    else:
        col32 = np.ascontiguousarray(pen.colind, dtype=np.uint32)
        rp, d = np.ascontiguousarray(pen.rowptr, dtype=np.uint64), np.ascontiguousarray(pen.d)
        C.c_uint64.from_buffer(buf, off["n"]).value = pen.n
        C.c_uint64.from_buffer(buf, off["nnz"]).value = len(col32)
        for name, arr in (("hRowptr", rp), ("hColind", col32), ("hD", d)):
            C.c_void_p.from_buffer(buf, off[name]).value = arr.ctypes.data
        keep = [col32, rp, d]
    if mass_set:
        C.c_void_p.from_buffer(buf, off["dMass"]).value = 0x1000
        C.c_void_p.from_buffer(buf, off["massOps"]).value = 0x1000
        C.c_double.from_buffer(buf, off["massLo"]).value = 0.25
        C.c_double.from_buffer(buf, off["massHi"]).value = 1.0
    return buf, keep


def test_set_consistent_mass_refuses_before_the_device_is_touched(layout):
    lib = _capi.load()
    fn, msg = lib.bfhipChebCovSetConsistentMass, lib.bfhipLastErrorMessage
    pen = kc.pencils()["mesh63"]
    obj, keep = _stand_in(layout, pen)
    good = pen.mdata

    def refused(c, md, lo, hi, want):
        rc = fn(c, None if md is None else md.ctypes.data, lo, hi)
        assert rc == INVALID and want in msg(), (rc, msg(), want)

    refused(None, good, 0.0, 0.0, b"NULL")
    refused(obj, None, 0.0, 0.0, b"NULL")
    for bad in (float("nan"), float("inf")):
        md = good.copy(); md[7] = bad
        refused(obj, md, 0.25, 1.0, b"not finite")
        refused(obj, good, bad, 1.0, b"not finite")
        refused(obj, good, 0.25, bad, b"not finite")
    refused(obj, good, 0.5, 0.5, b"0 < lo < hi")
    refused(obj, good, 1.0, 0.25, b"0 < lo < hi")
    refused(obj, good, 0.0, 1.0, b"0 < lo < hi")
    refused(obj, good, -1.0, 1.0, b"0 < lo < hi")
    md = good.copy(); md[3] *= 1 + 1e-9
    refused(obj, md, 0.0, 0.0, b"sums to")
    md = good.copy()
    row = 10
    ks = np.arange(int(pen.rowptr[row]), int(pen.rowptr[row + 1]))
    kd = ks[pen.colind[ks] == row][0]
    ko = ks[pen.colind[ks] != row][0]
    md[ko] += 2 * md[kd]; md[kd] = -md[kd]                  # the row sum stays, the diagonal turns negative
    refused(obj, md, 0.0, 0.0, b"diagonal")
    off = layout["off"]
    assert C.c_void_p.from_buffer(obj, off["dMass"]).value is None and C.c_void_p.from_buffer(obj, off["massOps"]).value is None
    del keep


def test_the_flag_and_mass_steps_are_refused_after_every_older_refusal(layout):
    lib = _capi.load()
    msg = lib.bfhipLastErrorMessage
    bare, _ = _stand_in(layout)
    with_mass, _ = _stand_in(layout, mass_set=True)
    lam = np.full(16, -5.0)
    dU = C.c_void_p(0x1000)
    F = _capi.EIGS_CONSISTENT_MASS

    def options(**kw):
        o = _capi.BfhipEigsOptions()
        o.structSize = C.sizeof(o)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def refused(fn_name, c, opt, want, locked=None):
        args = [c, C.byref(opt)] + ([C.byref(locked) if locked is not None else None] if fn_name.endswith("BandDevice") else [])
        rc = getattr(lib, fn_name)(*args, 10, lam.ctypes.data, None, dU, 10, None, None)
        assert rc == INVALID and want in msg(), (rc, msg(), want)

    for fn_name in ("bfhipChebCovEigsDevice", "bfhipChebCovEigsBandDevice"):
        # the older refusals still come first: the last of them is tol
        refused(fn_name, bare, options(flags=F, massSteps=65, guard=8, degree=2, tol=-1.0), b"tol")
        refused(fn_name, bare, options(flags=F, massSteps=65, guard=8, degree=1), b"degree")
        # then the flag without a mass, before massSteps
        refused(fn_name, bare, options(flags=F, massSteps=65, guard=8), b"no consistent mass")
        refused(fn_name, bare, options(flags=F), b"no consistent mass")
        # then massSteps
        refused(fn_name, with_mass, options(flags=F, massSteps=65, guard=8), b"massSteps")
    # a locked refusal (ld < count) precedes both
    lk = _capi.BfhipEigsLocked()
    lam_l = np.zeros(4)
    lk.structSize, lk.count, lk.dVectors, lk.ld, lk.lam = C.sizeof(lk), 4, 0x2000, 3, lam_l.ctypes.data
    refused("bfhipChebCovEigsBandDevice", bare, options(flags=F, massSteps=65, guard=8), b"locked: ld", locked=lk)
    # with a mass set a locked eigenvalue is held to lamMax / lo: the stand-in's lamMax is 0
    lk.ld = 4
    lam_l[2] = 1.0
    refused("bfhipChebCovEigsBandDevice", with_mass, options(flags=F, guard=8), b"lies above lamMax", locked=lk)
    assert (lam == -5.0).all()


def test_default_mass_steps():
    assert kc.default_mass_steps(0.25, 1.0, 1e-10) == 22 and kc.default_mass_steps(0.25, 1.0, 1e-12) == 26
    assert 2 * 3.0 ** -22 <= 1e-10 < 2 * 3.0 ** -21
    assert kc.default_mass_steps(1e-9, 1.0, 1e-10) == 64               # the cap


def test_the_mass_solve_of_the_restatement_meets_the_chebyshev_bound():
    s = kc.pencils()["sphere"]
    B = s.dense()[1]
    t = np.random.default_rng(0).standard_normal((s.n, 4))
    z = np.linalg.solve(B, t)
    for k in (8, 16, 24, 30):
        err = np.linalg.norm(kc.mass_solve(s.b_ell.mul, t, 0.25, 1.0, k) - z) / np.linalg.norm(z)
        print(f"k = {k}: {err:.2e} (2 x 3^-k = {2 * 3.0 ** -k:.2e})")
        assert err <= 2 * 3.0 ** -k + 64 * kc.U53


@pytest.fixture(scope="module")
def sphere_runs():
    s = kc.pencils()["sphere"]
    return s, {tol: kc.reference_eigs_consistent(s, kc.SPHERE_NEV, tol=tol, max_iter=2 * MEASURED_ITERS[f"sphere-81@{tol:g}"]) for tol in (1e-10, 1e-12)}


def test_the_restatement_reproduces_the_fixture_on_the_sphere(sphere_runs):
    s, runs = sphere_runs
    _, _, lam_fix, phi_fix = kc.sphere_fixture()
    M = cc.csr_to_dense(s.rowptr, s.colind, s.mdata, s.n)
    for tol, r in runs.items():
        key = f"sphere-81@{tol:g}"
        Phi = s.d[:, None] * r["U"]
        orth = np.abs(Phi.T @ M @ Phi - np.eye(81)).max()
        rel = np.abs(r["lam"][49:] / lam_fix - 1).max()
        lam_true, _ = s.truth()
        dist = [kc.cluster_distance(lambda V: M @ V, phi_fix[:, a - 49:b - 49], Phi[:, a:b]) for a, b in kc.SPHERE_CLUSTERS]
        bound = [kc.cluster_bound(r["residual"], lam_true, a, b) for a, b in kc.SPHERE_CLUSTERS]
        print(f"{key}: k = {r['mass_steps']}, {r['iterations']} iterations, largest degree {r['max_degree']}, worst residual {r['worst']:.2e} x lamMaxG, "
              f"eigenvalues {rel:.2e}, Phi^T M Phi - I {orth:.2e}, cluster distances {dist[0]:.2e} {dist[1]:.2e} (bounds {bound[0]:.2e} {bound[1]:.2e})")
        assert r["converged"] == 81 and r["iterations"] <= MEASURED_ITERS[key]
        assert rel <= 1e-13 and orth <= 1e-13 and dist[0] <= bound[0] and dist[1] <= bound[1]


def test_the_restatement_takes_a_band_after_49_locked_pairs():
    s = kc.pencils()["sphere"]
    _, _, lam_fix, _ = kc.sphere_fixture()
    lam, U = s.truth(49)
    r = kc.reference_eigs_consistent(s, kc.SPHERE_BAND, locked=(U, lam), max_iter=2 * MEASURED_ITERS["sphere-band-32"])
    rel = np.abs(r["lam"] / lam_fix - 1).max()
    B = s.dense()[1]
    cross = np.abs(U.T @ B @ r["U"]).max()
    print(f"band of 32 after 49: p = {r['p']}, {r['iterations']} iterations, eigenvalues {rel:.2e}, U_locked^T B U {cross:.2e}")
    assert r["converged"] == 32 and r["iterations"] <= MEASURED_ITERS["sphere-band-32"] and rel <= 1e-13 and cross <= 1e-13


def test_twelve_mass_steps_stagnate_above_the_tolerance():
    """Guards the default: the filter's subspace is the pencil's only to about 3^-k."""
    s = kc.pencils()["sphere"]
    r = kc.reference_eigs_consistent(s, kc.SPHERE_NEV, mass_steps=12, max_iter=2 * MEASURED_ITERS["sphere-81@1e-10"])
    print(f"k = 12: {r['converged']} of 81 converged, worst residual {r['worst']:.2e} x lamMaxG")
    assert r["converged"] < 81 and r["worst"] > 1e-9


@pytest.mark.parametrize("case", kc.SMALL_CASES, ids=kc.case_id)
def test_every_small_case_converges_in_the_restatement(case):
    name, nev, guard, _ = case
    pen = kc.pencils()[name]
    ev = np.linalg.eigvalsh(pen.dense()[1])
    assert pen.lo - 64 * kc.U53 <= ev[0] and ev[-1] <= pen.hi + 64 * kc.U53          # eigvalsh's own rounding
    r = kc.reference_eigs_consistent(pen, nev, guard, max_iter=2 * max(MEASURED_ITERS[kc.case_id(case)], 1))
    lam, _ = pen.truth(nev)
    print(f"{kc.case_id(case)}: [lo, hi] = [{pen.lo:.4f}, {pen.hi:.4f}], k = {r['mass_steps']}, p = {r['p']}, {r['iterations']} iterations")
    assert r["converged"] == nev and r["iterations"] <= MEASURED_ITERS[kc.case_id(case)]
    assert np.abs(r["lam"] - lam).max() <= 1e-10 * pen.lam_max_g
    if name == "two_grids":
        assert abs(lam[0]) < 1e-10 and abs(lam[1]) < 1e-10 and lam[2] > 1e-4           # lambda = 0 twice
    if name in ("path5", "grid33"):
        assert pen.bounds is not None and abs(pen.bounds[0] / ev[0] - 0.99) < 1e-12    # the caller's bounds: eigvalsh widened by 1 %


def test_the_new_host_code_alone_under_sanitizers(tmp_path):
    exe = tmp_path / "fem_mass_check"
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "fem_mass_check.c"),
                           os.path.join(CSRC, "bfhip_eigs_mass.c"), os.path.join(CSRC, "bfhip_cheb.c"), "-o", str(exe), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout + out.stderr)[-3000:]
    assert "runtime error" not in out.stderr and "ERROR: AddressSanitizer" not in out.stderr


def test_the_measurement_record_holds_every_leg():
    """profiles/r22_lbo_consistent.json (tools/lbo_consistent_rate.py on one MI355X): the legs DESIGN.md section 28 quotes."""
    import json
    rec = json.load(open(os.path.join(ROOT, "profiles", "r22_lbo_consistent.json")))
    assert rec["n"] == 1 << 20 and rec["p"] == 64 and rec["reps"] >= 10
    legs = rec["legs"]
    for k in ("eigs_step", "mass_step", "two_products", "dual_product", "filter_step_mass", "call_lumped", "call_consistent"):
        assert legs[k]["ms"]["min"] <= legs[k]["ms"]["median"] <= legs[k]["ms"]["max"], k
    assert legs["mass_step"]["over_eigs_step"]["median"] > 0 and legs["dual_product"]["bit_equal_to_the_two_launches"] is True
    for name in ("lumped", "consistent"):
        b = rec["first_band"][name]
        assert b["converged"] == 48 and b["code"] == 0 and len(b["degrees"]) == b["iterations"] + 1
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 28." in text and "r22_lbo_consistent.json" in text
