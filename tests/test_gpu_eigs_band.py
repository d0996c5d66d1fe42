"""Successive eigenbands on the device (bfhipChebCovEigsBandDevice) on the chains of
tests/eigsband_cases.py.  Every chain runs twice, each time into ONE device array dAll [n, T] with T odd and larger than the
total, filled with a sentinel: call k passes the columns found so far as the locked block and dAll + m as its output.  Per band,
with the bounds of tests/test_gpu_lbo_eigs.py: the return code, residuals recomputed in numpy float64, eigenvalues index by
index against the truth, the subspace, ascending values across the boundaries, ||U_all^T U_all - I||_max against the float64
restatement's own value, the restatement's iteration count, the columns right of the band still the sentinel, the locked
columns bit-unchanged, and the second run's bytes equal to the first's.  Across the chains: a call with nothing locked against
bfhipChebCovEigsDevice bit for bit, the in-place mass normalisation against one IEEE multiplication, ChebCovariance.eigs_bands
to 320 pairs against the analytic spectrum, a live conditioning object, and the C example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eigs_cases as ec
import eigsband_cases as eb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = eb.U53
SENT = -7.25


def options(guard, degree, flags=0):
    from butterfly_amd import _capi
    opt = _capi.BfhipEigsOptions()
    opt.structSize = C.sizeof(opt)
    opt.guard, opt.degree = guard or 0, degree or 0
    opt.flags = flags | (_capi.EIGS_NO_GUARD if guard == 0 else 0)
    return opt


def band_call(obj, dAll, T, lam_all, m, nev, guard, degree, null_locked=False):
    """One call in the aliased layout: (rc, lam, residual, info dict).  dAll is written in place."""
    import torch
    from butterfly_amd import _capi
    lib = _capi.load()
    opt = options(guard, degree)
    info = _capi.BfhipEigsInfo()
    info.structSize = C.sizeof(info)
    lk = _capi.BfhipEigsLocked()
    lk.structSize, lk.count, lk.dVectors, lk.ld, lk.lam = C.sizeof(lk), m, dAll.data_ptr(), T, lam_all.ctypes.data
    lam, res = np.full(nev, np.nan), np.full(nev, np.nan)
    rc = lib.bfhipChebCovEigsBandDevice(obj.handle, C.byref(opt), None if null_locked else C.byref(lk), nev, lam.ctypes.data, res.ctypes.data,
                                        C.c_void_p(dAll.data_ptr() + 8 * m), T, C.byref(info), C.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    return rc, lam, res, info.as_dict()


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


def run_chain(obj, n, chain):
    """The chain on the device: list per band of (rc, lam, res, info, the whole dAll on the host after the call), and (dAll, T, lam_all)."""
    import torch
    _, bands, _, degree = chain
    total = sum(bands)
    T = total + 3 if total % 2 == 0 else total + 2
    dAll = torch.full((n, T), SENT, dtype=torch.float64, device="cuda:0")
    lam_all, out, m = np.zeros(total), [], 0
    for k, nev in enumerate(bands):
        rc, lam, res, info = band_call(obj, dAll, T, lam_all, m, nev, eb.guard_of(chain, k), degree)
        lam_all[m:m + nev] = lam
        out.append((rc, lam, res, info, dAll.cpu().numpy()))
        m += nev
    return out, (dAll, T, lam_all)


@pytest.fixture(scope="module")
def chains(objects):
    made = {}

    def get(chain):
        if chain not in made:
            m, obj = objects(chain[0])
            a, dev = run_chain(obj, m.n, chain)
            b, _ = run_chain(obj, m.n, chain)
            total = sum(chain[1])
            lam, V = m.truth(min(m.n, total + 2))
            made[chain] = dict(m=m, a=a, b=b, dev=dev, ref=eb.reference_chain(chain), lam=lam, V=V)
        return made[chain]
    return get


@pytest.mark.parametrize("chain", eb.CHAINS, ids=eb.chain_id)
def test_every_band_of_the_chain(chains, chain):
    name, bands, _, degree = chain
    r = chains(chain)
    m, lam_true, V = r["m"], r["lam"], r["V"]
    lam_ref, U_ref, runs_ref = r["ref"]
    lam_max, total = m.lam_max, sum(bands)
    T = r["dev"][1]
    assert T % 2 == 1 and T > total
    done, prev = 0, None
    for k, nev in enumerate(bands):
        rc, theta, res, info, A = r["a"][k]
        tag = f"{eb.chain_id(chain)} band {k} (m = {done})"
        p = info["blockColumns"]
        U = A[:, done:done + nev]
        # 1. the call, the layout
        assert rc == 0 and info["converged"] == nev and p == eb.block_columns(m.n, done, nev, eb.guard_of(chain, k)) and info["lamMax"] == lam_max
        assert np.isfinite(U).all() and np.isfinite(theta).all() and (np.diff(theta) >= 0).all()
        assert info["operatorColumns"] >= p and info["workspaceBytes"] > 0 and info["maxDegreeUsed"] <= (degree or 20)
        assert (A[:, done + nev:] == SENT).all()                                     # nothing right of the band was written
        if prev is not None:
            assert A[:, :done].tobytes() == prev[:, :done].tobytes()                  # the locked columns are only read
            assert theta[0] >= r["a"][k - 1][1][-1]                                   # ascending across the boundary
        print(f"{tag}: p {p}, {info['iterations']} iterations (restatement {runs_ref[k]['iterations']}), largest degree {info['maxDegreeUsed']} "
              f"(restatement {runs_ref[k]['max_degree']}), max residual / lamMax {info['maxResidual']:.2e}")
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
        err = np.abs(theta - lam_true[done:done + nev])
        print(f"{tag}: eigenvalue error {err.max():.2e} (allowed {RF + 2 * p * U53 * lam_max:.2e})")
        assert (err <= RF + 2 * p * U53 * lam_max).all()
        # 4. the subspace: nothing of the band lies above the truth's pairs up to the boundary (up to the end of the double
        #    eigenvalue where the boundary cuts it)
        hi = eb.truth_extent(lam_true, done + nev, lam_max)
        assert hi == done + nev + ((name, k) == eb.SPLIT)
        if hi < m.n:
            delta = lam_true[hi] - theta.max()
            assert delta > 0
            Vh = V[:, :hi]
            out = np.linalg.norm(U - Vh @ (Vh.T @ U))
            print(f"{tag}: ||(I - P) U||_F {out:.2e} (allowed {RF / delta + p * 2 * U53:.2e})")
            assert out <= RF / delta + p * 2 * U53
        # 5. orthonormality of everything found so far, against the restatement's
        e_ref = eb.orthonormality(U_ref[:, :done + nev])
        bound = 8 * max(e_ref, (done + p) * U53)
        e_dev = eb.orthonormality(A[:, :done + nev])
        print(f"{tag}: ||U_all^T U_all - I||_max {e_dev:.2e}, restatement {e_ref:.2e} (allowed {bound:.2e})")
        assert e_dev <= bound
        # 6. the restatement's iteration count
        assert info["iterations"] == runs_ref[k]["iterations"]
        # 7. repeats
        rcb, thetab, resb, infob, B = r["b"][k]
        assert rcb == 0 and theta.tobytes() == thetab.tobytes() and res.tobytes() == resb.tobytes() and A.tobytes() == B.tobytes() and infob == info
        done, prev = done + nev, A
    if name == "path5":
        assert r["a"][1][3]["iterations"] == 0 and r["a"][1][3]["maxDegreeUsed"] == 0 and r["a"][1][3]["blockColumns"] == 3     # exact, no filter


def test_nothing_locked_is_the_single_call_bit_for_bit(objects):
    import torch
    from butterfly_amd import _capi
    lib = _capi.load()
    m, obj = objects("graph4221")
    nev, guard, degree = 64, 13, 60
    opt = options(guard, degree)
    info = _capi.BfhipEigsInfo()
    info.structSize = C.sizeof(info)
    lam0, res0 = np.full(nev, np.nan), np.full(nev, np.nan)
    dU = torch.full((m.n, nev), SENT, dtype=torch.float64, device="cuda:0")
    assert lib.bfhipChebCovEigsDevice(obj.handle, C.byref(opt), nev, lam0.ctypes.data, res0.ctypes.data, C.c_void_p(dU.data_ptr()), nev, C.byref(info),
                                      C.c_void_p(torch.cuda.current_stream(0).cuda_stream)) == 0
    U0, info0 = dU.cpu().numpy(), info.as_dict()
    for null_locked in (False, True):
        dB = torch.full((m.n, nev), SENT, dtype=torch.float64, device="cuda:0")
        rc, lam, res, inf = band_call(obj, dB, nev, np.zeros(nev), 0, nev, guard, degree, null_locked=null_locked)
        assert rc == 0 and lam.tobytes() == lam0.tobytes() and res.tobytes() == res0.tobytes() and dB.cpu().numpy().tobytes() == U0.tobytes()
        assert inf == info0


def test_mass_normalisation_in_place_is_one_multiplication(objects, chains):
    import torch
    from butterfly_amd import _capi
    lib = _capi.load()
    chain = eb.CHAINS[2]                                                   # two_grids: D != 1
    r = chains(chain)
    m, obj = objects("two_grids")
    dAll, T, _ = r["dev"]
    total = sum(chain[1])
    work = dAll.clone()
    before = work.cpu().numpy()
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    assert lib.bfhipChebCovEigsMassNormaliseDevice(obj.handle, C.c_void_p(work.data_ptr()), T, total, stream) == 0
    after = work.cpu().numpy()
    assert np.ptp(m.d) > 0.1
    assert after[:, :total].tobytes() == np.ascontiguousarray(m.d[:, None] * before[:, :total]).tobytes()
    assert (after[:, total:] == SENT).all()
    e = np.abs(after[:, :total].T @ (m.mass[:, None] * after[:, :total]) - np.eye(total)).max()
    print(f"||Phi^T M Phi - I||_max {e:.2e}")
    assert e <= 8 * max(eb.orthonormality(r["ref"][1]), (total + 31) * U53)
    # a column count below the leading dimension and an offset start: columns 1 .. 16 alone
    work = dAll.clone()
    assert lib.bfhipChebCovEigsMassNormaliseDevice(obj.handle, C.c_void_p(work.data_ptr() + 8), T, 16, stream) == 0
    after = work.cpu().numpy()
    assert after[:, 1:17].tobytes() == np.ascontiguousarray(m.d[:, None] * before[:, 1:17]).tobytes()
    assert after[:, :1].tobytes() == before[:, :1].tobytes() and after[:, 17:].tobytes() == before[:, 17:].tobytes()


def test_eigs_bands_to_320_pairs_against_the_analytic_spectrum(objects, chains):
    m, obj = objects("graph4221")
    lam, U, infos = obj.eigs_bands(320, band=64, guard=13, degree=60)
    lam_true, _ = m.truth(321)
    U = U.cpu().numpy()
    assert lam.shape == (320,) and U.shape == (m.n, 320) and len(infos) == 5 and all(i["code"] == 0 and i["converged"] == 64 for i in infos)
    R = m.ell.mul(U) - U * lam
    err, allowed = np.abs(lam - lam_true[:320]).max(), np.linalg.norm(R) + 2 * 77 * U53 * m.lam_max
    e_ref = eb.orthonormality(eb.reference_chain(eb.CHAINS[0])[1][:, :320])
    e_dev = eb.orthonormality(U)
    print(f"320 pairs in 5 bands: eigenvalue error {err:.2e} (allowed {allowed:.2e}), ||U^T U - I||_max {e_dev:.2e} (restatement {e_ref:.2e}), "
          f"iterations {[i['iterations'] for i in infos]}, degrees {[i['maxDegreeUsed'] for i in infos]}")
    assert (np.diff(lam) >= 0).all() and err <= allowed and e_dev <= 8 * max(e_ref, (256 + 77) * U53)
    # the same bits as the chain of raw calls (the first five bands of chain 0)
    A = chains(eb.CHAINS[0])["a"][4][4]
    assert U.tobytes() == np.ascontiguousarray(A[:, :320]).tobytes()
    # a ragged last band and the mass normalisation at the end, on a mesh with D != 1
    m2, obj2 = objects("two_grids")
    lam2, U2, infos2 = obj2.eigs_bands(40, band=17)
    lam2b, Phi, _ = obj2.eigs_bands(40, band=17, mass_normalised=True)
    U2, Phi = U2.cpu().numpy(), Phi.cpu().numpy()
    assert [i["blockColumns"] for i in infos2] == [25, 25, 14] and all(i["code"] == 0 for i in infos2)
    assert lam2.tobytes() == lam2b.tobytes() and Phi.tobytes() == np.ascontiguousarray(m2.d[:, None] * U2).tobytes()
    R2 = m2.ell.mul(U2) - U2 * lam2
    e_ref2 = eb.orthonormality(eb.reference_chain(("two_grids", (17, 17, 6), None, None))[1])
    e = np.abs(Phi.T @ (m2.mass[:, None] * Phi) - np.eye(40)).max()
    print(f"two_grids 17+17+6: ||Phi^T M Phi - I||_max {e:.2e} (restatement {e_ref2:.2e})")
    assert e <= 8 * max(e_ref2, (34 + 25) * U53) and np.abs(lam2 - m2.truth(40)[0]).max() <= np.linalg.norm(R2) + 2 * 25 * U53 * m2.lam_max
    # eigs_band with an [n, m] view of its own and a fresh output
    lam3, U3, info3 = obj.eigs_band(64, (torch_view(U[:, :64]), lam[:64]), guard=13, degree=60)
    assert info3["code"] == 0 and lam3.tobytes() == lam[64:128].tobytes()


def torch_view(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def test_a_live_conditioning_object_is_not_disturbed(objects, chains):
    import torch
    from butterfly_amd import matern_density
    chain = eb.CHAINS[2]
    m, obj = objects("two_grids")
    dAll, T, lam_all = chains(chain)["dev"]
    obj.set_density(matern_density(0.9, 1.5), 24)
    gen = np.random.default_rng(5)
    obs = gen.choice(m.n, 40, replace=False).astype(np.uint64)
    cond = obj.condition(obs, np.full(40, 0.05))
    y = torch.from_numpy(gen.standard_normal(40)).to("cuda:0")
    before = cond.mean(y).cpu().numpy()
    work = obj.info()["workspaceBytes"]
    scratch = dAll.clone()
    rc, *_ = band_call(obj, scratch, T, lam_all, 17, 23, None, None)
    assert rc == 0
    after = cond.mean(y).cpu().numpy()
    cond.close()
    assert before.tobytes() == after.tobytes() and obj.info()["workspaceBytes"] == work and obj.info()["order"] == 24
    assert scratch.cpu().numpy().tobytes() == dAll.cpu().numpy().tobytes()               # and the band came out the same


def test_the_c_example_builds_with_werror_and_exits_zero(tmp_path):
    lib = os.path.join(ROOT, "butterfly_amd", "csrc")
    exe = str(tmp_path / "lbo_bands_device")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "lbo_bands_device.c"), "-L", lib, "-lbfhip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-lm", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0
    assert "band 2" in p.stdout and "l(l+1)" in p.stdout
