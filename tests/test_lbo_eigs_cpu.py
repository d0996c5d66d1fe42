"""The device eigensolver (bfhipChebCovEigsDevice), the part that needs no GPU: the exported names
and both structs' sizes against a compiled C program, every argument refusal in the header's order before a device is
touched, the conditions the cases of tests/eigs_cases.py must meet so that their choice cannot hide a failure, and the host
eigen-routine alone under AddressSanitizer and UBSan (tests/native/eigs_symeig_check.c, a program of its own)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eigs_cases as ec
from butterfly_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "butterfly_amd", "csrc")
INVALID = 1


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """sizeof / offsetof of the public structs, and where the private object keeps n (the refusals below read it)."""
    d = tmp_path_factory.mktemp("eigs_sz")
    src = d / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bfhip_internal.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(BfhipEigsOptions), offsetof(BfhipEigsOptions, tol), offsetof(BfhipEigsOptions, flags), sizeof(BfhipEigsInfo), '
                   'offsetof(BfhipEigsInfo, operatorColumns), offsetof(BfhipEigsInfo, lamMax), sizeof(struct BfhipChebCov), '
                   'offsetof(struct BfhipChebCov, n));return 0;}\n')
    exe = d / "sz"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src), "-o", str(exe)])
    return [int(v) for v in subprocess.check_output([str(exe)]).split()]


def test_the_new_names_are_exported_and_both_structs_have_the_c_layout(layout):
    from butterfly_amd.cheb import ChebCovariance
    lib = _capi.load()
    assert hasattr(lib, "bfhipChebCovEigsDevice") and hasattr(lib, "bfEigsSymEig")
    hdr = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    assert "bfhipChebCovEigsDevice(" in hdr and "bfEigsSymEig" not in hdr            # the eigen-routine is linkable, not public
    assert callable(ChebCovariance.eigs)
    fn = lib.bfhipChebCovEigsDevice
    assert fn.restype is C.c_int and len(fn.argtypes) == 9 and fn.argtypes[2] is C.c_size_t and fn.argtypes[6] is C.c_size_t
    O, I = _capi.BfhipEigsOptions, _capi.BfhipEigsInfo
    assert layout[:6] == [C.sizeof(O), O.tol.offset, O.flags.offset, C.sizeof(I), I.operatorColumns.offset, I.lamMax.offset]
    assert _capi.EIGS_MASS_NORMALISED == 1 and "#define BFHIP_EIGS_MASS_NORMALISED 1u" in hdr


def test_argument_refusals_come_in_order_before_a_device_is_touched(layout):
    """The object is a zeroed stand-in with only n set (device 0 is never entered: every call below returns before), the
    device pointer 0x1000 stands for "not NULL".  Each call breaks one rule and every later one too where it can, so the
    message shows which check came first."""
    lib = _capi.load()
    fn, msg = lib.bfhipChebCovEigsDevice, lib.bfhipLastErrorMessage
    size, off_n = layout[6], layout[7]

    def obj(n):
        buf = (C.c_char * size)()
        C.c_uint64.from_buffer(buf, off_n).value = n
        return buf

    def options(**kw):
        o = _capi.BfhipEigsOptions()
        o.structSize = C.sizeof(o)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    lam = np.full(256, -5.0)
    dU = C.c_void_p(0x1000)
    info = _capi.BfhipEigsInfo()
    info.structSize = C.sizeof(info)

    def refused(c, opt, nev, lam_p, du, ldu, want, inf=info):
        rc = fn(c, C.byref(opt) if opt is not None else None, nev, lam_p, None, du, ldu, C.byref(inf) if inf is not None else None, None)
        assert rc == INVALID and want in msg(), (rc, msg(), want)

    c100, bad_all = obj(100), options(structSize=3, guard=300, degree=1, tol=-1.0)
    L = lam.ctypes.data
    # 1. NULLs, before anything else (nev = 0, ldu = 0 and a bad struct ride along)
    refused(None, bad_all, 0, L, dU, 0, b"NULL")
    refused(c100, bad_all, 0, None, dU, 0, b"NULL")
    refused(c100, bad_all, 0, L, None, 0, b"NULL")
    # 2. nev
    refused(c100, bad_all, 0, L, dU, 0, b"nev out of range")
    refused(c100, bad_all, 101, L, dU, 0, b"nev out of range")           # > n
    refused(obj(1000), bad_all, 256, L, dU, 0, b"nev out of range")      # > 255
    # 3. ldu
    refused(c100, bad_all, 10, L, dU, 9, b"ldu")
    # 4. structSize, of either struct
    refused(c100, bad_all, 10, L, dU, 10, b"sizeof(BfhipEigsOptions)")
    bad_info = _capi.BfhipEigsInfo()
    bad_info.structSize = 8
    refused(c100, options(guard=300, degree=1, tol=-1.0), 10, L, dU, 10, b"sizeof(BfhipEigsInfo)", inf=bad_info)
    # 5. the guard
    refused(obj(1000), options(guard=247, degree=1, tol=-1.0), 10, L, dU, 10, b"more than 256")
    refused(c100, options(flags=_capi.EIGS_NO_GUARD, degree=1, tol=-1.0), 10, L, dU, 10, b"guard")          # explicit guard == 0, nev < n
    refused(c100, options(guard=91, degree=1, tol=-1.0), 10, L, dU, 10, b"more than n")
    # 6. degree
    refused(c100, options(guard=8, degree=1, tol=-1.0), 10, L, dU, 10, b"degree")
    # 7. tol
    for bad in (-1e-300, float("nan"), float("inf"), float("-inf")):
        refused(c100, options(guard=8, degree=2, tol=bad), 10, L, dU, 10, b"tol")
    assert (lam == -5.0).all() and info.iterations == 0 and info.blockColumns == 0      # nothing was written


@pytest.fixture(scope="module")
def mats():
    return ec.matrices()


def test_the_cases_are_the_ones_the_kernels_branch_on(mats):
    assert [mats[k].n for k in ("n1", "path5", "mesh63", "two_grids", "grid33", "graph4221")] == [1, 5, 63, 800, 1089, 4221]
    w = mats["wide_and_empty"]
    deg = np.diff(w.rowptr.astype(np.int64))
    assert deg.max() == 70 and deg.min() == 0 and w.mass is not None
    assert mats["two_grids"].mass is not None and np.ptp(mats["two_grids"].d) > 0.1           # D != 1
    assert mats["graph4221"].mass is None and 4221 > 4 * 1024                                    # crosses Gram chunks (1024 rows)
    ps = [ec.block_columns(mats[name].n, nev, guard) for name, nev, guard, _ in ec.CASES]
    assert ps == [1, 5, 3, 16, 9, 10, 24, 49, 77, 130, 20]
    assert 77 % 16 and 130 > 128 and 130 % 16 and 20 % 16 and 4221 % 4 and 1089 % 4               # ragged tiles, ragged rows
    lam, _ = mats["two_grids"].truth(3)
    assert abs(lam[0]) < 1e-12 and abs(lam[1]) < 1e-12 and lam[2] > 1e-4                        # lambda = 0 twice
    lam, V = mats["graph4221"].truth(130)
    assert (np.diff(lam) >= 0).all() and np.abs(V.T @ V - np.eye(130)).max() < 1e-12
    assert np.abs(mats["graph4221"].ell.mul(V) - V * lam).max() < 1e-12                          # the analytic truth is the truth
    lam, _ = mats["grid33"].truth(34)
    near = np.diff(lam[:33]) / mats["grid33"].lam_max
    assert (near < 1e-5).sum() >= 5                                                                # degenerate pairs inside the wanted set


@pytest.mark.parametrize("case", ec.CASES, ids=ec.case_id)
def test_every_case_has_a_gap_and_converges_in_the_restatement(mats, case):
    name, nev, guard, degree = case
    m = mats[name]
    if nev < m.n:
        lam, _ = m.truth(nev + 1)
        gap = (lam[nev] - lam[nev - 1]) / m.lam_max
        print(f"{ec.case_id(case)}: relative boundary gap {gap:.2e}")
        assert gap >= ec.MIN_GAP
    r = ec.reference_eigs(m, nev, guard, degree)
    print(f"{ec.case_id(case)}: p {r['p']}, {r['iterations']} iterations, largest degree {r['max_degree']}, worst cond(X^T X) {r['cond_max']:.1e}")
    assert r["converged"] == nev and r["iterations"] <= ec.MAX_REF_ITERS
    lam, _ = m.truth(nev)
    assert np.abs(r["lam"] - lam).max() <= 1e-10 * m.lam_max


def test_the_degree_cap_acts_on_the_63_vertex_mesh(mats):
    m = mats["mesh63"]
    capped = ec.reference_eigs(m, 8, 8, 20)
    free = ec.reference_eigs(m, 8, 8, 20, cap=False)
    print(f"largest degree with the cap {capped['max_degree']}; cond(X^T X) without it {free['cond_max']:.1e}, with it {capped['cond_max']:.1e}")
    assert capped["max_degree"] < 20 and free["cond_max"] > 1e15 > 2.0 ** 46 > capped["cond_max"]


def test_the_host_eigen_routine_alone_under_sanitizers(tmp_path):
    exe = tmp_path / "eigs_symeig_check"
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "eigs_symeig_check.c"),
                           os.path.join(CSRC, "bfhip_eigs.c"), "-o", str(exe), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout + out.stderr)[-3000:]
    assert "runtime error" not in out.stderr and "ERROR: AddressSanitizer" not in out.stderr
