"""Matrix-free Chebyshev covariance, the part that needs no GPU: the exported names and the info
struct's size, every argument check that comes before the device is touched, the Chebyshev fit and evaluation against a
numpy restatement, the P1 assembly of a triangle mesh against a numpy cotangent assembly, and the Gershgorin bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cheb_cases as cc
from butterfly_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("bfhipChebCovCreate", "bfhipChebCovSetCoefficients", "bfhipChebCovFree", "bfhipChebCovGetInfo", "bfhipChebFit", "bfhipChebEval",
         "bfhipTrimeshLboFemCount", "bfhipTrimeshLboFem", "bfhipChebCovApplyBlockDevice", "bfhipChebCovSampleBlockDevice",
         "bfhipChebCovMatvecBlockDevice", "bfhipChebCovDrawDevice", "bfhipChebCovMomentsDevice")


def ptr(a):
    return a.ctypes.data if a is not None else None


def test_the_new_names_are_exported_and_the_info_struct_has_the_c_size(tmp_path):
    import butterfly_amd
    from butterfly_amd.cheb import ChebCovariance
    lib = _capi.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    for name in NAMES:
        assert name + "(" in hdr, name
    for name in ("from_csr", "from_trimesh", "set_coefficients", "set_density", "apply_block_device", "sample_block_device",
                 "matvec_block_device", "draw_device", "moments_device", "info", "close"):
        assert callable(getattr(ChebCovariance, name)), name
    for name in ("ChebCovariance", "cheb_fit", "cheb_eval", "matern_density"):
        assert hasattr(butterfly_amd, name), name
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bfhip.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(BfhipChebCovInfo), '
                   'offsetof(BfhipChebCovInfo, lamMax), offsetof(BfhipChebCovInfo, errorEstimate));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    I = _capi.BfhipChebCovInfo
    assert got == [C.sizeof(I), I.lamMax.offset, I.errorEstimate.offset]


def create(n, rowptr, colind, data, mass, lam_max, out=True):
    lib = _capi.load()
    h = C.c_void_p()
    rc = lib.bfhipChebCovCreate(0, n, ptr(rowptr), ptr(colind), ptr(data), ptr(mass), lam_max, C.byref(h) if out else None)
    assert not h.value
    return rc


def test_create_refuses_bad_arguments_before_the_device_is_touched():
    u64 = lambda *v: np.array(v, dtype=np.uint64)
    rowptr, colind, data, mass = u64(0, 2, 2, 3), u64(0, 1, 2), np.array([1.0, -1.0, 2.0]), np.array([1.0, 2.0, 3.0])   # row 1 is empty: legal
    bad = [
        ("NULL rowptr", (3, None, colind, data, mass, 1.0)),
        ("NULL colind", (3, rowptr, None, data, mass, 1.0)),
        ("NULL data", (3, rowptr, colind, None, mass, 1.0)),
        ("n == 0", (0, rowptr, colind, data, mass, 1.0)),
        ("n >= 2^32", (1 << 32, rowptr, colind, data, mass, 1.0)),
        ("rowptr[0] != 0", (3, u64(1, 2, 2, 3), colind, data, mass, 1.0)),
        ("rowptr not monotone", (3, u64(0, 2, 1, 3), colind, data, mass, 1.0)),
        ("colind >= n", (3, rowptr, u64(0, 3, 2), data, mass, 1.0)),
        ("mass zero", (3, rowptr, colind, data, np.array([1.0, 0.0, 3.0]), 1.0)),
        ("mass negative", (3, rowptr, colind, data, np.array([1.0, -2.0, 3.0]), 1.0)),
        ("mass NaN", (3, rowptr, colind, data, np.array([1.0, np.nan, 3.0]), 1.0)),
        ("mass infinite", (3, rowptr, colind, data, np.array([1.0, np.inf, 3.0]), 1.0)),
        ("lamMax NaN", (3, rowptr, colind, data, mass, float("nan"))),
        ("lamMax +inf", (3, rowptr, colind, data, mass, float("inf"))),
        ("lamMax -inf", (3, rowptr, colind, data, None, float("-inf"))),
    ]
    for what, args in bad:
        assert create(*args) == INVALID, what
    assert create(3, rowptr, colind, data, mass, 1.0, out=False) == INVALID
    # S == 0 has no interval [0, lamMax] when the Gershgorin bound is asked for
    assert create(3, rowptr, colind, np.zeros(3), mass, 0.0) == INVALID


def test_entries_refuse_a_null_object_and_null_arguments():
    lib = _capi.load()
    buf = (C.c_double * 8)()
    p, q = C.addressof(buf), C.addressof(buf) + 32
    for fn in (lib.bfhipChebCovApplyBlockDevice, lib.bfhipChebCovSampleBlockDevice, lib.bfhipChebCovMatvecBlockDevice):
        assert fn(None, p, 1, q, None) == INVALID
    assert lib.bfhipChebCovDrawDevice(None, 1, 0, 1, p, None) == INVALID
    assert lib.bfhipChebCovMomentsDevice(None, 1, 0, 1, 1, p, q, None) == INVALID
    assert lib.bfhipChebCovSetCoefficients(None, p, 1) == INVALID
    info = _capi.BfhipChebCovInfo()
    info.structSize = C.sizeof(info)
    assert lib.bfhipChebCovGetInfo(None, C.byref(info)) == INVALID
    h = C.c_void_p()
    lib.bfhipChebCovFree(C.byref(h))            # freeing nothing is legal
    lib.bfhipChebCovFree(None)
    f = _capi.CHEB_DENSITY_FN(lambda x, _: x)
    coef = np.zeros(4)
    assert lib.bfhipChebFit(0, 0.0, 1.0, f, None, ptr(coef)) == INVALID
    assert lib.bfhipChebFit(4, 0.0, 1.0, f, None, None) == INVALID
    assert lib.bfhipChebFit(4, 0.0, 1.0, _capi.CHEB_DENSITY_FN(), None, ptr(coef)) == INVALID
    assert lib.bfhipChebFit(4, 1.0, 1.0, f, None, ptr(coef)) == INVALID
    assert lib.bfhipChebFit(4, 0.0, float("inf"), f, None, ptr(coef)) == INVALID
    assert np.isnan(lib.bfhipChebEval(0, 0.0, 1.0, ptr(coef), 0.5)) and np.isnan(lib.bfhipChebEval(4, 0.0, 1.0, None, 0.5))


def nodes(order):
    j = np.arange(order)
    return np.sin(np.pi * (2 * j + 1 - order) / (2 * order))


def fit_restated(f, order, a, b):
    """c_0 = (1 / order) sum_j y_j, c_k = (2 / order) sum_j T_k(x_j) y_j with T_k(x_j) = cos(k arccos x_j), summed in long double."""
    x = nodes(order)
    y = np.array([f((b - a) * (t + 1) / 2 + a) for t in x])
    k = np.arange(order)[:, None]
    T = np.cos(k.astype(cc.LD) * np.arccos(x.astype(cc.LD))[None, :])
    c = (T * y.astype(cc.LD)).sum(axis=1) * (cc.LD(2) / order)
    c[0] /= 2
    return c, x, y


@pytest.mark.parametrize("order", [1, 2, 3, 8, 64, 129])
def test_the_fit_matches_a_numpy_restatement_and_reproduces_f_at_the_nodes(order):
    from butterfly_amd import cheb_fit, cheb_eval, matern_density
    a, b = 0.0, 37.5
    for f in (matern_density(0.8, 2.0), matern_density(0.05, 0.0)):
        coef = cheb_fit(f, order, a, b)
        want, x, y = fit_restated(f, order, a, b)
        # per coefficient: the sum of `order` products |T_k| <= 1 times y_j, each T_k(x_j) within a few ulp of 1
        bound = 4 * 2.0 ** -52 * np.abs(y).sum()
        err = np.abs(coef.astype(cc.LD) - want).astype(np.float64)
        print(f"order {order}: fit error {err.max():.2e} (bound {bound:.2e})")
        assert (err <= bound).all()
        t = (b - a) * (x + 1) / 2 + a
        got = cheb_eval(coef, a, b, t)
        # The exact interpolant of the exact coefficients equals y at the nodes.  What is left: (1) the coefficients' own
        # error, at most `bound` each, times |T_k| <= 1: order * bound; (2) Clenshaw's rounding, by a running error
        # analysis: step k rounds three times on terms of size |c_k| + 2 |t| |b_{k+1}| + |b_{k+2}|, and an error made in b_k
        # reaches the result times |U_k(t)| <= min(k + 1, 1 / sqrt(1 - t^2))
        xs = (2 * t - a - b) / (b - a)
        amp = np.minimum(np.arange(order)[:, None] + 1.0, 1 / np.sqrt(1 - xs ** 2)[None, :])
        b1, b2, run = np.zeros(order), np.zeros(order), np.zeros(order)
        for k in range(order - 1, -1, -1):
            run += 3 * 2.0 ** -53 * amp[k] * (abs(coef[k]) + 2 * np.abs(xs * b1) + np.abs(b2))
            b1, b2 = coef[k] + 2 * xs * b1 - b2, b1
        err = np.abs(got - y)
        print(f"order {order}: worst error at a node {err.max():.2e} (bound {(run + order * bound).max():.2e})")
        assert (err <= run + order * bound).all()


def test_a_degree_5_polynomial_is_reproduced_everywhere_with_order_6():
    from butterfly_amd import cheb_fit, cheb_eval
    p = np.polynomial.Polynomial([0.3, -1.2, 0.5, 2.0, -0.7, 0.11])
    a, b = -1.5, 2.5
    coef = cheb_fit(p, 6, a, b)
    xs = np.linspace(a, b, 201)
    scale = np.abs(coef).sum()
    assert np.abs(cheb_eval(coef, a, b, xs) - p(xs)).max() <= 64 * 2.0 ** -52 * scale
    assert isinstance(cheb_eval(coef, a, b, 0.25), float)


@pytest.fixture(scope="module")
def mesh63():
    from butterfly_amd import trimesh_lbo_fem
    verts, faces = cc.jittered_grid_mesh()
    return verts, faces, trimesh_lbo_fem(verts, faces), cc.cotan_dense(verts, faces)


def test_the_assembler_matches_a_numpy_cotangent_assembly(mesh63):
    verts, faces, (rowptr, colind, data, mass), (Lref, mref, area) = mesh63
    n = 63
    assert len(verts) == n and rowptr[0] == 0 and len(rowptr) == n + 1 and rowptr[n] == len(colind) == len(data)
    deg = np.diff(rowptr.astype(np.int64))
    assert deg.min() == 3 and deg.max() == 7
    lib = _capi.load()
    nnz = C.c_uint64()
    assert lib.bfhipTrimeshLboFemCount(n, len(faces), ptr(faces), C.byref(nnz)) == 0 and nnz.value == rowptr[n]
    for i in range(n):
        row = colind[int(rowptr[i]):int(rowptr[i + 1])].astype(np.int64)
        assert (np.diff(row) > 0).all() and i in row                       # sorted, diagonal present
        assert set(row) == set(np.nonzero(Lref[i])[0]) | {i}
    L = cc.csr_to_dense(rowptr, colind, data, n)
    scale = np.abs(Lref).max()
    assert np.abs(L - Lref).max() <= 64 * 2.0 ** -52 * scale               # a handful of cotangents per entry, each a quotient
    assert np.abs(L - L.T).max() <= 16 * 2.0 ** -52 * scale
    assert np.abs(L @ np.ones(n)).max() <= 64 * 2.0 ** -52 * scale
    assert np.abs(mass - mref).max() <= 16 * 2.0 ** -52 * mref.max() and (mass > 0).all()
    assert abs(mass.sum() - area) <= 64 * 2.0 ** -52 * area


def test_the_assembler_refuses_bad_meshes():
    lib = _capi.load()
    verts, faces = cc.jittered_grid_mesh()
    n, nf = len(verts), len(faces)
    nnz = C.c_uint64()
    rowptr, colind, data, mass = np.zeros(n + 1, dtype=np.uint64), np.zeros(500, dtype=np.uint64), np.zeros(500), np.zeros(n)
    run = lambda v, f: lib.bfhipTrimeshLboFem(n, ptr(v), nf, ptr(f), ptr(rowptr), ptr(colind), ptr(data), ptr(mass))
    assert run(verts, faces) == 0
    bad = faces.copy(); bad[5, 1] = n
    assert run(verts, bad) == INVALID and lib.bfhipTrimeshLboFemCount(n, nf, ptr(bad), C.byref(nnz)) == INVALID
    bad = faces.copy(); bad[7, 2] = bad[7, 0]                                # a repeated vertex
    assert run(verts, bad) == INVALID
    flat = verts.copy(); flat[faces[3].astype(np.int64)] = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]     # collinear: zero area
    assert run(flat, faces) == INVALID
    assert run(None, faces) == INVALID
    assert lib.bfhipTrimeshLboFem(n, ptr(verts), nf, ptr(faces), None, ptr(colind), ptr(data), ptr(mass)) == INVALID
    assert lib.bfhipTrimeshLboFemCount(n, nf, ptr(faces), None) == INVALID
    assert lib.bfhipTrimeshLboFemCount(0, nf, ptr(faces), C.byref(nnz)) == INVALID


def test_the_gershgorin_bound_is_an_upper_bound_of_the_spectrum(mesh63):
    _, _, (rowptr, colind, data, mass), _ = mesh63
    val, d, gersh = cc.fold(rowptr, colind, data, mass)
    S = cc.csr_to_dense(rowptr, colind, val, 63)
    S = (S + S.T) / 2
    top = np.linalg.eigvalsh(S)[-1]
    print(f"Gershgorin {gersh:.6f}, largest eigenvalue {top:.6f}")
    assert gersh >= top > 0
