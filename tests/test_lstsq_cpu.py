"""CPU side of the least-squares tests: the router (bfhipLstSqRoutes) and the catalogue's route coverage, the long-double
reference against two independent checks, the fp64 emulator of the device's rules against the bounds, the bounds' teeth
(mutants of the emulator must fail them), and the three suspects of the per-column freeze settled on the emulator."""
import ctypes as C

import numpy as np
import pytest

import lstsq_catalogue as cat
import lstsq_emulator as emu
import lstsq_ref as ref

_CASES = cat.catalogue()
_REF = {}


def _reference(c):
    if c["name"] not in _REF:
        _REF[c["name"]] = ref.reference(c["A"], c["B"])
    return _REF[c["name"]]


def _small(c):
    return c["ref"] == "ld"


def _plain_classes_by_brute_force():
    """Every (W, threads, LDS class, resident) of the plain Jacobi kernel the router emits, over every shape the kernel
    takes (me <= 2304, mt + me <= 4607) with the Gram form and the QR stage switched off, each with the shape (mt, me) of the
    smallest mt me^2 that reaches it (among equals: the fewest columns)."""
    from butterfly_amd import _capi
    from butterfly_amd.operator import _lstsq_options
    lib = _capi.load()
    opts = _lstsq_options(qr_min=cat.HUGE, gram_min=cat.HUGE, force_global=0)
    found = {}
    for me in range(1, 2305):
        mts = np.arange(1, 4608 - me + 1, dtype=np.uint32)
        sh = np.zeros((len(mts), 3), np.uint32)
        sh[:, 0], sh[:, 1], sh[:, 2] = mts, me, 1
        out = (_capi.BfhipLstSqRoute * len(mts))()
        assert lib.bfhipLstSqRoutes(len(mts), sh.ctypes.data, None, C.byref(opts), out) == 0
        r = np.frombuffer(out, dtype=np.uint32).reshape(-1, 8)
        plain = r[:, 3] == 0
        classes, first = np.unique(r[plain, 4:8], axis=0, return_index=True)       # mts ascend: the first is the shortest
        for k, mt in zip(map(tuple, classes.tolist()), mts[plain][first].tolist()):
            if k not in found or mt * me * me < found[k][0] * found[k][1] ** 2:
                found[k] = (mt, me)
    return found


# (W, threads, LDS class, resident) of the plain kernel -> the smallest shape (mt, me) routed to it, as the router stood
# when the tile geometry was its own copy of the kernel's: bfJacobiTile, which both now call, must reproduce it
_PLAIN_ROUTES = {
    (4, 256, 0, 1): (1, 1), (4, 256, 1, 1): (1, 31), (4, 256, 2, 1): (1, 45), (4, 256, 3, 1): (1, 63),
    (4, 1024, 3, 0): (1, 95), (4, 1024, 3, 1): (1, 65), (8, 256, 0, 1): (5, 1), (8, 256, 1, 1): (5, 29),
    (8, 256, 2, 1): (5, 43), (8, 256, 3, 0): (221, 35), (8, 256, 3, 1): (5, 61), (8, 1024, 3, 0): (5, 93),
    (8, 1024, 3, 1): (5, 65), (16, 256, 0, 1): (9, 1), (16, 256, 1, 1): (9, 27), (16, 256, 2, 1): (97, 17),
    (16, 256, 3, 0): (441, 19), (16, 256, 3, 1): (211, 17), (16, 1024, 3, 0): (9, 91), (16, 1024, 3, 1): (9, 65),
    (32, 256, 0, 1): (17, 1), (32, 256, 1, 1): (93, 9), (32, 256, 2, 1): (195, 9), (32, 256, 3, 0): (757, 11),
    (32, 256, 3, 1): (401, 9), (32, 1024, 3, 0): (17, 123), (64, 256, 0, 1): (33, 1), (64, 256, 1, 1): (511, 1),
    (64, 256, 2, 1): (1023, 1), (64, 256, 3, 0): (2301, 3), (64, 256, 3, 1): (2047, 1), (64, 1024, 3, 0): (207, 65),
}


def test_the_catalogue_reaches_every_reachable_route():
    from butterfly_amd.operator import lstsq_routes
    representatives = _plain_classes_by_brute_force()
    assert representatives == _PLAIN_ROUTES
    for (w, threads, lds, res), (mt, me) in _PLAIN_ROUTES.items():
        r = lstsq_routes([(mt, me, 1)], **cat.PLAIN)[0]
        assert (r["jacobi"], r["w"], r["threads"], r["ldsClass"], r["resident"]) == (0, w, threads, lds, res), (mt, me, r)
    reachable = set(representatives)
    assert reachable == set(cat.PLAIN_SHAPES)
    # the unreachable (W, threads, LDS) classes: 1024 threads only with the 144 KiB tile (catalogue docstring)
    wtl = {(w, t, l) for w, t, l, _ in reachable}
    assert len(wtl) == 25
    assert {(w, t, l) for w in (4, 8, 16, 32, 64) for t in (256, 1024) for l in range(4)} - wtl == \
        {(w, 1024, l) for w in (4, 8, 16, 32, 64) for l in range(3)}
    assert not [k for k in reachable if k[1] == 1024 and k[3] == 1 and k[0] > 16]
    reached, qr_classes, qr_paths, jacobi = set(), set(), set(), set()
    for c in _CASES:
        mt, me = c["A"].shape
        r = lstsq_routes([(mt, me, c["B"].shape[1])], ranks=[c["rank"]], **(c["opts"] or {}))[0]
        for k, v in c["route"].items():
            assert r[k] == v, (c["name"], k, r)
        if r["jacobi"] == 0:
            reached.add((r["w"], r["threads"], r["ldsClass"], r["resident"]))
        jacobi.add(r["jacobi"])
        if r["qr"]:
            qr_classes.add(r["qrLdsClass"])
            qr_paths.add(r["qrStreaming"])
    assert reached == reachable
    assert jacobi == {0, 1, 2} and qr_classes == set(range(6)) and qr_paths == {0, 1}
    # the other edges the catalogue promises
    shapes = [c["A"].shape for c in _CASES]
    assert any(me == 1 for _, me in shapes) and any(me == 2 for _, me in shapes) and any(mt == 1 for mt, _ in shapes)
    assert any(mt < me for mt, me in shapes) and any(me % 2 for _, me in shapes)
    grams = [c["A"].shape for c in _CASES if c["route"].get("jacobi") == 1]
    assert any(me % 16 for _, me in grams) and any(mt % 32 for mt, _ in grams)
    assert any(c["rank"] == 0 for c in _CASES if c["route"].get("qr") == 1)
    assert any(0 < c["rank"] < min(c["A"].shape) for c in _CASES)


def test_routes_follow_the_options_and_the_environment(monkeypatch):
    from butterfly_amd.operator import lstsq_routes
    assert lstsq_routes([(200, 100, 1)])[0]["qr"] == 1
    assert lstsq_routes([(200, 100, 1)], qr_min=101)[0]["qr"] == 0
    monkeypatch.setenv("BFHIP_JACOBI_QR_MIN", "1000")
    assert lstsq_routes([(200, 100, 1)])[0]["qr"] == 0
    assert lstsq_routes([(200, 100, 1)], qr_min=0)[0]["qr"] == 1             # the options override the environment
    monkeypatch.setenv("BFHIP_JACOBI_GLOBAL", "1")
    assert lstsq_routes([(40, 20, 1)])[0]["jacobi"] == 2
    assert lstsq_routes([(40, 20, 1)], force_global=0)[0]["jacobi"] == 0
    monkeypatch.setenv("BFHIP_JACOBI_GRAM_MIN", "0")
    assert lstsq_routes([(40, 20, 1)], force_global=0)[0]["jacobi"] == 1
    with pytest.raises(ValueError):
        lstsq_routes([(0, 3, 1)])


@pytest.mark.parametrize("c", [c for c in _CASES if c["gap"] and c["rank"] and c["X_design"] is not None and _small(c)],
                         ids=lambda c: c["name"])
def test_reference_against_designed_factors_and_lapack(c):
    from oracle import helm2_build as hb
    X, s, k = _reference(c)
    assert k == c["rank"]
    Xd = np.asarray(c["X_design"], dtype=np.complex128)
    bound = ref.x_bound(c["A"], c["B"], X, s)
    # the factors: off the stored matrix by its rounding, u ||A|| -- within the bound, not bit-exact
    assert np.linalg.norm(np.asarray(X, dtype=np.complex128) - Xd) <= bound, c["name"]
    # LAPACK zgesvd in fp64
    Xl = hb.lstsq_truncated(c["A"], c["B"])
    assert np.linalg.norm(np.asarray(X, dtype=np.complex128) - Xl) <= bound, c["name"]
    sl = np.linalg.svd(c["A"], compute_uv=False)[:k]
    assert np.max(np.abs(s - sl)) <= ref.sigma_bound(c["A"], s)


def _emulated(c, **kw):
    return emu.solve(c["A"], c["B"], qr=c["route"].get("qr", 0) == 1, **kw)


def _within(c, X, sig, rank):
    Xr, sr, kr = _reference(c)
    if rank != kr or len(sig) != len(sr):
        return False
    if kr and np.max(np.abs(sig - sr)) > ref.sigma_bound(c["A"], sr):
        return False
    if c["gap"]:
        return bool(np.linalg.norm(X - np.asarray(Xr, dtype=np.complex128)) <= ref.x_bound(c["A"], c["B"], Xr, sr))
    return True


_GAP_SMALL = [c for c in _CASES if _small(c) and (c["gap"] or c["name"].startswith("near"))]


@pytest.mark.parametrize("c", _GAP_SMALL, ids=lambda c: c["name"])
def test_emulator_meets_the_bounds(c):
    for qr in (False, True):
        X, sig, rank, flagged = emu.solve(c["A"], c["B"], qr=qr)
        assert not flagged and rank == c["rank"], (c["name"], qr, rank)
        assert _within(c, X, sig, rank), (c["name"], qr)


def test_mutants_fail_the_bounds():
    """Each deliberate mistake in the emulator is caught by the bounds on some catalogue case -- and none of them passes
    everywhere unnoticed."""
    caught = {}
    for m in ("phase", "short", "thresh2x", "drop"):
        caught[m] = [c["name"] for c in _GAP_SMALL
                     if not _within(c, *_emulated(c, mutant=m)[:3])]
    assert all(caught.values()), caught
    assert "near-threshold-24x10" in caught["thresh2x"]


def test_suspect1_subthreshold_columns_confirmed_and_fixed():
    c = [c for c in _CASES if c["name"].startswith("suspect1")][0]
    X, s, k = _reference(c)
    assert k == 2
    for qr in (False, True):
        Xo, so, ko, _ = emu.solve(c["A"], c["B"], qr=qr, freeze="each", qr_stop="max")
        assert ko == 1, qr                                    # the old rules: rank 1 ...
        r_old = np.linalg.norm(c["A"] @ Xo[:, :1] - c["B"][:, :1])
        assert r_old > 0.99                                   # ... and a residual of 1 for B = e2
        Xn, sn, kn, _ = emu.solve(c["A"], c["B"], qr=qr)
        assert kn == 2 and _within(c, Xn, sn, kn), qr         # the sum rule: the reference's answer


def test_suspect2_nan_on_the_plain_path_confirmed_and_fixed():
    c = [c for c in _CASES if c["name"] == "gemm-49x33x31"][0]
    A = c["A"].copy()
    A[3, 5] = np.nan
    # old rules: no flag (the QR route counted the same input as a failure) -- but X is not the finite a_j^H B / |a_j|^2
    # the issue feared: the NaN column's scale is 0, and 0 x NaN in the first GEMM poisons every entry of X through V T
    X, _, _, flagged = emu.solve(A, c["B"], finish="fmax", freeze="each")
    assert not flagged and not np.any(np.isfinite(X))
    assert emu.solve(A, c["B"], qr=True, finish="fmax", freeze="each", qr_stop="max")[3]
    for qr in (False, True):
        assert emu.solve(A, c["B"], qr=qr)[3]                # now flagged on both routes


def test_suspect3_underflow_confirmed_and_fixed():
    c = [c for c in _CASES if c["name"] == "underflow-30x20"][0]
    assert _reference(c)[2] == 0
    assert emu.solve(c["A"], c["B"], qr=True, qr_rank0="fail")[3]      # old: the QR route called it a failure
    for qr in (False, True):
        X, sig, rank, flagged = emu.solve(c["A"], c["B"], qr=qr)
        assert rank == 0 and not flagged and np.array_equal(X, np.zeros_like(X))
