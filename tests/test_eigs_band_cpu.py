"""Successive eigenbands by deflation (bfhipChebCovEigsBandDevice), the part that needs no GPU: the
exported names and BfhipEigsLocked against a compiled C program, every refusal in the header's order before a device is
touched, the conditions the chains of tests/eigsband_cases.py must meet so that their choice cannot hide a failure, the degree
cap with a locked eigenvalue, and what each omission a deflation kernel could make does to the cross-orthogonality bound of
tests/test_gpu_eigs_band.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eigs_cases as ec
import eigsband_cases as eb
from butterfly_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "butterfly_amd", "csrc")
INVALID = 1


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("eigsband_sz")
    src = d / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bfhip_internal.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(BfhipEigsLocked), offsetof(BfhipEigsLocked, count), offsetof(BfhipEigsLocked, dVectors), offsetof(BfhipEigsLocked, ld), '
                   'offsetof(BfhipEigsLocked, lam), sizeof(struct BfhipChebCov), offsetof(struct BfhipChebCov, n), '
                   'offsetof(struct BfhipChebCov, lamMax), sizeof(BfhipEigsOptions));return 0;}\n')
    exe = d / "sz"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src), "-o", str(exe)])
    return [int(v) for v in subprocess.check_output([str(exe)]).split()]


def test_the_new_names_are_exported_and_the_struct_has_the_c_layout(layout):
    from butterfly_amd.cheb import ChebCovariance
    lib = _capi.load()
    for name in ("bfhipChebCovEigsBandDevice", "bfhipChebCovEigsMassNormaliseDevice", "bfdevEigsCrossGram", "bfdevEigsDeflate", "bfdevEigsProject",
                 "bfdevEigsCrossChunkRows"):
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    assert "bfhipChebCovEigsBandDevice(" in hdr and "bfhipChebCovEigsMassNormaliseDevice(" in hdr and "bfdevEigs" not in hdr
    assert callable(ChebCovariance.eigs_band) and callable(ChebCovariance.eigs_bands)
    fn = lib.bfhipChebCovEigsBandDevice
    assert fn.restype is C.c_int and len(fn.argtypes) == 10 and fn.argtypes[3] is C.c_size_t and fn.argtypes[7] is C.c_size_t
    K = _capi.BfhipEigsLocked
    assert layout[:5] == [C.sizeof(K), K.count.offset, K.dVectors.offset, K.ld.offset, K.lam.offset]
    assert layout[8] == C.sizeof(_capi.BfhipEigsOptions)                       # the options keep their layout


def test_refusals_come_in_order_before_a_device_is_touched(layout):
    """A zeroed stand-in object with n and lamMax set; 0x1000 stands for a device pointer.  Each call breaks one rule and every
    later one where it can, so the message shows which check came first: section 25's with n - m for n, then the locked block's."""
    lib = _capi.load()
    fn, msg = lib.bfhipChebCovEigsBandDevice, lib.bfhipLastErrorMessage
    size, off_n, off_lam = layout[5], layout[6], layout[7]

    def obj(n, lam_max=4.0):
        buf = (C.c_char * size)()
        C.c_uint64.from_buffer(buf, off_n).value = n
        C.c_double.from_buffer(buf, off_lam).value = lam_max
        return buf

    def options(**kw):
        o = _capi.BfhipEigsOptions()
        o.structSize = C.sizeof(o)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    good_lam = np.linspace(0.0, 1.0, 64)
    held = []

    def locked(count, vectors=0x2000, ld=None, lam=good_lam, struct_size=None):
        k = _capi.BfhipEigsLocked()
        k.structSize = C.sizeof(k) if struct_size is None else struct_size
        k.count, k.dVectors, k.ld = count, vectors, count if ld is None else ld
        k.lam = lam.ctypes.data if lam is not None else None
        held.append(lam)
        return k

    lam = np.full(256, -5.0)
    L, dU = lam.ctypes.data, C.c_void_p(0x1000)
    info = _capi.BfhipEigsInfo()
    info.structSize = C.sizeof(info)

    def refused(c, opt, lk, nev, lam_p, du, ldu, want, inf=info):
        rc = fn(c, C.byref(opt) if opt is not None else None, C.byref(lk) if lk is not None else None, nev, lam_p, None, du, ldu,
                C.byref(inf) if inf is not None else None, None)
        assert rc == INVALID and want in msg(), (rc, msg(), want)

    c100 = obj(100)
    bad_all = options(structSize=3, guard=300, degree=1, tol=-1.0, flags=_capi.EIGS_MASS_NORMALISED)
    nan_lam = good_lam.copy(); nan_lam[7] = np.nan
    bad_lk = locked(40, vectors=None, ld=3, lam=nan_lam)                       # breaks every later locked rule it can
    # 1. section 25's refusals, in its order, with n - m = 60 in place of n
    refused(None, bad_all, bad_lk, 0, L, dU, 0, b"NULL")
    refused(c100, bad_all, bad_lk, 0, None, dU, 0, b"NULL")
    refused(c100, bad_all, bad_lk, 0, L, None, 0, b"NULL")
    refused(c100, bad_all, bad_lk, 0, L, dU, 0, b"nev out of range")
    refused(c100, bad_all, bad_lk, 61, L, dU, 0, b"nev out of range")                      # <= n, > n - m
    refused(obj(1000), bad_all, bad_lk, 256, L, dU, 0, b"nev out of range")
    refused(c100, bad_all, bad_lk, 10, L, dU, 9, b"ldu")
    refused(c100, bad_all, bad_lk, 10, L, dU, 10, b"sizeof(BfhipEigsOptions)")
    bad_info = _capi.BfhipEigsInfo()
    bad_info.structSize = 8
    rest = dict(degree=1, tol=-1.0, flags=_capi.EIGS_MASS_NORMALISED)
    refused(c100, options(guard=300, **rest), bad_lk, 10, L, dU, 10, b"sizeof(BfhipEigsInfo)", inf=bad_info)
    refused(obj(1000), options(guard=247, **rest), bad_lk, 10, L, dU, 10, b"more than 256")
    refused(c100, options(degree=1, tol=-1.0, flags=_capi.EIGS_MASS_NORMALISED | _capi.EIGS_NO_GUARD), bad_lk, 10, L, dU, 10, b"guard")
    refused(c100, options(guard=51, **rest), bad_lk, 10, L, dU, 10, b"more than n")        # 61 <= n, > n - m
    refused(c100, options(guard=8, **rest), bad_lk, 10, L, dU, 10, b"degree")
    for bad in (-1e-300, float("nan"), float("inf"), float("-inf")):
        refused(c100, options(guard=8, degree=2, tol=bad, flags=_capi.EIGS_MASS_NORMALISED), bad_lk, 10, L, dU, 10, b"tol")
    # 2. the locked block's
    mn = options(guard=8, degree=2, flags=_capi.EIGS_MASS_NORMALISED)
    refused(c100, mn, locked(40, vectors=None, ld=3, lam=nan_lam, struct_size=16), 10, L, dU, 10, b"sizeof(BfhipEigsLocked)")
    refused(c100, mn, bad_lk, 10, L, dU, 10, b"NULL dVectors or lam")
    refused(c100, mn, locked(40, ld=3, lam=None), 10, L, dU, 10, b"NULL dVectors or lam")
    refused(c100, mn, locked(40, ld=39, lam=nan_lam), 10, L, dU, 10, b"ld is less than count")
    # count >= n cannot pass section 25's nev test (n - m is 0 there), so it is refused there, as an argument error all the same
    refused(c100, mn, locked(100, lam=np.zeros(100)), 1, L, dU, 10, b"nev out of range")
    refused(c100, mn, locked(40, lam=nan_lam), 10, L, dU, 10, b"eigenvalue 7 is not finite or lies above lamMax")
    for v in (np.inf, -np.inf, 4.0 + 1e-12):
        bad = good_lam.copy(); bad[39] = v
        refused(c100, mn, locked(40, lam=bad), 10, L, dU, 10, b"eigenvalue 39 is not finite or lies above lamMax")
    refused(c100, mn, locked(40), 10, L, dU, 10, b"BFHIP_EIGS_MASS_NORMALISED")
    assert (lam == -5.0).all() and info.iterations == 0 and info.blockColumns == 0      # nothing was written
    # 3. the mass normalisation
    nm = lib.bfhipChebCovEigsMassNormaliseDevice
    assert nm(None, dU, 4, 4, None) == INVALID and b"NULL" in msg()
    assert nm(c100, None, 4, 4, None) == INVALID and b"NULL" in msg()
    assert nm(c100, dU, 3, 4, None) == INVALID and b"ldu is less than count" in msg()
    assert nm(c100, dU, 3, 0, None) == 0                                               # nothing to do: no device either


@pytest.fixture(scope="module")
def mats():
    return ec.matrices()


def test_the_chains_reach_the_branches_they_name(mats):
    ps = {eb.chain_id(ch): [eb.block_columns(mats[ch[0]].n, sum(ch[1][:k]), nev, eb.guard_of(ch, k)) for k, nev in enumerate(ch[1])] for ch in eb.CHAINS}
    assert ps["graph4221-64+64+64+64+64+30"] == [77] * 5 + [43] and ps["graph4221-120+120+120"] == [130] * 3
    assert ps["two_grids-1+16+23"] == [9, 24, 31] and ps["path5-2+3"] == [3, 3] and ps["mesh63-8+8"] == [9, 9] and ps["grid33-33+21"] == [41, 29]
    assert sum(eb.CHAINS[0][1]) == 350 > 255                                             # past the single call's limit
    assert [len(eb.panels_of(m)) for m in (64, 256, 257, 320)] == [1, 1, 2, 2]          # locked counts of chain 0: one and two panels
    assert eb.panels_of(320) == [(0, 256), (256, 320)]
    assert len(eb.cross_chunks_of(4221, 80)) == 5 and len(eb.cross_chunks_of(63, 16)) == 1
    assert mats["path5"].n - 2 == 3                                                      # nev = n - m: exact, no filter
    lam, _ = mats["two_grids"].truth(3)
    assert abs(lam[0]) < 1e-12 and abs(lam[1]) < 1e-12 and lam[2] > 1e-4                 # the first boundary cuts lambda = 0 twice


@pytest.mark.parametrize("chain", eb.CHAINS, ids=eb.chain_id)
def test_every_band_has_a_gap_and_converges_in_the_restatement(mats, chain):
    name, bands, _, degree = chain
    m = mats[name]
    total = sum(bands)
    lam, _ = m.truth(min(m.n, total + 1))
    lam_r, U_r, runs = eb.reference_chain(chain)
    done = 0
    for k, nev in enumerate(bands):
        done += nev
        r = runs[k]
        if done < m.n:
            gap = (lam[done] - lam[done - 1]) / m.lam_max
            print(f"{eb.chain_id(chain)} band {k}: relative boundary gap {gap:.2e}, p {r['p']}, {r['iterations']} iterations, largest degree {r['max_degree']}")
            if (name, k) == eb.SPLIT:
                assert gap < 1e-12 and eb.truth_extent(lam, done, m.lam_max) == done + 1
            else:
                assert gap >= eb.MIN_GAP and eb.truth_extent(lam, done, m.lam_max) == done
        assert r["converged"] == nev and r["iterations"] <= eb.MAX_REF_ITERS
    assert (np.diff(lam_r) >= 0).all()
    assert np.abs(lam_r - lam[:total]).max() <= 1e-10 * m.lam_max
    e = eb.orthonormality(U_r)
    print(f"{eb.chain_id(chain)}: eigenvalue error {np.abs(lam_r - lam[:total]).max():.2e}, ||U^T U - I||_max {e:.2e}")
    assert e <= 64 * (total + max(r["p"] for r in runs)) * eb.U53
    if name == "path5":
        assert runs[1]["iterations"] == 0 and runs[1]["max_degree"] == 0                 # p = n - m: the first Rayleigh-Ritz step is exact


def test_the_locked_eigenvalue_lowers_the_degree_on_band_5_of_the_grid_graph(mats):
    chain = eb.CHAINS[0]
    m = mats["graph4221"]
    lam_r, U_r, runs = eb.reference_chain(chain)
    first = {cap: eb.reference_band(m, 64, U_r[:, :256], lam_r, 13, 60, max_iter=1, lock_cap=cap)["max_degree"] for cap in (True, False)}
    print(f"band 5 at degree 60, first filter: degree {first[True]} with the locked eigenvalue in the cap, {first[False]} without; over the run {runs[4]['max_degree']}")
    assert first[True] < first[False] <= 60 and runs[4]["max_degree"] < runs[0]["max_degree"] <= 60


def test_every_omission_breaks_the_cross_orthogonality_bound_by_1e3(mats):
    """The block a filter at the cap's limit hands to the projection: X = X0 + 2^23 Q A with X0 orthonormal and orthogonal to Q,
    A of unit entries -- the locked directions amplified 2^23 times over the block's own, the most the degree cap admits.  After
    the whole projection (two passes) and Cholesky QR twice, ||[Q X]^T [Q X] - I||_max is held to the bound of
    tests/test_gpu_eigs_band.py, 8 max(e_ref, (m + p) 2^-53); each omission must exceed that by 1e3."""
    lam_r, U_r, _ = eb.reference_chain(eb.CHAINS[0])
    n, m, p = 4221, 320, 77
    Q = U_r[:, :m]
    rng = np.random.default_rng(27)
    X0 = np.linalg.qr(eb.project_twice(rng.standard_normal((n, p)), Q))[0]
    X = X0 + 2.0 ** 23 * (Q @ rng.choice([-1.0, 1.0], size=(m, p)))
    assert len(eb.panels_of(m)) == 2 and len(eb.cross_chunks_of(n, 80)) == 5

    def cross(Xp):
        return eb.orthonormality(np.concatenate([Q, ec._cholqr2(Xp, n, p)], axis=1))

    e_ref = cross(eb.project_twice(X, Q))
    bound = 8 * max(e_ref, (m + p) * eb.U53)
    broken = {"one panel of Q": cross(eb.project_twice(X, Q, skip_panel=1)), "one chunk of rows": cross(eb.project_twice(X, Q, skip_chunk=4)),
              "Q's last column": cross(eb.project_twice(X, Q, skip_last_column=True)), "the second pass": cross(eb.project_twice(X, Q, passes=1))}
    print(f"whole projection {e_ref:.2e}, bound {bound:.2e}; " + ", ".join(f"without {k}: {v:.2e} ({v / bound:.1e} x)" for k, v in broken.items()))
    assert e_ref <= (m + p) * eb.U53 * 8
    for k, v in broken.items():
        assert v >= 1e3 * bound, k


def test_the_kernel_shapes_reach_both_operand_paths_and_plain_float64_passes_the_bounds():
    import eigs_kernel_cases as ek
    S = eb.kernel_shapes()
    assert len(set(S)) == len(S)
    assert {s[1] for s in S} == set(eb.K_MQS) and {s[2] for s in S} == set(eb.K_LDS) and {s[5] for s in S} == set(eb.K_M0S)
    assert set(eb.K_NS) <= {s[0] for s in S} and {len(eb.cross_chunks_of(s[0], s[2])) for s in S} == {1, 2, 3}
    assert {tuple(ek.tile_groups(ld)) for ld in eb.K_LDS} == {(1,), (3,), (4, 3), (4, 4, 4, 4)}
    assert 2 * sum(s[3] < s[2] for s in S) >= len(S) - 1                                  # p < ld in half of them
    vec, scal = [s for s in S if eb.vector_path(s)], [s for s in S if not eb.vector_path(s)]
    assert len(vec) >= 8 and len(scal) >= 8
    assert any(s[1] % 4 for s in vec) and any(s[6] == 1 and s[5] % 4 for s in S)         # a ragged last quad on the vector path; 8-byte alignment only
    for s in S:
        n, mq, ld, p, ldq, m0, base = s
        kinds = {mq: "mq", mq + 1: "mq + 1", mq + 3: "mq + 3"}
        assert ldq in kinds or (ldq % 4 == 0 and ldq >= m0 + mq)
    for s in S[::5]:
        d = eb.band_design(s, "float")
        flat, base = d.flat_q()
        n, mq, ld, p, ldq, m0, _ = s
        idx = base + m0 + np.arange(n)[:, None] * ldq + np.arange(mq)[None, :]
        assert np.isfinite(flat[idx]).all() and np.isnan(flat).sum() == flat.size - n * mq           # NaN wherever the panel is not
        C64 = np.zeros((d.mq16, ld)); C64[:mq] = d.Q.T @ d.X
        assert ek.ratio(C64, *d.cross()) <= 1 and ek.ratio(d.X - d.Q @ d.C[:mq], *d.deflate()) <= 1
        # an omission breaks the bound by 1e3: the last row of the chunk, the last column of the panel
        if n > 1:
            C64[:mq] = d.Q[:-1].T @ d.X[:-1]
            assert ek.ratio(C64, *d.cross()) >= 1e3
        short = d.X - d.Q[:, :mq - 1] @ d.C[:mq - 1]
        assert ek.ratio(short, *d.deflate()) >= 1e3
    for m in eb.WALK_MS:
        assert len(eb.panels_of(m)) == 2
