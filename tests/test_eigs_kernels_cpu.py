"""The eigensolver's kernels launched one at a time, the part that needs no GPU: BfEigsStep's layout
against a compiled C program, bfdevEigsChunkRows (a host function of the loaded library) against its restatement and the
invariants the driver's allocation relies on, the branches each shape of tests/eigs_kernel_cases.py is there for, and, on
the references alone, that every omission a kernel could make -- the last row, a whole chunk, a 16-column tile, a row's last
nonzero -- breaks a bound by at least 1e3 while the same operation in plain float64 passes it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eigs_kernel_cases as ek
from butterfly_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "butterfly_amd", "csrc")
BREAKS = 1e3
FLOAT_SHAPES = ek.dense_shapes()


def test_the_step_struct_has_the_c_layout(tmp_path):
    fields = [name for name, _ in ek.BfEigsStep._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bfhip_internal.h"\nint main(void){printf("%zu", sizeof(BfEigsStep));\n'
                   + "".join(f'printf(" %zu", offsetof(BfEigsStep, {f}));\n' for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(ek.BfEigsStep)] + [getattr(ek.BfEigsStep, f).offset for f in fields]
    lib = _capi.load()
    for name in ("bfdevEigsStep", "bfdevEigsGram", "bfdevEigsRotate", "bfdevEigsResidual", "bfdevEigsStore", "bfdevEigsChunkRows"):
        assert hasattr(lib, name)


def test_chunk_rows_against_the_restatement_and_the_allocation_invariants():
    lib = ek.bind(_capi.load())
    for (n, ld), want in ek.CHUNK_TABLE:
        assert lib.bfdevEigsChunkRows(n, ld) == want == ek.chunk_rows(n, ld), (n, ld)
    rng = np.random.default_rng(25)
    ns = [1, 1023, 1024, 1025, 65535, 65536, 65537, 131072, 131073, 1 << 20, (1 << 20) + 1, (1 << 32) + 5] + \
         [int(v) for v in 2 ** (rng.random(200) * 34)]
    for ld in range(16, 257, 16):
        cap = ek.max_chunks(ld)
        assert 64 <= cap <= 1024 and (cap == (1 << 23) // (ld * ld) or cap in (64, 1024))
        for n in ns + [1024 * cap - 1, 1024 * cap, 1024 * cap + 1, 1040 * cap, 1040 * cap + 1]:
            rows = lib.bfdevEigsChunkRows(n, ld)
            assert rows == ek.chunk_rows(n, ld)
            assert rows % 16 == 0 and rows >= 1024 and -(-n // rows) <= cap, (n, ld, rows)
    # the chunk-growth shape: 1040 rows, 127 chunks, the last of 49 rows (49 mod 4 = 1)
    ch = ek.chunks_of(*ek.BIG)
    assert ek.chunk_rows(*ek.BIG) == 1040 and len(ch) == 127 and ch[-1][1] - ch[-1][0] == 49 and 49 % 4 == 1
    assert ek.BIG[0] > 1024 * ek.max_chunks(ek.BIG[1]) == 131072


def test_the_dense_shapes_reach_the_branches_they_are_there_for():
    shapes = ek.dense_shapes()
    assert {ld: ek.tile_groups(ld) for ld in ek.DENSE_LDS} == ek.WANTED_GROUPS
    assert max(ek.DENSE_LDS) == 256                                              # the solver's maximum: four full groups
    nts_first = {g[0] for g in ek.WANTED_GROUPS.values()}
    nts_later = {nt for g in ek.WANTED_GROUPS.values() for nt in g[1:]}
    assert nts_first == {1, 3, 4} and nts_later == {1, 2, 3, 4}                  # <2> and <3> at tj0 > 0, <3> at tj0 = 0
    have = {(n, ld) for n, ld, _ in shapes}
    assert have == {(n, ld) for ld in ek.DENSE_LDS for n in ek.DENSE_NS if n in (17, 1025, 2049) or ld in (48, 112)} and len(shapes) == 36
    assert {15, 16, 17, 1023, 1024, 1025} <= set(ek.DENSE_NS)                    # the 16-row prefetch window and the chunk edge
    assert all(len(ek.chunks_of(n, ld)) == -(-n // 1024) for n, ld, _ in shapes) and len(ek.chunks_of(2049, 256)) == 3
    padded = [(n, ld, p) for n, ld, p in shapes if p < ld]
    assert 2 * len(padded) == len(shapes)
    assert {ld - p for _, ld, p in padded} == {15, 1} and all(1 <= p <= ld for _, ld, p in shapes)
    for ld in (48, 112):                                                         # both paddings at both of the new tile variants
        assert {ld - p for _, l, p in padded if l == ld} == {15, 1}
    assert sorted(ld for _, ld, _ in ek.gram_xx_shapes()) == list(ek.DENSE_LDS)
    for n, ld, p in shapes:
        d = ek.Dense(n, ld, p, "int", operands_only=True)
        assert not d.X[:, p:].any() and not d.Y[:, p:].any() and np.abs(d.X).max() <= 3
        assert d.X.any() and d.Y.any() and not np.array_equal(d.X, d.Y)


def test_the_step_and_store_designs_reach_the_branches_they_are_there_for():
    lanes = {p: ek.step_lanes(p) for p in ek.STEP_PS}
    assert {1, 2, 3, 4, 5, 8, 9, 16, 33, 64, 65, 130, 256} <= set(ek.STEP_PS)
    assert {l for l, _ in lanes.values()} == {1, 2, 4, 8, 16, 32, 64}            # below 8 (BF_CHEB_GATHERS): per-lane pairs; from 8 on: shared
    assert lanes[3] == (4, 1) and lanes[5] == (8, 1) and lanes[9] == (16, 1) and lanes[17] == (32, 1) and lanes[33] == (64, 1)      # dead lanes in one panel
    assert lanes[64] == (64, 1) and lanes[65] == (64, 2) and lanes[130] == (64, 3) and lanes[256] == (64, 4)
    assert 65 % 64 and 130 % 64                                                  # dead lanes in the last panel
    assert set(ek.STEP_COLUMNWISE_PS) == {3, 9, 65, 130}
    rowptr, colind = ek.ladder259()
    n, deg = len(rowptr) - 1, np.diff(rowptr.astype(np.int64))
    assert n == 259 and all(n % (256 >> lg) for lg in range(7)) and (deg == np.arange(n) % 20).all()
    assert set(deg) == set(range(20)) and {7, 8, 9, 15, 16, 17} <= set(deg)      # row lengths around the multiples of 8
    for i in range(n):
        cols = colind[int(rowptr[i]):int(rowptr[i + 1])].astype(np.int64)
        assert (np.diff(cols) > 0).all() and (cols < n).all()
        if deg[i] == 2:
            assert list(cols) == [0, n - 1]
    ones = [int(colind[int(rowptr[i])]) for i in range(n) if deg[i] == 1]
    assert set(ones) == {0, n - 1}
    w = ek.step_design("wide_and_empty", "float")
    assert w.deg.min() == 0 and w.deg.max() == 70 and ek.step_design("mesh63", "float").n == 63
    for name in ek.STEP_MATRICES:
        for kind in ("int", "float"):
            s = ek.step_design(name, kind)
            assert s.colind.max() < s.n and s.val.all() and s.alpha > 0 and s.beta and s.gamma
    n, ld, nev, ldu = ek.STORE_SHAPES[-1]
    assert n * nev == 16800240 > ek.STORE_ONE_PASS == 16777216 and n * nev < 2 * ek.STORE_ONE_PASS
    assert all(nev <= ld and nev <= ldu for _, ld, nev, ldu in ek.STORE_SHAPES) and any(ldu > nev for *_, nev, ldu in ek.STORE_SHAPES)


def test_integer_designs_stay_below_2_to_the_53():
    worst = ek.int_worst_case(ek.BIG[0], 256)
    assert worst["gram"] == 9 * 131089 and max(worst.values()) < 2 ** 53 // 2 ** 20
    for name in ek.STEP_MATRICES:
        s = ek.step_design(name, "int")
        assert ek.int_worst_case(0, 0, int(s.deg.max()), ek.STEP_SCALARS["int"])["step"] < 2 ** 20
        assert np.abs(s.val).max() <= 3 and np.abs(s.b1).max() <= 3 and np.abs(s.b2).max() <= 3
        assert (s.val == np.rint(s.val)).all() and (s.b1 == np.rint(s.b1)).all()
    d = ek.dense(17, 48, 47, "int")
    for a in (d.X, d.Y, d.W, d.theta):
        assert (a == np.rint(a)).all() and np.abs(a).max() <= 3
    ref, bound = d.gram()
    assert not bound.any() and (ref == np.rint(ref)).all()


@pytest.mark.parametrize("shape", FLOAT_SHAPES, ids=ek.shape_id)
def test_dense_float_designs_every_omission_breaks_a_bound_and_float64_passes(shape):
    """The deltas of the omissions are formed in float64: they are magnitudes, compared with a bound 1e3 times smaller."""
    n, ld, p = shape
    d = ek.dense(n, ld, p, "float")
    X, Y, W, th = d.X, d.Y, d.W, d.theta
    worst = {}

    def over(delta, bound):
        """|delta| / bound entry by entry, 0 where the bound is 0 (the padding, where delta is 0 too)."""
        q = np.zeros(bound.shape)
        nz = bound > 0
        q[nz] = (np.abs(np.asarray(delta, dtype=np.float64))[nz] / bound[nz]).astype(np.float64)
        return q

    def broken(what, delta, bound):
        worst[what] = min(worst.get(what, np.inf), float(over(delta, bound).max()))

    def per_tile(q, axes):
        """The largest entry of q per 16 x 16 tile (axes (1, 3)) or per 16-column tile column (axes (0, 1, 3)), live tiles only."""
        t = q.reshape(-1, 16, ld // 16, 16) if axes == (1, 3) else q.reshape(1, -1, ld // 16, 16)
        t = t.max(axis=axes)
        live = len(d.live_tiles)
        return t[:live, :live] if t.ndim == 2 else t[:live]

    # Gram
    ref, bound = d.gram()
    assert ek.ratio(d.gram64(), ref, bound) <= 1
    assert not ref[p:].any() and not ref[:, p:].any() and not bound[p:].any() and not bound[:, p:].any()
    broken("gram last row", np.outer(X[-1], Y[-1]), bound)
    for r0, r1 in ek.chunks_of(n, ld):
        broken("gram chunk", X[r0:r1].T @ Y[r0:r1], bound)
    worst["gram tile"] = float(per_tile(over(ref, bound), (1, 3)).min())          # a tile left unwritten: the worst over the live tiles
    if shape in ek.gram_xx_shapes():
        ref, bound = d.gram(True)
        assert ek.ratio(d.gram64(True), ref, bound) <= 1
        broken("gram(X, X) last row", np.outer(X[-1], X[-1]), bound)
    # rotation: the last row left unwritten, one block of 16 contraction indices left out, one tile column left unwritten
    ref, bound = d.rotate()
    assert ek.ratio(d.rotate64(), ref, bound) <= 1 and not ref[:, p:].any() and not bound[:, p:].any()
    broken("rotate last row", ref[-1], bound[-1])
    for t in d.live_tiles:
        broken("rotate k-block", X[:, 16 * t:16 * t + 16] @ W[16 * t:16 * t + 16], bound)
    worst["rotate tile column"] = float(per_tile(over(ref, bound), (0, 1, 3)).min())
    # residual
    ref, bound = d.residual()
    assert ek.ratio(d.residual64(), ref, bound) <= 1 and not ref[p:].any()
    D = Y - th * X
    broken("residual last row", D[-1] ** 2, bound)
    for r0, r1 in ek.chunks_of(n, ld):
        broken("residual chunk", (D[r0:r1] ** 2).sum(axis=0), bound)
    print(f"{ek.shape_id(shape)}: each omission breaks its bound by at least " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert min(worst.values()) >= BREAKS


@pytest.mark.parametrize("name", ek.STEP_MATRICES)
def test_step_float_designs_every_last_nonzero_matters_and_float64_passes(name):
    s = ek.step_design(name, "float")
    worst = np.inf
    for with_b2 in (False, True):
        ref, bound = s.reference(with_b2)
        assert (bound > 0).all()
        r64 = ek.ratio(s.eval(np.float64, with_b2), ref, bound)
        print(f"{name} b2={with_b2}: float64 on the host at {r64:.2e} of the bound")
        assert r64 <= 1
        for row in np.nonzero(s.deg)[0]:
            last = int(s.rowptr[row + 1]) - 1
            delta = np.abs(s.alpha * s.val[last] * s.b1[int(s.colind[last])])
            worst = min(worst, float((delta / bound[row]).max()))
        # a design is a fixed point of its mutation helper: the mutated values differ in that one entry
        row = int(np.nonzero(s.deg)[0][-1])
        assert np.count_nonzero(s.without_last_nonzero(row) != s.val) == 1
        mut = s.eval(np.float64, with_b2, s.without_last_nonzero(row))
        assert ek.ratio(mut, ref, bound) >= BREAKS
    print(f"{name}: a row's last nonzero left out breaks the bound by at least {worst:.1e}")
    assert worst >= BREAKS


def test_store_reference_is_one_multiplication_per_element():
    X, d = ek.store_design(*ek.STORE_SHAPES[1])
    assert X.all() and (d >= 0.5).all() and not np.array_equal(d[:, None] * X, X)
