"""Eigenbands to the butterfly of Phi (butterfly_amd/streamer_build.py, bfhipTruncSvdDevice), the part
that needs no GPU: the pipeline's plumbing with a host factorizer against oracle/streamer_values.py, `densify` on every block
the streamer hands to the SVD, the numpy restatement of the device algorithm (tests/tsvd_emulator.py) on every designed case
against gesdd -- what shows, without a device, that the chosen block Jacobi converges --, the C entry's refusals, its structs
and schedule against a compiled C program, and its host side alone under AddressSanitizer and UBSan
(tests/native/tsvd_host_check.c, a program of its own)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tsvd_cases as tc
import tsvd_emulator as te
from butterfly_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "butterfly_amd", "csrc")
WMAX = float(np.sqrt(11 * 12.0) * 1.0001)


class NumpyFactorizer:
    """gesdd and the reference's count rule, as oracle/streamer_values.SvdFactorizer, on streamer_build's own densify;
    keeps every block it was handed."""

    def __init__(self, tol=1e-3):
        self.tol, self.record, self.blocks = tol, [], []

    def svd(self, block, row_node, col_node, tree):
        from butterfly_amd import streamer_build as sb, streamer_structure as ss
        from oracle import streamer_values as sv
        self.blocks.append(block)
        a = sb.densify(block)
        with sv._blas_threads(2):
            u, s, vt = np.linalg.svd(a, full_matrices=False)
        k = 0
        while k < len(s) and s[k] >= self.tol * s[0]:
            k += 1
        self.record.append((a.shape[0], a.shape[1], k))
        return k, len(s), ss.Dense(a.shape[0], k, np.ascontiguousarray(u[:, :k])), ss.Dense(k, a.shape[1], np.ascontiguousarray(s[:k, None] * vt[:k]))


@pytest.fixture(scope="module")
def runs():
    from butterfly_amd import streamer_build as sb, streamer_structure as ss
    from oracle import streamer_values as sv
    pts, phi, freqs = sv.sphere_lbo_problem(600, 11)
    rec = []
    st, a_phi = sv.stream_columns(pts, phi, freqs, WMAX, 2, record=rec)
    desc, vals = ss.to_desc(st.get_mat())
    fz = NumpyFactorizer()
    op, perm, info = sb.stream_butterfly(pts, phi, freqs, WMAX, freq_depth=2, factorizer=fz, device=-1, flags=_capi.FLAG_PLAN_ONLY)
    return dict(st=st, a_phi=a_phi, desc=desc, vals=vals, rec=rec, fz=fz, op=op, perm=perm, info=info, pts=pts)


def test_pipeline_with_a_host_factorizer_is_the_oracle_run(runs):
    """stream_butterfly with a numpy factorizer: the descriptor arrays of oracle stream_columns + to_desc, the leaf values bit
    for bit, the permutation, the counters and the SVD records."""
    from butterfly_amd import streamer_structure as ss
    r = runs
    d, e = r["info"]["desc"], r["desc"]
    assert d.root == e.root and d.kind == e.kind and d.rows == e.rows and d.cols == e.cols and d.block_kind == e.block_kind
    assert [[tuple(c) for c in ch] for ch in d.children] == [[tuple(c) for c in ch] for ch in e.children]
    got, want = r["info"]["leaf_values"], r["vals"]
    assert sorted(got) == sorted(want) and len(want) > 50
    for node in want:
        assert got[node].shape == want[node].shape and got[node].tobytes() == want[node].tobytes(), node
    assert np.array_equal(r["perm"], ss.Octree(r["pts"], 1).perm) and r["perm"].dtype == np.int64
    assert {k: r["info"][k] for k in ("svds", "merges", "feeds")} == r["st"].stats
    assert r["info"]["svds"] == 52 and r["info"]["columns"] == 144 and r["info"]["freq_depth"] == 2
    assert [(m, n, k) for m, n, _, _, k in r["rec"]] == r["fz"].record == r["info"]["svd_records"]
    assert r["info"]["leaf_bytes"] == sum(v.nbytes for v in want.values())
    assert r["op"].shape == (600, 144)
    # the case the GPU test runs: 52 SVDs, rows 74-600, columns 27-209, 24 of them wide
    ms, ns = [t[0] for t in r["fz"].record], [t[1] for t in r["fz"].record]
    assert (min(ms), max(ms), min(ns), max(ns), sum(m < n for m, n in zip(ms, ns))) == (74, 600, 27, 209, 24)


def test_default_frequency_depth_and_argument_checks(runs):
    from butterfly_amd import streamer_build as sb
    from oracle import streamer_values as sv
    pts, phi, freqs = sv.sphere_lbo_problem(600, 11)
    with pytest.raises(ValueError):
        sb.stream_butterfly(pts, phi[:, :10], freqs, WMAX, factorizer=NumpyFactorizer(), device=-1, flags=_capi.FLAG_PLAN_ONLY)
    with pytest.raises(ValueError):
        sb.stream_butterfly(pts, phi, freqs, WMAX, factorizer=NumpyFactorizer(), device=-1, dtype="c128")
    op, perm, info = sb.stream_butterfly(pts, phi, freqs, WMAX, factorizer=NumpyFactorizer(), device=-1, flags=_capi.FLAG_PLAN_ONLY, max_cols=40)
    from butterfly_amd import streamer_structure as ss
    assert info["freq_depth"] == ss.Octree(pts, 1).max_depth - 3 and 40 <= info["columns"] < 144


def test_densify_equals_the_oracles_on_every_block_of_the_run(runs):
    from butterfly_amd import streamer_build as sb, streamer_structure as ss
    from oracle import streamer_values as sv
    kinds = set()
    for b in runs["fz"].blocks:
        kinds.add(type(b).__name__)
        got, want = sb.densify(b), sv.densify(b)
        assert got.shape == want.shape == (b.m, b.n) and got.dtype == np.float64 and np.array_equal(got, want)
    assert len(runs["fz"].blocks) == 52 and {"Dense", "BlockDense"} <= kinds, kinds
    with pytest.raises(TypeError):
        sb.densify(ss.Product([ss.Identity(3), ss.Identity(3)]))
    with pytest.raises(ValueError):
        sb.densify(ss.Dense(2, 2))


EMU_CASES = tc.cases()
_SWEEPS = {}


@pytest.mark.parametrize("name,A,tol,check_values", EMU_CASES, ids=[c[0] for c in EMU_CASES])
def test_emulator_meets_the_device_bounds_on_every_designed_case(name, A, tol, check_values):
    """Same k as gesdd, the three residuals and the two value checks, within the default cap of 30 sweeps.  Largest sweep
    count over the cases: 8 (random 1025 x 130 and its transpose, the graded case); the rank-deficient case needs 5."""
    r = te.trunc_svd(A, tol)
    fig = tc.judge(A, tol, r["k"], r["sigma"], r["U"], r["W"], check_values)
    _SWEEPS[name] = r["sweeps"]
    print(f"{name}: sweeps {r['sweeps']} offNorm {r['offNorm']:.2e} {fig}")
    assert r["converged"] and r["sweeps"] <= te.DEFAULT_MAX_SWEEPS and r["offNorm"] <= te.thr_out(max(A.shape))
    assert r["transposed"] == (A.shape[0] < A.shape[1])


def test_emulator_on_the_strided_case_the_zero_matrix_and_one_sweep():
    _, view = tc.strided_case()
    r = te.trunc_svd(view, 1e-3)
    tc.judge(view, 1e-3, r["k"], r["sigma"], r["U"], r["W"])
    z = te.trunc_svd(np.zeros((40, 24)), 1e-3)
    assert z["k"] == 0 and z["sweeps"] == 1 and z["converged"]
    one = te.trunc_svd(tc.graded_matrix(), 1e-3, max_sweeps=1)
    assert not one["converged"] and one["offNorm"] > 1e-10


def test_the_graded_grid_itself_sits_on_both_thresholds():
    """Why tests/tsvd_cases.graded_matrix is half a step off the grid 10^(-j / 8): on the grid sigma_24 = 1e-3 sigma_0 and
    sigma_48 = 1e-6 sigma_0, and the design check on the reference side refuses the case, as it must."""
    A = tc.with_spectrum(300, 96, 10.0 ** (-np.arange(96) / 8.0), 1)
    for tol in (1e-3, 1e-6):
        with pytest.raises(AssertionError, match="badly designed"):
            tc.reference(A, tol)
        tc.reference(tc.graded_matrix(), tol)


def test_refusals_before_a_device_is_touched():
    lib = _capi.load()
    a = np.zeros(64)
    s = np.zeros(8)
    info = _capi.BfhipTruncSvdInfo()
    info.structSize = C.sizeof(info)

    def call(m=4, n=4, lda=4, tol=1e-3, size=None, flags=0, dA=a.ctypes.data, sigma=s.ctypes.data, dU=None, ldu=0, capU=0, dW=None, ldw=0, capW=0, opt=True):
        o = _capi.BfhipTruncSvdOptions()
        o.structSize, o.tol, o.flags = C.sizeof(o) if size is None else size, tol, flags
        rc = lib.bfhipTruncSvdDevice(0, dA, m, n, lda, C.byref(o) if opt else None, sigma, dU, ldu, capU, dW, ldw, capW, C.byref(info), None)
        return rc, lib.bfhipLastErrorMessage().decode()

    assert call(dA=None)[0] == 1 and call(sigma=None)[0] == 1 and call(opt=False)[0] == 1
    assert call(size=8) == (1, "structSize is not sizeof(BfhipTruncSvdOptions)")
    for tol in (0.0, -1e-3, 1.0, 1.5, float("nan")):
        assert call(tol=tol) == (1, "tol is not in (0, 1)")
    assert call(flags=1)[0] == 1
    assert call(m=0) == (1, "min(m, n) is 0") and call(n=0) == (1, "min(m, n) is 0")
    assert call(m=16385, n=16385, lda=16385) == (1, "min(m, n) is more than 16384")
    assert call(lda=3) == (1, "lda is less than n")
    assert call(dU=a.ctypes.data, ldu=2, capU=4) == (1, "ldu is less than capU")
    assert call(dW=a.ctypes.data, ldw=3, capW=4) == (1, "ldw is less than n")
    bad = _capi.BfhipTruncSvdInfo()
    bad.structSize = 4
    o = _capi.BfhipTruncSvdOptions()
    o.structSize, o.tol = C.sizeof(o), 1e-3
    assert lib.bfhipTruncSvdDevice(0, a.ctypes.data, 4, 4, 4, C.byref(o), s.ctypes.data, None, 0, 0, None, 0, 0, C.byref(bad), None) == 1


def test_structs_schedule_and_thresholds_match_the_c_side(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "bfhip.h"\n#include "bfhip_tsvd.h"\nint main(void){\n'
                   'printf("%zu %zu\\n", sizeof(BfhipTruncSvdOptions), sizeof(BfhipTruncSvdInfo));\n'
                   'unsigned const nts[] = {2, 4, 10, 32};\n'
                   'for (int i = 0; i < 4; ++i) for (unsigned s = 0; s + 1 < nts[i]; ++s) for (unsigned p = 0; p < nts[i] / 2; ++p) {\n'
                   '  uint32_t a, b; bfTsvdPair(nts[i], s, p, &a, &b); printf("%u %u %u %u %u\\n", nts[i], s, p, a, b); }\n'
                   'printf("%u %u %u %u\\n", bfTsvdLd(1), bfTsvdLd(32), bfTsvdLd(33), bfTsvdLd(130));\n'
                   'printf("%a %a %a %a\\n", bfTsvdThreshold(33), bfTsvdThreshold(65536), bfTsvdNoise(20), bfTsvdNoise(130));\n'
                   'return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src), "-o", str(exe), "-lm"])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    assert [int(v) for v in lines[0].split()] == [C.sizeof(_capi.BfhipTruncSvdOptions), C.sizeof(_capi.BfhipTruncSvdInfo)]
    pairs = [tuple(int(v) for v in ln.split()) for ln in lines[1:-2]]
    assert len(pairs) == 1 + 6 + 45 + 31 * 16
    for nt, s, p, a, b in pairs:
        assert te.round_robin_pair(nt, s, p) == (a, b)
    assert [int(v) for v in lines[-2].split()] == [te.padded_ld(1), te.padded_ld(32), te.padded_ld(33), te.padded_ld(130)] == [32, 32, 64, 160]
    assert [float.fromhex(v) for v in lines[-1].split()] == [te.thr_out(33), te.thr_out(65536), te.noise_level(20), te.noise_level(130)]
    hip = open(os.path.join(CSRC, "bfhip_tsvd.hip")).read()
    assert te.INNER_SWEEPS == 12 and "BF_TSVD_INNER_SWEEPS 12u" in open(os.path.join(CSRC, "bfhip_tsvd.h")).read() and "2 * BF_TSVD_EPS * sqrt(a * d)" in hip


def test_the_host_side_alone_under_sanitizers(tmp_path):
    exe = tmp_path / "tsvd_host_check"
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "tsvd_host_check.c"),
                           os.path.join(CSRC, "bfhip_tsvd.c"), "-o", str(exe), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout + out.stderr)[-3000:]
    assert "runtime error" not in out.stderr and "ERROR: AddressSanitizer" not in out.stderr
