"""Batched truncated SVDs for the streamer (bfhipTruncSvdBatchDevice, butterfly_amd/streamer_build.FrontierStreamer; DESIGN.md
section 30), the part that needs no GPU: the breadth-first streamer against the depth-first one with a deterministic numpy
factorizer (same descriptor, same leaf bits, same counters, the batch sizes the frontiers must have), the host driver alone under
AddressSanitizer and UBSan against stand-ins of every launch (tests/native/tsvd_batch_host_check.c, a program of its own), the
refusals through ctypes before a device is touched, and the struct layouts against a compiled C probe."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from butterfly_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "butterfly_amd", "csrc")


class NumpyFactorizer:
    """gesdd and the reference's count rule on streamer_build's densify: deterministic, so the depth-first and the breadth-first
    walk must give the same bits.  record: (m, n, k) per SVD; batches: the size of every svd_many call."""

    def __init__(self, tol=1e-3):
        self.tol, self.record, self.batches = tol, [], []

    def svd(self, block, row_node, col_node, tree):
        from butterfly_amd import streamer_build as sb, streamer_structure as ss
        from oracle import streamer_values as sv
        a = sb.densify(block)
        with sv._blas_threads(2):
            u, s, vt = np.linalg.svd(a, full_matrices=False)
        k = 0
        while k < len(s) and s[k] >= self.tol * s[0]:
            k += 1
        self.record.append((a.shape[0], a.shape[1], k))
        return k, len(s), ss.Dense(a.shape[0], k, np.ascontiguousarray(u[:, :k])), ss.Dense(k, a.shape[1], np.ascontiguousarray(s[:k, None] * vt[:k]))


class NumpyBatchFactorizer(NumpyFactorizer):
    def svd_many(self, requests):
        self.batches.append(len(requests))
        return [self.svd(*r) for r in requests]


def stream(pts, phi, freqs, wmax, depth, streamer_class, fz):
    """stream_butterfly's loop on a streamer class of choice: (streamer, descriptor, leaf values)."""
    from butterfly_amd import streamer_structure as ss
    tree = ss.Octree(np.ascontiguousarray(pts, dtype=np.float64), 1)
    st = streamer_class(tree, depth, fz, 20, 20, 0)
    a_phi = np.ascontiguousarray(phi[tree.perm])
    j0, J = 0, phi.shape[1]
    while not st.is_done():
        a, b, left, right = st.cols.leaf_interval(st.current_col_node(), 0.0, wmax)
        lo, hi = (-np.inf if left else a), (np.inf if right else b)
        j1 = j0
        while j1 < J and lo <= freqs[j1] < hi:
            j1 += 1
        st.feed(ss.Dense(len(pts), j1 - j0, a_phi[:, j0:j1]))
        j0 = j1
    desc, vals = ss.to_desc(st.get_mat())
    return st, desc, vals


def same_operator(d, dv, e, ev):
    assert d.root == e.root and d.kind == e.kind and d.rows == e.rows and d.cols == e.cols and d.block_kind == e.block_kind
    assert [[tuple(c) for c in ch] for ch in d.children] == [[tuple(c) for c in ch] for ch in e.children]
    assert sorted(dv) == sorted(ev) and len(ev) > 50
    for node in ev:
        assert dv[node].shape == ev[node].shape and dv[node].tobytes() == ev[node].tobytes(), node


CASES = [(600, 11, 2, dict(svds=52, merges=3, feeds=4)), (1500, 15, 3, dict(svds=423, merges=7, feeds=8))]


@pytest.fixture(scope="module", params=CASES, ids=["n600_l11_d2", "n1500_l15_d3"])
def walks(request):
    from butterfly_amd import streamer_build as sb, streamer_structure as ss
    from oracle import streamer_values as sv
    n, lmax, depth, stats = request.param
    pts, phi, freqs = sv.sphere_lbo_problem(n, lmax)
    wmax = float(np.sqrt(lmax * (lmax + 1.0)) * 1.0001)
    out = dict(n=n, stats=stats, pts=pts, phi=phi, freqs=freqs, wmax=wmax, depth=depth)
    for name, cls, fz in (("depth", ss.Streamer, NumpyFactorizer()), ("frontier", sb.FrontierStreamer, NumpyBatchFactorizer()),
                          ("frontier_svd_only", sb.FrontierStreamer, NumpyFactorizer())):
        st, desc, vals = stream(pts, phi, freqs, wmax, depth, cls, fz)
        out[name] = dict(st=st, desc=desc, vals=vals, fz=fz)
    return out


def test_frontier_streamer_is_the_depth_first_one_bit_for_bit(walks):
    ref = walks["depth"]
    assert ref["st"].stats == walks["stats"]
    for name in ("frontier", "frontier_svd_only"):
        got = walks[name]
        same_operator(got["desc"], got["vals"], ref["desc"], ref["vals"])
        assert got["st"].stats == ref["st"].stats
        assert sorted(got["fz"].record) == sorted(ref["fz"].record) and len(ref["fz"].record) == walks["stats"]["svds"]
    assert walks["frontier_svd_only"]["fz"].batches == []


def test_frontiers_have_the_batch_sizes_of_the_row_tree(walks):
    b = walks["frontier"]["fz"].batches
    print("batches:", b)
    assert sum(b) == walks["stats"]["svds"]
    if walks["n"] == 600:
        assert b == [1, 8, 1, 8, 1, 8, 1, 8, 8, 8]
    else:
        assert len(b) == 24 and max(b) == 48


def test_stream_butterfly_batched_gives_the_unbatched_descriptor():
    from butterfly_amd import streamer_build as sb
    from oracle import streamer_values as sv
    pts, phi, freqs = sv.sphere_lbo_problem(600, 11)
    wmax = float(np.sqrt(11 * 12.0) * 1.0001)
    fa, fb = NumpyFactorizer(), NumpyBatchFactorizer()
    _, perm_a, a = sb.stream_butterfly(pts, phi, freqs, wmax, freq_depth=2, factorizer=fa, device=-1, flags=_capi.FLAG_PLAN_ONLY)
    _, perm_b, b = sb.stream_butterfly(pts, phi, freqs, wmax, freq_depth=2, factorizer=fb, device=-1, flags=_capi.FLAG_PLAN_ONLY, batched=True)
    same_operator(b["desc"], b["leaf_values"], a["desc"], a["leaf_values"])
    assert np.array_equal(perm_a, perm_b) and {k: a[k] for k in ("svds", "merges", "feeds", "columns")} == {k: b[k] for k in ("svds", "merges", "feeds", "columns")}
    assert "svd_batches" in b and "svd_batches" not in a and fb.batches == [1, 8, 1, 8, 1, 8, 1, 8, 8, 8]
    assert sorted(b["svd_records"]) == sorted(a["svd_records"])


def test_the_batched_host_driver_alone_under_sanitizers(tmp_path):
    exe = tmp_path / "tsvd_batch_host_check"
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", os.path.join(ROOT, "tests", "native"),
                           os.path.join(ROOT, "tests", "native", "tsvd_batch_host_check.c"), os.path.join(CSRC, "bfhip_tsvd_batch.c"),
                           os.path.join(CSRC, "bfhip_tsvd.c"), "-o", str(exe), "-lm"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout + out.stderr)[-3000:]
    assert "runtime error" not in out.stderr and "ERROR: AddressSanitizer" not in out.stderr


def test_refusals_before_a_device_is_touched():
    lib = _capi.load()
    a, s = np.zeros(16), np.zeros(4)
    opt = _capi.BfhipTruncSvdOptions()
    opt.structSize, opt.tol = C.sizeof(opt), 1e-3
    probs = (_capi.BfhipTruncSvdProblem * 2)()
    infos = (_capi.BfhipTruncSvdInfo * 2)()
    for i in range(2):
        probs[i].dA, probs[i].m, probs[i].n, probs[i].lda, probs[i].dSigma = a.ctypes.data, 4, 4, 4, s.ctypes.data
        infos[i].structSize = C.sizeof(_capi.BfhipTruncSvdInfo)
    bi = _capi.BfhipTruncSvdBatchInfo()
    bi.structSize = C.sizeof(bi)

    def call(count=2, o=opt, p=probs, b=bi):
        rc = lib.bfhipTruncSvdBatchDevice(0, p, count, C.byref(o) if o is not None else None, 0, infos, None, C.byref(b), None)
        return rc, lib.bfhipLastErrorMessage().decode()

    assert call(o=None)[0] == 1 and call(p=None)[0] == 1
    bad = _capi.BfhipTruncSvdOptions()
    bad.structSize, bad.tol = 8, 1e-3
    assert call(o=bad)[0] == 1
    bi.structSize = 4
    assert call() == (1, "structSize is not sizeof(BfhipTruncSvdBatchInfo)")
    bi.structSize = C.sizeof(bi)
    assert call(count=(1 << 20) + 1)[0] == 1
    probs[1].lda = 3
    assert call() == (1, "problem 1: lda is less than n")
    probs[1].lda = 4
    probs[0].m = 0
    assert call() == (1, "problem 0: min(m, n) is 0")
    probs[0].m = 4
    probs[1].dSigma = None
    assert call() == (1, "problem 1: NULL argument")
    probs[1].dSigma = s.ctypes.data
    infos[1].structSize = 3
    assert call()[1].startswith("problem 1: structSize")
    infos[1].structSize = C.sizeof(_capi.BfhipTruncSvdInfo)
    opt.tol = 1.0
    assert call() == (1, "problem 0: tol is not in (0, 1)")
    opt.tol = 1e-3
    # nothing to do is no error and touches no device
    assert call(count=0)[0] == 0 and bi.groups == 0 and bi.launches == 0 and bi.synchronisations == 0
    from butterfly_amd import streamer_build as sb
    assert sb.truncated_svd_batch_device([], 1e-3) == []
    with pytest.raises(ValueError):
        sb.truncated_svd_batch_device([np.zeros(4)], 1e-3)


def test_structs_and_device_tables_match_the_c_side(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bfhip.h"\n#include "bfhip_tsvd_batch.h"\nint main(void){\n'
                   'printf("%zu %zu %zu %zu\\n", sizeof(BfhipTruncSvdProblem), sizeof(BfhipTruncSvdBatchInfo), offsetof(BfhipTruncSvdProblem, dW), '
                   'offsetof(BfhipTruncSvdBatchInfo, seconds));\n'
                   'printf("%zu %zu %zu\\n", sizeof(BfTsvdBatchItem) % 8, sizeof(BfTsvdBatchWords), sizeof(BfTsvdBatchFin) % 8);\n'
                   'uint32_t const nts[] = {2, 4, 10, 66}; uint32_t first[5], owner[41];\n'
                   'printf("%llu", (unsigned long long)bfTsvdBatchPairTable(nts, 4, first, owner));\n'
                   'for (int i = 0; i < 5; ++i) printf(" %u", first[i]);\nprintf("\\n");\n'
                   'printf("%llu %llu\\n", (unsigned long long)bfTsvdBatchProblemBytes(33, 20, 0), (unsigned long long)bfTsvdBatchProblemBytes(33, 20, 1));\n'
                   'return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src), os.path.join(CSRC, "bfhip_tsvd_batch.c"),
                           os.path.join(CSRC, "bfhip_tsvd.c"), "-Wl,--unresolved-symbols=ignore-all", "-o", str(exe), "-lm"])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    assert [int(v) for v in lines[0].split()] == [C.sizeof(_capi.BfhipTruncSvdProblem), C.sizeof(_capi.BfhipTruncSvdBatchInfo),
                                                  _capi.BfhipTruncSvdProblem.dW.offset, _capi.BfhipTruncSvdBatchInfo.seconds.offset]
    assert [int(v) for v in lines[1].split()] == [0, 32, 0]
    assert [int(v) for v in lines[2].split()] == [41, 0, 1, 3, 8, 41]
    small, full = (int(v) for v in lines[3].split())
    # 33 x 20: one pair of tiles, one chunk: B 33 x 32, one partial Gram matrix, one Q, 32 sums; the recovery adds 33 x 32 + 32 x 32 doubles
    assert small >= (33 * 32 + 1024 + 1024 + 32) * 8 and full - small == (33 * 32 + 32 * 32) * 8
