"""Seeded least-squares cases for bfhipLstSqTruncated, each declaring the route(s) it reaches.

A case: name, A (mt x me), B (mt x n), the designed rank, `opts` (the route switches it is run with: qr_min, gram_min,
force_global; None = the defaults), `route` (the fields of bfhipLstSqRoute it must reach under `opts`, with the QR stage
leaving the designed rank), `alt` (other option sets it fits and is also run with on the GPU), `gap` (the spectrum keeps
>= 4x on each side of the truncation tol: rank, sigma and X are checked against the bounds; else only what the case says),
and `ref`: "ld" (long-double Jacobi, tests/lstsq_ref.py) or "designed" (the long-double factors; used where the Jacobi
reference would be slow -- tall QR cases -- and only with well-conditioned spectra, where the two agree within the bound).

Route coverage (checked by tests/test_lstsq_cpu.py against the router itself, bfhipLstSqRoutes):
* plain Jacobi kernel: every reachable (W, threads, LDS class, resident) -- 32 of them, found by brute force over every
  shape the kernel takes (me <= 2304, 2 (mt + me) 16 B <= 144 KiB) with the Gram form and the QR stage switched off.  The
  15 (W, threads, LDS) classes of 1024 threads with a 16/32/64 KiB tile are unreachable: 1024 threads means me > 64, and
  then the stacked matrix alone (me + 1)(mt + me + 1) 16 B >= 66 x 67 x 16 B > 64 KiB.  Resident 1024-thread launches exist
  only for W <= 16: resident means b >= me / 2 > 32 column pairs per step, and W = 32 / 64 gives 32 / 16 lane groups;
* the Gram form: natural (rows + columns >= 512) with me and mt off the 16 / 32 multiples, and forced (gram_min = 0);
* the global-memory kernel: natural only beyond 2304 columns or 4600 stacked rows (and > 4096 columns for it to beat the
  Gram form): here always FORCED (force_global = 1) on small shapes;
* QR: all six LDS classes, the register column path (<= 1024 rows) and the streaming one, exact rank deficiency,
  duplicate columns, rank 0 (GEMM with K = 0).
"""
from __future__ import annotations

import numpy as np

from lstsq_ref import designed, truncation_tol

HUGE = 1 << 40
PLAIN = dict(qr_min=HUGE, gram_min=HUGE, force_global=0)
GRAM = dict(qr_min=HUGE, gram_min=0, force_global=0)
GLOBAL = dict(qr_min=HUGE, gram_min=HUGE, force_global=1)
QR = dict(qr_min=0, gram_min=None, force_global=0)

# (mt, me) reaching each plain class (jacobi, w, threads, ldsClass, resident): the smallest mt me^2 (bfhipLstSqRoutes)
PLAIN_SHAPES = {
    (4, 256, 0, 1): (1, 1), (4, 256, 1, 1): (4, 30), (4, 256, 2, 1): (3, 43), (4, 256, 3, 1): (4, 62),
    (4, 1024, 3, 0): (4, 94), (4, 1024, 3, 1): (1, 65), (8, 256, 0, 1): (5, 1), (8, 256, 1, 1): (8, 28),
    (8, 256, 2, 1): (27, 33), (8, 256, 3, 0): (221, 35), (8, 256, 3, 1): (87, 33), (8, 1024, 3, 0): (8, 92),
    (8, 1024, 3, 1): (5, 65), (16, 256, 0, 1): (9, 1), (16, 256, 1, 1): (39, 17), (16, 256, 2, 1): (97, 17),
    (16, 256, 3, 0): (441, 19), (16, 256, 3, 1): (211, 17), (16, 1024, 3, 0): (69, 67), (16, 1024, 3, 1): (9, 65),
    (32, 256, 0, 1): (17, 1), (32, 256, 1, 1): (93, 9), (32, 256, 2, 1): (195, 9), (32, 256, 3, 0): (757, 11),
    (32, 256, 3, 1): (401, 9), (32, 1024, 3, 0): (75, 65), (64, 256, 0, 1): (33, 1), (64, 256, 1, 1): (511, 1),
    (64, 256, 2, 1): (1023, 1), (64, 256, 3, 0): (2301, 3), (64, 256, 3, 1): (2047, 1), (64, 1024, 3, 0): (207, 65),
}


def _case(name, A, B, rank, opts, route, alt=(), gap=True, ref="ld", X_design=None, note=""):
    return dict(name=name, A=A, B=B, rank=rank, opts=opts, route=route, alt=list(alt), gap=gap, ref=ref, X_design=X_design,
                note=note)


def _spectrum(kind, k):
    if kind == "well":
        return np.linspace(1.0, 0.5, k)
    if kind == "graded":
        return np.geomspace(1.0, 1e-8, k)
    if kind == "clustered":
        return 1.0 + 1e-12 * np.arange(k)
    raise ValueError(kind)


def _designed_case(name, mt, me, n, kind, seed, opts, route, rank=None, alt=(), rhs="range", ref="ld"):
    k = min(mt, me) if rank is None else rank
    A, B, X = designed(mt, me, n, _spectrum(kind, k), seed, rhs=rhs)
    return _case(name, A, B, k, opts, route, alt, ref=ref, X_design=X)


def plain_cases():
    out = []
    for i, ((w, threads, lds, res), (mt, me)) in enumerate(sorted(PLAIN_SHAPES.items())):
        n = 1 + (i % 3) * 16                      # 1, 17, 33 right-hand sides
        alt = [GRAM, GLOBAL] if mt * me <= 4096 else []
        out.append(_designed_case(f"plain-W{w}-t{threads}-lds{lds}-{'res' if res else 'blk'}-{mt}x{me}", mt, me, n,
                                  "well" if i % 2 else "graded", 100 + i, PLAIN,
                                  dict(qr=0, jacobi=0, w=w, threads=threads, ldsClass=lds, resident=res), alt=alt))
    return out


def suspect1_case():
    """Suspect 1: 99 columns of 2.2e-14 e2 each (below dim eps x the largest column on their own) carry sigma_2 =
    sqrt(99) 2.2e-14 ~ 5 tol together; zgesvd keeps it."""
    mt, me = 200, 100
    A = np.zeros((mt, me), dtype=np.complex128)
    A[0, 0] = 1.0
    A[1, 1:] = 2.2e-14
    B = np.zeros((mt, 2), dtype=np.complex128)
    B[1, 0] = 1.0
    B[0, 1] = 1.0
    B[1, 1] = 0.5
    return _case("suspect1-many-subthreshold-columns", A, B, 2, None, dict(qr=1, jacobi=0), alt=[PLAIN, GRAM, GLOBAL],
                 note="rank 2 in the reference; the per-column freeze / max-column QR stop gave rank 1")


def gram_cases():
    return [
        _designed_case("gram-natural-600x40", 600, 40, 5, "graded", 201, None, dict(qr=0, jacobi=1), alt=[PLAIN, GLOBAL]),
        _designed_case("gram-natural-480x48", 480, 48, 3, "well", 202, None, dict(qr=0, jacobi=1), alt=[PLAIN]),
        _designed_case("gram-natural-497x33", 497, 33, 2, "clustered", 203, None, dict(qr=0, jacobi=1)),
        _designed_case("gram-forced-50x37", 50, 37, 4, "graded", 204, GRAM, dict(qr=0, jacobi=1), alt=[PLAIN, GLOBAL]),
        _designed_case("gram-forced-wide-20x45", 20, 45, 3, "well", 205, GRAM, dict(qr=0, jacobi=1), alt=[PLAIN, GLOBAL]),
    ]


def global_cases():
    return [
        _designed_case("global-forced-40x21", 40, 21, 3, "graded", 301, GLOBAL, dict(qr=0, jacobi=2), alt=[PLAIN, GRAM]),
        _designed_case("global-forced-odd-31x7", 31, 7, 1, "clustered", 302, GLOBAL, dict(qr=0, jacobi=2), alt=[PLAIN]),
    ]


def qr_cases():
    out = []
    # the six LDS classes (need = 16 mt + 12 me + 64 bytes) and both column paths; tall: the factors are the reference
    for cls, (mt, me) in enumerate([(200, 65), (600, 80), (1500, 70), (3000, 66), (6000, 65), (9000, 65)]):
        big = mt * me > 40_000
        out.append(_designed_case(f"qr-lds{cls}-{mt}x{me}", mt, me, 3, "well" if big else "graded", 400 + cls, None,
                                  dict(qr=1, qrLdsClass=cls, qrStreaming=int(mt > 1024)), ref="designed" if big else "ld",
                                  rank=8 if big else None, alt=[] if big else [PLAIN]))
    out.append(_designed_case("qr-deficient-90x70-r20", 90, 70, 4, "graded", 410, None, dict(qr=1, qrLdsClass=0), rank=20,
                              alt=[PLAIN, GRAM, GLOBAL]))
    out.append(_designed_case("qr-forced-deficient-30x12-r5", 30, 12, 2, "well", 411, QR, dict(qr=1), rank=5,
                              alt=[PLAIN, GRAM, GLOBAL]))
    rng = np.random.default_rng(412)
    A = rng.standard_normal((40, 10)) + 1j * rng.standard_normal((40, 10))
    A[:, 5:] = A[:, :5]                                       # duplicate columns: rank 5
    B = A[:, :5] @ (rng.standard_normal((5, 3)) + 0j)
    out.append(_case("qr-duplicate-columns-40x10", A, B, 5, QR, dict(qr=1), alt=[PLAIN, GRAM, GLOBAL]))
    return out


def edge_cases():
    out = []
    # GEMM edges: M = me, N = n, K = mt (first GEMM) / me (second): 0, +-1 mod 32 / 16
    for i, (mt, me, n) in enumerate([(48, 32, 33), (49, 33, 31), (47, 31, 32), (17, 16, 1), (15, 15, 16), (64, 63, 65)]):
        out.append(_designed_case(f"gemm-{mt}x{me}x{n}", mt, me, n, "well", 500 + i, PLAIN, dict(qr=0, jacobi=0),
                                  alt=[GRAM, GLOBAL, QR]))
    out.append(_designed_case("me1-7x1", 7, 1, 3, "well", 510, PLAIN, dict(qr=0, jacobi=0), alt=[GRAM, GLOBAL, QR]))
    out.append(_designed_case("me2-9x2", 9, 2, 2, "graded", 511, PLAIN, dict(qr=0, jacobi=0), alt=[GRAM, GLOBAL, QR]))
    out.append(_designed_case("mt1-1x5", 1, 5, 2, "well", 512, PLAIN, dict(qr=0, jacobi=0), alt=[GRAM, GLOBAL, QR]))
    out.append(_designed_case("wide-12x30-odd", 12, 29, 4, "graded", 513, PLAIN, dict(qr=0, jacobi=0), alt=[GRAM, GLOBAL, QR]))
    out.append(_designed_case("clustered-60x40", 60, 40, 3, "clustered", 514, PLAIN, dict(qr=0, jacobi=0), alt=[GRAM, GLOBAL, QR]))
    out.append(_designed_case("random-rhs-50x20", 50, 20, 5, "graded", 515, PLAIN, dict(qr=0, jacobi=0), rhs="random",
                              alt=[GRAM, GLOBAL, QR]))
    # rank 0: zero, and entries whose squares underflow (sigma << eps: the reference keeps nothing)
    rng = np.random.default_rng(516)
    B = rng.standard_normal((30, 2)) + 1j * rng.standard_normal((30, 2))
    out.append(_case("zero-30x20", np.zeros((30, 20), dtype=np.complex128), B, 0, QR, dict(qr=1), alt=[PLAIN, GRAM, GLOBAL]))
    U = 1e-170 * (rng.standard_normal((30, 20)) + 1j * rng.standard_normal((30, 20)))
    out.append(_case("underflow-30x20", U, B, 0, QR, dict(qr=1), alt=[PLAIN, GRAM, GLOBAL]))
    # a kept sigma at 1.5 tol (no gap below it: rank and sigma only) -- the mutant with the threshold doubled drops it
    mt, me = 24, 10
    s = np.linspace(1.0, 0.5, 6)
    s = np.append(s, 1.5 * truncation_tol(1.0, max(mt, me)))
    A, B, X = designed(mt, me, 2, s, 517)
    out.append(_case("near-threshold-24x10", A, B, 7, PLAIN, dict(qr=0, jacobi=0), gap=False, X_design=X,
                     alt=[GRAM, GLOBAL, QR]))
    return out


def catalogue():
    return plain_cases() + [suspect1_case()] + gram_cases() + global_cases() + qr_cases() + edge_cases()


def opts_key(opts):
    return tuple(sorted((opts or {}).items()))
