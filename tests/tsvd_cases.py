"""The designed cases of the truncated-SVD tests (tests/test_streamer_build_cpu.py runs the emulator on them,
tests/test_gpu_tsvd.py the device), each judged against numpy's gesdd of the same matrix by `judge`."""
from __future__ import annotations

import numpy as np


def _orth(rng, m, n):
    q, _ = np.linalg.qr(rng.standard_normal((m, n)))
    return q


def with_spectrum(m, n, sigma, seed):
    rng = np.random.default_rng(seed)
    r = len(sigma)
    return (_orth(rng, m, r) * np.asarray(sigma)) @ _orth(rng, n, r).T


def cases():
    """[(name, A, tol, check_values)]: check_values False where the singular values are all equal (only reconstruction and
    orthogonality are defined there)."""
    rng = np.random.default_rng(29)
    out = []
    for m, n in ((33, 20), (20, 33), (64, 32), (100, 17), (257, 48), (1025, 130), (130, 1025)):
        out.append((f"random_{m}x{n}", rng.standard_normal((m, n)), 1e-3, True))
    graded = graded_matrix()
    out.append(("graded_tol1e-3", graded, 1e-3, True))
    out.append(("graded_tol1e-6", graded, 1e-6, True))
    out.append(("rank25_200x60", with_spectrum(200, 60, 1.0 + np.arange(25)[::-1] / 5.0, 2), 1e-3, True))
    out.append(("orthonormal_120x40", _orth(np.random.default_rng(3), 120, 40) * 0.75, 1e-3, False))
    # the streamer's own kind of block: most columns exactly zero, so the transposed block has rank 34 of 76 columns and a
    # ladder of noise columns (this is the shape on which a noise level relative to the pair's own largest column stalls)
    z = np.zeros((76, 209))
    z[:, np.sort(np.random.default_rng(6).choice(209, 34, replace=False))] = with_spectrum(76, 34, 10.0 ** (-np.arange(34) / 6.5), 6)
    out.append(("zero_columns_76x209", z, 1e-3, True))
    out.append(("clusters_150x40", with_spectrum(150, 40, np.r_[np.full(20, 1.0), np.full(20, 0.01)], 4), 1e-3, True))
    return out


def graded_matrix():
    """300 x 96, sigma_0 = 1 and sigma_j = 10^(-(j - 1/2) / 8) below it: eight values per decade over twelve decades.  The grid
    10^(-j / 8) itself has sigma_24 = 1e-3 sigma_0 and sigma_48 = 1e-6 sigma_0 exactly, i.e. a singular value ON both
    thresholds, which `reference` refuses; half a step aside the nearest value is 15 % from either."""
    j = np.arange(96)
    return with_spectrum(300, 96, np.where(j == 0, 1.0, 10.0 ** (-(j - 0.5) / 8.0)), 1)


def strided_case():
    """(the larger array, the (48, 40) view with lda = 56 inside it)."""
    big = np.random.default_rng(5).standard_normal((52, 56))
    return big, big[2:50, 8:48]


def reference(A, tol):
    """(sigma, k) of gesdd, with the case's own design checked: no singular value within 1e-6 relative of the threshold."""
    s = np.linalg.svd(A, compute_uv=False)
    thr = tol * s[0]
    assert np.all(np.abs(s - thr) > 1e-6 * thr), "badly designed case: a singular value sits on the threshold"
    k = 0
    while k < len(s) and s[k] >= thr:
        k += 1
    return s, k


def judge(A, tol, k, sigma, U, W, check_values=True):
    """The five checks of the issue; returns the measured figures, asserts every bound."""
    s_ref, k_ref = reference(A, tol)
    fig = dict(k=int(k), k_ref=k_ref)
    assert k == k_ref, fig
    U, W = np.asarray(U)[:, :k], np.asarray(W)[:k]
    fig["orth"] = float(np.abs(U.T @ U - np.eye(k)).max())
    assert fig["orth"] <= 1e-12 / tol, fig
    tail = float(np.sqrt(np.sum(s_ref[k:] ** 2)))
    fig["recon"] = float(np.linalg.norm(A - U @ W))
    fig["recon_bound"] = tail + 1e-12 * float(np.linalg.norm(A))
    assert fig["recon"] <= fig["recon_bound"], fig
    if check_values:
        fig["sigma"] = float(np.abs(np.asarray(sigma) - s_ref).max() / s_ref[0])
        assert fig["sigma"] <= 1e-12, fig
        fig["wrows"] = float(np.abs(np.linalg.norm(W, axis=1) - s_ref[:k]).max() / s_ref[0])
        assert fig["wrows"] <= 1e-12, fig
    return fig
