"""bfhipTruncSvdDevice one call at a time, on the shapes at which each mechanism can go wrong, every
case judged against numpy's gesdd of the same matrix by tests/tsvd_cases.judge: k equal; sigma to 1e-12 sigma_0; U_k^T U_k - I
to 1e-12 / tol; || A - U_k W ||_F within the discarded tail + 1e-12 || A ||_F; the rows of W of norm sigma_j to 1e-12 sigma_0.

The graded case is tests/tsvd_cases.graded_matrix: the grid 10^(-j / 8) itself puts a singular value exactly on both
thresholds (1e-3 and 1e-6), which the reference-side design check refuses, so the grid is taken half a step aside."""
import ctypes as C

import numpy as np
import pytest

import tsvd_cases as tc

pytestmark = pytest.mark.gpu

CASES = tc.cases()


def raw_call(a, m, n, lda, tol, cap_u=None, cap_w=None, max_sweeps=0, values_only=False):
    """The C entry on a device tensor `a` (first element of the view) with explicit capacities: (rc, info, sigma, U, W)."""
    import torch
    from butterfly_amd import _capi
    lib = _capi.load()
    dev = a.device
    N = min(m, n)
    cap_u = N if cap_u is None else cap_u
    cap_w = N if cap_w is None else cap_w
    opt = _capi.BfhipTruncSvdOptions()
    opt.structSize, opt.tol, opt.maxSweeps = C.sizeof(opt), tol, max_sweeps
    info = _capi.BfhipTruncSvdInfo()
    info.structSize = C.sizeof(info)
    sigma = torch.full((N,), -1.0, dtype=torch.float64, device=dev)
    U = torch.full((m, max(cap_u, 1)), -7.0, dtype=torch.float64, device=dev)
    W = torch.full((max(cap_w, 1), n), -7.0, dtype=torch.float64, device=dev)
    rc = lib.bfhipTruncSvdDevice(0, C.c_void_p(a.data_ptr()), m, n, lda, C.byref(opt), C.c_void_p(sigma.data_ptr()),
                                 None if values_only else C.c_void_p(U.data_ptr()), max(cap_u, 1), cap_u,
                                 None if values_only else C.c_void_p(W.data_ptr()), n, cap_w, C.byref(info), None)
    torch.cuda.synchronize()
    return rc, info, sigma, U, W


@pytest.mark.parametrize("name,A,tol,check_values", CASES, ids=[c[0] for c in CASES])
def test_designed_case_against_gesdd(name, A, tol, check_values):
    from butterfly_amd.streamer_build import truncated_svd_device
    k, sigma, U, W, info = truncated_svd_device(A, tol)
    fig = tc.judge(A, tol, k, sigma, U, W, check_values)
    print(f"{name}: sweeps {info['sweeps']} transposed {info['transposed']} offNorm {info['offNorm']:.2e} {fig}")
    assert info["transposed"] == (1 if A.shape[0] < A.shape[1] else 0) and info["numSingular"] == min(A.shape)
    assert info["sweeps"] <= 30 and U.shape == (A.shape[0], k) and W.shape == (k, A.shape[1])


def test_strided_view_and_its_surroundings():
    """A (48, 40) view with lda = 56 inside a larger array: judged like the others; the array, the view included, bitwise
    untouched; U and W written in their first k columns / rows and nowhere else."""
    import torch
    big, view = tc.strided_case()
    d = torch.from_numpy(big).cuda()
    keep = d.clone()
    a = d[2:50, 8:48]
    assert a.stride(0) == 56
    rc, info, sigma, U, W = raw_call(a, 48, 40, 56, 1e-3, cap_u=40, cap_w=40)
    assert rc == 0
    assert torch.equal(d, keep)
    k = int(info.k)
    fig = tc.judge(view, 1e-3, k, sigma.cpu().numpy(), U.cpu().numpy(), W.cpu().numpy())
    print("strided:", fig)
    assert bool((U[:, k:] == -7.0).all()) and bool((W[k:] == -7.0).all())


def test_two_calls_give_the_same_bits():
    import torch
    from butterfly_amd.streamer_build import truncated_svd_device
    A = torch.from_numpy(tc.graded_matrix()).cuda()
    r1, r2 = truncated_svd_device(A, 1e-3), truncated_svd_device(A, 1e-3)
    assert r1[0] == r2[0] and all(torch.equal(x, y) for x, y in zip(r1[1:4], r2[1:4]))
    big, _ = tc.strided_case()
    d = torch.from_numpy(big).cuda()
    a = d[2:50, 8:48]
    c1, c2 = raw_call(a, 48, 40, 56, 1e-3), raw_call(a, 48, 40, 56, 1e-3)
    assert c1[0] == c2[0] == 0 and c1[1].k == c2[1].k and all(torch.equal(x, y) for x, y in zip(c1[2:], c2[2:]))


def test_capacity_values_only_and_non_convergence():
    import torch
    A = tc.graded_matrix()
    s_ref, k_ref = tc.reference(A, 1e-3)
    d = torch.from_numpy(A).cuda()
    # values only
    rc, info, sigma, U, W = raw_call(d, 300, 96, 96, 1e-3, values_only=True)
    assert rc == 0 and info.k == k_ref and info.numSingular == 96
    assert np.abs(sigma.cpu().numpy() - s_ref).max() <= 1e-12 * s_ref[0]
    # capU < k: the error, info.k set, U and W untouched
    rc, info, sigma, U, W = raw_call(d, 300, 96, 96, 1e-3, cap_u=k_ref - 1, cap_w=96)
    assert rc == 5 and info.k == k_ref and bool((U == -7.0).all()) and bool((W == -7.0).all())
    rc, info, sigma, U, W = raw_call(d, 300, 96, 96, 1e-3, cap_u=96, cap_w=k_ref - 1)
    assert rc == 5 and info.k == k_ref
    # one sweep cannot converge on the graded case: the error, with info filled in and no U, W
    rc, info, sigma, U, W = raw_call(d, 300, 96, 96, 1e-3, max_sweeps=1)
    from butterfly_amd import _capi
    assert rc == 2 and b"did not converge" in _capi.load().bfhipLastErrorMessage()
    assert info.sweeps == 1 and info.numSingular == 96 and info.offNorm > 1e-10 and bool((U == -7.0).all())
    # an all-zero matrix: k = 0
    z = torch.zeros((40, 24), dtype=torch.float64, device="cuda")
    rc, info, sigma, U, W = raw_call(z, 40, 24, 24, 1e-3)
    assert rc == 0 and info.k == 0 and bool((sigma == 0).all()) and bool((U == -7.0).all())
