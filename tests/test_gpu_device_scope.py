"""Every host entry point runs on its operator's device and hands the caller's device back, on every exit (bfDevEnter /
bfDevLeave, bfhip_internal.h).  The operand of tests/test_gpu_cov_condition.py (211 x 93, real, with its adjoint plan) is
compiled on device 1 while device 0 is current; after each call -- succeeding or failing after the switch -- device 0 is still
current.  The same sequence with device 1 current gives the same bits: where the caller stands changes no result."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, N, K, Q = 211, 93, 3, 2


def run_sequence(current, tmp_path, target=1):
    """All calls with `current` the current device and everything else on device `target`; returns the results as host arrays."""
    import torch
    import randgraph
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from oracle import bfref

    def here(what):
        assert torch.cuda.current_device() == current, f"after {what} the current device is {torch.cuda.current_device()}, not {current}"

    torch.cuda.set_device(current)
    rng = np.random.default_rng(77)
    desc, vals = randgraph.random_operand(rng, depth=4, size_hint=120, cplx=False, m=M, n=N)
    A = bfref.from_desc(desc, vals)
    gam_h = rng.random(N) + 0.1
    row_perm = rng.permutation(M)
    rev = np.empty(M, dtype=np.int64); rev[row_perm] = np.arange(M)
    missing = row_perm.copy()
    other = (rev[4] + 1) % M
    missing[rev[4]] = missing[other]                                   # no row lands on index 4 any more
    obs = np.array([o for o in (100, 17, 60, 33) if o != missing[other]][:K])
    noise = np.full(K, 0.1)
    dev = torch.device("cuda", target)
    on_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gam, perm, bad_perm = on_dev(gam_h), on_dev(row_perm.astype(np.int64)), on_dev(missing.astype(np.int64))
    X, V, W = on_dev(rng.standard_normal((N, Q))), on_dev(rng.standard_normal((M, Q))), on_dev(rng.standard_normal((N, Q)))
    here("the uploads")
    out = {}

    op = HipOperator.from_bfmat(A.ptr.value, flags=_capi.FLAG_ADJOINT, device=target)
    here("compile")
    lib = op._lib
    assert lib.bfhipOperatorDevice(op.handle) == target
    out["apply"] = op.apply_device(X); here("apply")
    out["applyT"] = op.apply_transpose_device(V); here("transposed apply")
    lib.bfhipOperatorReserveRhs.argtypes, lib.bfhipOperatorReserveRhs.restype = [C.c_void_p, C.c_uint32], C.c_int
    _capi.check(lib.bfhipOperatorReserveRhs(op.handle, 8)); here("reserve")             # the applies above made it 2 wide
    out["sample"] = op.cov_sample_block_device(gam, perm, W); here("block sample")
    s, sq = torch.zeros(M, dtype=torch.float64, device=dev), torch.zeros(M, dtype=torch.float64, device=dev)
    op.cov_moments_device(gam, perm, 11, 0, 5, 2, s, sq); here("moments")
    out["sum"], out["sumsq"] = s, sq

    cond = op.cov_condition(gam, perm, obs, noise); here("create")
    with pytest.raises(_capi.BfhipError) as ei:
        op.cov_condition(gam, bad_perm, np.array([100, 4, 17]), noise)
    assert ei.value.code == 1 and "exactly once" in str(ei.value)
    here("create failing after the switch")
    y = on_dev(rng.standard_normal(K))
    out["draw"] = cond.draw(y, 5, 6, 0, 1); here("draw")
    out["lik"], out["gradGamma"], out["gradNoise"] = cond.log_likelihood(y, grad_log_gamma=True, grad_noise=True); here("log-likelihood")
    out["variance"] = cond.variance([30, 7]); here("variance")
    bad = op.cov_condition(gam, bad_perm, obs, noise); here("create on the damaged permutation")
    with pytest.raises(_capi.BfhipError) as ei:
        bad.variance([int(obs[0]), 4])
    assert ei.value.code == 1 and "exactly once" in str(ei.value)
    here("variance failing after the switch")
    bad.close(); here("free of a conditioning object")

    out["extract"] = op.extract(rows=[0, 5, 100, 210], cols=[1, 2, 50, 92]); here("extraction")
    assert out["extract"].device == dev
    path = tmp_path / f"op{current}.bfhip"
    op.save(path); here("save")
    loaded = HipOperator.load(path, device=target); here("load")
    assert lib.bfhipOperatorDevice(loaded.handle) == target
    out["loadedApply"] = loaded.apply_device(X); here("apply of the loaded operator")
    assert torch.equal(out["loadedApply"], out["apply"])
    loaded.close(); here("free of the loaded operator")
    cond.close(); op.close(); here("free")
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_every_entry_hands_the_callers_device_back(tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    try:
        away = run_sequence(0, tmp_path)
        home = run_sequence(1, tmp_path)
    finally:
        torch.cuda.set_device(0)
    assert sorted(away) == sorted(home)
    for name in away:
        assert np.array_equal(away[name], home[name]), name
