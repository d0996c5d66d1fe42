"""Complex64 output of the device Helmholtz builder (BfhipHelm2Problem.outDtype = BFHIP_C64) and the one-build operator pair
(bfhipBuildHelm2Pair).  The packing is checked bit for bit against the host packer: a descriptor compiled from the builder's own
double-precision leaves under demote_to_f32 has the same plan, hence must hold the same arena.  tests/test_build_c64_cpu.py
checks that the operands used here contain every piece layout of a complex64 plan."""
import numpy as np
import pytest

import build_c64_cases as bc

pytestmark = pytest.mark.gpu

TOL_OP = 1e-5      # a complex64 operator against a complex128 truth (tests/test_gpu_c64.py)


def rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rand(n, nrhs, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, nrhs)) + 1j * rng.standard_normal((n, nrhs))


# ---- 1. bit-exact packing -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def thin():
    """The thin-leaf block, its decorations, and the builder's own double-precision leaves, one by one, on the host."""
    from butterfly_amd.operator import helm2_build_leaf
    desc, pts = bc.thin_leaf_block()
    k = 40.0
    deco = bc.thin_leaf_problem()
    vals = {node: helm2_build_leaf(pts, k, rc, **deco) for node, rc in desc.recipe.items()}
    return desc, pts, k, deco, vals


def test_control_a_leaf_built_alone_equals_the_leaf_built_in_a_batch(thin):
    """The premise of the next test, on complex128 (passes without the feature)."""
    from butterfly_amd.operator import HipOperator
    desc, pts, k, deco, vals = thin
    built, st = HipOperator.build_helm2(desc, pts, k, **deco)
    host = HipOperator.from_desc(desc, vals)
    assert st["kernelLeaves"] == 40 and st["reexpLeaves"] == 0
    x = _rand(desc.cols[desc.root], 3, 1)
    assert np.array_equal(built.apply_host(x), host.apply_host(x))
    built.close(); host.close()


def test_complex64_arena_is_the_host_packers_bit_for_bit(thin, tmp_path):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    desc, pts, k, deco, vals = thin
    m, n = desc.rows[desc.root], desc.cols[desc.root]
    built, st = HipOperator.build_helm2(desc, pts, k, out_dtype=_capi.BFHIP_C64, flags=_capi.FLAG_ADJOINT, **deco)
    host = HipOperator.from_desc(desc, vals, demote_to_f32=True, flags=_capi.FLAG_ADJOINT)
    assert built.dtype == host.dtype == _capi.BFHIP_C64 and built.shape == (m, n)
    sb, sh = built.stats(), host.stats()
    assert all(sb[f] == sh[f] for f in ("numStages", "numItems", "numPieces", "leafBytes", "arenaBytes"))
    x1, x3, x5, xt = _rand(n, 1, 2)[:, 0], _rand(n, 3, 3), _rand(n, 5, 4), _rand(m, 2, 5)
    want1, want3, wantt = host.apply_host(x1), host.apply_host(x3), host.apply_transpose_host(xt)
    assert np.all(np.isfinite(want3)) and np.linalg.norm(want3) > 0
    assert np.array_equal(built.apply_host(x1), want1)
    assert np.array_equal(built.apply_host(x3), want3)
    assert np.array_equal(built.apply_transpose_host(xt), wantt)
    # the complex64 RHS-block kernels read the same arena
    built.set_rhs_blocks(2); host.set_rhs_blocks(2)
    want5 = host.apply_host(x5)
    assert np.array_equal(built.apply_host(x5), want5)
    built.set_rhs_blocks(0); host.set_rhs_blocks(0)
    # more than one batch: the same arena
    small, st2 = HipOperator.build_helm2(desc, pts, k, out_dtype=_capi.BFHIP_C64, flags=_capi.FLAG_ADJOINT, workspace_bytes=1 << 20, **deco)
    assert st2["numBatches"] > 1 and st["numBatches"] == 1
    assert np.array_equal(small.apply_host(x3), want3) and np.array_equal(small.apply_transpose_host(xt), wantt)
    small.close()
    # save -> load
    path = tmp_path / "thin_c64.bfhip"
    built.save(path)
    back = HipOperator.load(path)
    assert back.dtype == _capi.BFHIP_C64
    assert np.array_equal(back.apply_host(x3), want3) and np.array_equal(back.apply_transpose_host(xt), wantt)
    back.close(); built.close(); host.close()


# ---- 2. / 3. a real butterfly: the second-kind system of tests/test_gpu_build.py ----------------------------------------------
N2, K2 = 2048, 64.0


@pytest.fixture(scope="module")
def second_kind(helm2_cases):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from oracle import helm2_build as hb
    desc, tp, _ = helm2_cases(N2, K2)
    nrm = tp.copy()
    w = np.full(N2, 2 * np.pi / N2)
    deco = dict(layer_pot="Sp", normals=nrm, col_weights=w, self_value=0.5)
    dense = 0.5 * np.eye(N2) + hb.kernel_matrix_sp(K2, tp, tp, nrm) * w[None, :]
    op, st = HipOperator.build_helm2(desc, tp, K2, **deco)
    low, st_low = HipOperator.build_helm2(desc, tp, K2, out_dtype=_capi.BFHIP_C64, **deco)
    d = np.array([np.cos(0.3), np.sin(0.3)])
    b = 1j * K2 * (nrm @ d) * np.exp(1j * K2 * (tp @ d))      # normal derivative of a plane wave on the circle
    yield dict(desc=desc, tp=tp, deco=deco, dense=dense, op=op, st=st, low=low, st_low=st_low, b=b, x=hb.complex_randn(N2, 0))
    op.close(); low.close()


COUNTS = ("kernelLeaves", "reexpLeaves", "kernelEvals")


def test_complex64_butterfly_against_the_dense_matrix(second_kind):
    from butterfly_amd import _capi
    s = second_kind
    op, low, x = s["op"], s["low"], s["x"]
    assert low.dtype == _capi.BFHIP_C64 and s["st_low"]["notConverged"] == 0
    err = rel(low.apply_host(x), s["dense"] @ x)
    print(f"complex64-built operator vs dense: {err:.3e}; complex128-built: {rel(op.apply_host(x), s['dense'] @ x):.3e}")
    assert err <= TOL_OP
    assert 2 * low.stats()["leafBytes"] == op.stats()["leafBytes"]
    for f in COUNTS + ("qrProblems", "sumSweeps", "truncated"):
        assert s["st_low"][f] == s["st"][f], f
    assert s["st_low"]["kernelLeaves"] + s["st_low"]["reexpLeaves"] == len(s["desc"].recipe) and s["st_low"]["reexpLeaves"] > 0
    bj, info = low.block_jacobi()
    assert bj.dtype == _capi.BFHIP_C64 and bj.shape == (N2, N2)
    bj.close()
    rows = np.arange(1000, 1064)
    d64, d128 = low.extract(rows=rows, device=False), op.extract(rows=rows, device=False)
    assert d64.shape == (64, N2) and rel(d64, d128) <= TOL_OP


@pytest.fixture(scope="module")
def pair(second_kind):
    from butterfly_amd.operator import HipOperator
    s = second_kind
    op, low, st = HipOperator.build_helm2_pair(s["desc"], s["tp"], K2, **s["deco"])
    yield op, low, st
    op.close(); low.close()


def test_pair_is_one_build_and_two_single_builds_bit_for_bit(second_kind, pair):
    from butterfly_amd import _capi
    s, x = second_kind, second_kind["x"]
    op, low, st = pair
    assert op.dtype == _capi.BFHIP_C128 and low.dtype == _capi.BFHIP_C64 and st["notConverged"] == 0
    assert np.array_equal(op.apply_host(x), s["op"].apply_host(x))
    assert np.array_equal(low.apply_host(x), s["low"].apply_host(x))
    for f in COUNTS + ("sumSweeps", "qrProblems", "numBatches"):
        assert st[f] == s["st"][f], f                      # once, not twice


def test_refinement_on_the_pair(second_kind, pair):
    """The pair is the two operators of the mixed-precision refinement.  Measured on an MI355X: 2 outer steps, residual
    history 1, 1.0e-6, 9.9e-13; rel-l2 against plain complex128 GMRES (74 iterations) 6.6e-13; with the complex64 operator's
    block-Jacobi inverse as inner preconditioner 3 outer steps to 6.3e-15."""
    import time
    op, low, _ = pair
    b = _dev(second_kind["b"])
    t0 = time.perf_counter()
    xr, outer, inner, res, hist = op.solve_gmres_refine_device(b, low, tol=1e-12)
    t1 = time.perf_counter()
    xg, iters, res_g = op.solve_gmres_device(b, tol=1e-12, max_num_iter=400)
    t2 = time.perf_counter()
    agree = rel(xr.cpu().numpy(), xg.cpu().numpy())
    print(f"refinement on the pair: outer={outer} inner={inner} res={res:.3e} hist={hist} ({t1 - t0:.2f} s); "
          f"GMRES iters={iters} res={res_g:.3e} ({t2 - t1:.2f} s); rel-l2 of the two x {agree:.3e}")
    assert res <= 1e-12
    assert agree <= 1e-10
    pre, _ = low.block_jacobi()
    t3 = time.perf_counter()
    xp, outer_p, inner_p, res_p, _ = op.solve_gmres_refine_device(b, low, tol=1e-12, precond=pre)
    print(f"with block-Jacobi of the complex64 operator: outer={outer_p} inner={inner_p} res={res_p:.3e} ({time.perf_counter() - t3:.2f} s)")
    assert res_p <= 1e-12
    pre.close()


# ---- 4. shards and the one-call entry ---------------------------------------------------------------------------------------
def test_complex64_row_shards_against_the_oracle(helm2_cases):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from oracle import bfref, helm2_build as hb
    n, k = 4096, 100.0
    desc, tp, vals = helm2_cases(n, k)
    x = hb.complex_randn(n, 0)
    y_cpu = bfref.mat_mul(bfref.from_desc(desc, vals), x)
    nrb = len(desc.meta["top_rows"])
    parts = []
    for b, e in ((0, 5), (5, nrb)):
        op, st = HipOperator.build_helm2(desc, tp, k, out_dtype=_capi.BFHIP_C64, row_blocks=(b, e))
        assert op.dtype == _capi.BFHIP_C64 and st["kernelLeaves"] + st["reexpLeaves"] < len(desc.recipe)
        parts.append(op.apply_host(x))
        op.close()
    err = rel(np.concatenate(parts), y_cpu)
    print(f"complex64 row shards vs oracle: {err:.3e}")
    assert err <= TOL_OP


def test_complex64_evaluation_operator_in_one_native_call():
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from oracle import helm2_build as hb
    n, m, k = 3000, 1500, 90.0
    t, u = 2 * np.pi * np.arange(n) / n, 2 * np.pi * np.arange(m) / m
    pts = np.stack([np.cos(t), 0.5 * np.sin(t)], axis=1)
    tgt = 2.5 * np.stack([np.cos(u), np.sin(u)], axis=1)
    w = (2 * np.pi / n) * np.hypot(np.sin(t), 0.5 * np.cos(t))
    ev, (ps, pt), st = HipOperator.fac_helm2_make_multilevel(pts, k, col_weights=w, tgt_points=tgt, out_dtype=_capi.BFHIP_C64)
    assert ev.shape == (m, n) and ev.dtype == _capi.BFHIP_C64 and st["notConverged"] == 0
    x = hb.complex_randn(n, 2)
    err = rel(ev.apply_host(x[ps]), ((hb.kernel_matrix(k, pts, tgt) * w[None, :]) @ x)[pt])
    print(f"complex64 evaluation operator vs dense kernel: {err:.3e}")
    assert err <= TOL_OP
    ev.close()


def test_pair_whose_low_half_is_a_row_shard(second_kind):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    s = second_kind
    desc, tp, x = s["desc"], s["tp"], s["x"]
    nrb = len(desc.meta["top_rows"])
    shard = (1, max(2, nrb // 2))
    op, low, st = HipOperator.build_helm2_pair(desc, tp, K2, low_opts=dict(row_blocks=shard), **s["deco"])
    single, st1 = HipOperator.build_helm2(desc, tp, K2, out_dtype=_capi.BFHIP_C64, row_blocks=shard, **s["deco"])
    assert low.shape == single.shape and low.shape[0] < N2 and st1["kernelLeaves"] + st1["reexpLeaves"] < len(desc.recipe)
    assert np.array_equal(op.apply_host(x), s["op"].apply_host(x))
    assert np.array_equal(low.apply_host(x), single.apply_host(x))
    for f in COUNTS:
        assert st[f] == s["st"][f], f                      # the union of the two plans' leaves is the whole operator, built once
    single.close()
    # and the other way round: the complex128 half is the shard, the complex64 one the whole operator
    op2, low2, st2 = HipOperator.build_helm2_pair(desc, tp, K2, row_blocks=shard, low_opts=dict(), **s["deco"])
    single, _ = HipOperator.build_helm2(desc, tp, K2, row_blocks=shard, **s["deco"])
    assert np.array_equal(op2.apply_host(x), single.apply_host(x))
    assert np.array_equal(low2.apply_host(x), s["low"].apply_host(x))
    for o in (op, low, op2, low2, single):
        o.close()
