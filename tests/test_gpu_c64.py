"""Complex64 operators on the GPU (BFHIP_C64: demoteToF32 on a complex128 operand).

Two bounds: against the complex128 operator (the oracle's answer: tests/test_gpu_parity.py holds it to 1e-12 of the oracle)
rel-l2 <= 1e-5, and against the complex128 operator built from the complex64-rounded leaves applied to the rounded x
rel-l2 <= 1e-6 (what is left is the kernels' own rounding: double accumulation, one float rounding per stage output)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_OP, TOL_ROUNDED = 1e-5, 1e-6


def rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def _round(v):
    return v.astype(np.complex64).astype(np.complex128)


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _check_pair(desc, vals, flags, nrhs_list, rng, device_entry=True):
    import torch
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    mx = max(nrhs_list)
    op = HipOperator.from_desc(desc, vals, flags=flags, max_rhs=mx, demote_to_f32=True)
    assert op.stats()["dtype"] == _capi.BFHIP_C64
    ref = HipOperator.from_desc(desc, vals, flags=flags, max_rhs=mx)
    ref_r = HipOperator.from_desc(desc, {k: _round(v) for k, v in vals.items()}, flags=flags, max_rhs=mx)
    m, n = op.shape
    adj = flags & (_capi.FLAG_ADJOINT | _capi.FLAG_ADJOINT_PACKED)
    for nrhs in nrhs_list:
        for t in ((False, True) if adj else (False,)):
            x = _crandn(rng, m if t else n, nrhs)
            f = (lambda o, v: o.apply_transpose_host(v)) if t else (lambda o, v: o.apply_host(v))
            y = f(op, x)
            assert y.dtype == np.complex128
            assert rel(y, f(ref, x)) <= TOL_OP, (nrhs, t)
            assert rel(y, f(ref_r, _round(x))) <= TOL_ROUNDED, (nrhs, t)
            if device_entry:
                xd = torch.from_numpy(x.astype(np.complex64)).to("cuda:0")
                yd = op.apply_transpose_device(xd) if t else op.apply_device(xd)
                torch.cuda.synchronize()
                assert yd.dtype == torch.complex64
                # the device entry computes what the host entry computes: the host entry only converts x and y
                assert np.array_equal(yd.cpu().numpy(), y.astype(np.complex64)), (nrhs, t)
    for o in (op, ref, ref_r):
        o.close()


@pytest.mark.parametrize("adjoint", ["shared", "packed"])
def test_golden_multilevel_forward_and_adjoint(helm2_cases, adjoint):
    from butterfly_amd import _capi
    from oracle import bfref
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "helm2_multilevel_n2048_k128_vectors.npz"))
    desc, tp, vals = helm2_cases(int(z["n"]), float(z["k"]))
    flags = _capi.FLAG_ADJOINT if adjoint == "shared" else _capi.FLAG_ADJOINT_PACKED
    _check_pair(desc, vals, flags, [1, 2, 3, 17, 64], np.random.default_rng(1))
    from butterfly_amd.operator import HipOperator
    op = HipOperator.from_desc(desc, vals, demote_to_f32=True)
    assert rel(op.apply_host(z["x"]), z["y_oracle"]) <= TOL_OP
    assert rel(op.apply_host(z["x"]), bfref.mat_mul(bfref.from_desc(desc, {k: _round(v) for k, v in vals.items()}), _round(z["x"]))) <= TOL_ROUNDED
    op.close()


def _shape_cases():
    import randgraph
    from test_c64_cpu import _complexify
    rng = np.random.default_rng(9)
    for seed, depth in ((0, 3), (1, 5), (2, 7), (3, 9)):
        d, v = randgraph.random_operand(np.random.default_rng(900 + seed), depth=depth, cplx=True, coo=False)
        yield f"randgraph{seed}_depth{depth}", d, v
    d, v, _ = randgraph.few_row_operand(rng)
    yield ("few_row",) + _complexify(rng, d, v)
    d, v, _ = randgraph.narrow_items_operand(rng)
    yield ("narrow_items",) + _complexify(rng, d, v)
    d, v, _ = randgraph.few_row_column_operand(rng, 40, 2100)
    yield ("wide_tall_column",) + _complexify(rng, d, v)
    d, v, _, _ = randgraph.long_contraction_operand(rng, 0)
    yield "long_contraction", d, v


_SHAPES = list(_shape_cases())


@pytest.mark.parametrize("case", range(len(_SHAPES)), ids=[c[0] for c in _SHAPES])
def test_graph_shapes_forward_and_transposed(case):
    from butterfly_amd import _capi
    _, d, v = _SHAPES[case]
    _check_pair(d, v, _capi.FLAG_ADJOINT, [1, 3], np.random.default_rng(case))
    _check_pair(d, v, _capi.FLAG_ADJOINT_PACKED, [1, 2], np.random.default_rng(case + 50), device_entry=False)


def test_synthetic_leaves_are_the_packed_host_values_bit_for_bit():
    import randgraph
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from test_c64_cpu import _synthetic_values
    desc, _ = randgraph.random_operand(np.random.default_rng(77), depth=4, cplx=True)
    host = _synthetic_values(desc, 1234)
    syn = HipOperator.from_desc(desc, None, seed=1234, flags=_capi.FLAG_ADJOINT, demote_to_f32=True, max_rhs=3)
    hst = HipOperator.from_desc(desc, host, flags=_capi.FLAG_ADJOINT, demote_to_f32=True, max_rhs=3)
    m, n = syn.shape
    x = _crandn(np.random.default_rng(2), n, 3)
    y = syn.apply_host(x)
    assert np.array_equal(y, hst.apply_host(x)) and np.array_equal(y, syn.apply_host(x))
    v = _crandn(np.random.default_rng(3), m, 1)
    assert np.array_equal(syn.apply_transpose_host(v), hst.apply_transpose_host(v))
    syn.close(); hst.close()


def test_shim_over_a_complex64_operator(helm2_cases):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from oracle import bfref, helm2_build as hb
    from test_gpu_parity import _handle
    n, k = 1024, 64
    desc, tp, vals = helm2_cases(n, k)
    dense = bfref.mat_mul(bfref.from_desc(desc, vals), np.eye(n, dtype=np.complex128))
    x = hb.complex_randn(n * 3, 5).reshape(n, 3)
    lib = bfref.load()
    op = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_ADJOINT, max_rhs=3, demote_to_f32=True)
    a_hip = C.c_void_p(op.as_bfmat())
    h = _handle(a_hip, (n, n))
    assert rel(bfref.mat_mul(h, x), dense @ x) <= TOL_OP
    assert rel(bfref.mat_rmul(h, np.ascontiguousarray(x.T)), x.T @ dense) <= TOL_OP
    lib.bfMatTranspose(a_hip)
    assert rel(bfref.mat_mul(h, x), dense.conj().T @ x) <= TOL_OP
    assert rel(bfref.mat_mul(h, x[:, ::2]), dense.conj().T @ x[:, ::2]) <= TOL_OP
    lib.bfMatTranspose(a_hip)
    assert rel(bfref.mat_mul(h, x), dense @ x) <= TOL_OP
    # MulVec / RmulVec take a BfVecReal: real operators only, as for complex128
    with pytest.raises(Exception):
        bfref.mat_mul_vec(h, np.ones(n))
    lib.bfMatDelete(C.byref(a_hip))
    op.close()


def test_save_load_round_trip(helm2_cases, tmp_path):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from oracle import helm2_build as hb
    desc, tp, vals = helm2_cases(2048, 128)
    op = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_ADJOINT_PACKED, max_rhs=2, demote_to_f32=True)
    big = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_ADJOINT_PACKED, max_rhs=2)
    assert op.stats()["arenaBytes"] <= 0.55 * big.stats()["arenaBytes"]
    big.close()
    op.save(tmp_path / "c64.bfhip")
    back = HipOperator.load(tmp_path / "c64.bfhip")
    assert back.stats()["dtype"] == _capi.BFHIP_C64 and back.stats()["arenaBytes"] == op.stats()["arenaBytes"]
    x = hb.complex_randn(2048 * 2, 4).reshape(2048, 2)
    assert np.array_equal(back.apply_host(x), op.apply_host(x))
    assert np.array_equal(back.apply_transpose_host(x), op.apply_transpose_host(x))
    back.close(); op.close()


@pytest.mark.parametrize("mode", ["rows", "blocks"])
def test_rccl_sharded_one_rank_is_the_plain_apply(helm2_cases, mode):
    import torch
    from butterfly_amd import _capi
    from butterfly_amd.dist import RcclShardedApply, ShardLayout
    from butterfly_amd.operator import HipOperator
    from oracle import helm2_build as hb
    n, k = 4096, 100
    desc, tp, vals = helm2_cases(n, k)
    op = HipOperator.from_desc(desc, vals, max_rhs=3, flags=_capi.FLAG_ADJOINT, demote_to_f32=True)
    top_rows = desc.meta["top_rows"]
    layout = ShardLayout(top_rows, [0] * len(top_rows), 1)
    for nrhs in (1, 3):
        x = hb.complex_randn(n * nrhs, 3).reshape(n, nrhs)
        xd = torch.from_numpy(x.astype(np.complex64)).to("cuda:0")
        want, want_t = op.apply_device(xd).cpu().numpy(), op.apply_transpose_device(xd).cpu().numpy()
        step = RcclShardedApply(layout, 0, op, 0, nrhs=nrhs, mode=mode)
        got = step(xd)
        got_t = step.apply_transpose(xd)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_t.cpu().numpy(), want_t)
        step.close()
    op.close()


def test_row_range_shards_are_the_whole_operator_bit_for_bit():
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.dist import row_partition
    from butterfly_amd.operator import HipOperator
    from oracle import helm2_build as hb
    n, k, world = 16384, 1024.0, 4
    desc, perm = hs.native_multilevel_structure(hs.circle_points(n), k)
    cuts, _ = row_partition(desc, world)
    full = HipOperator.from_desc(desc, None, seed=5, demote_to_f32=True)
    x = hb.complex_randn(n, 8)
    y = full.apply_host(x)
    for r in range(world):
        part = HipOperator.from_desc(desc, None, seed=5, demote_to_f32=True, row_range=(int(cuts[r]), int(cuts[r + 1])))
        assert np.array_equal(part.apply_host(x), y[int(cuts[r]):int(cuts[r + 1])])
        part.close()
    full.close()


def test_refusals(helm2_cases):
    import torch
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    desc, tp, vals = helm2_cases(1024, 64)
    op = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_ADJOINT, demote_to_f32=True)
    b = np.ones(1024, dtype=np.complex128)
    with pytest.raises(_capi.BfhipError) as e:
        op.solve_gmres(b)
    assert e.value.code == 3 and "complex64" in str(e.value)
    c128 = HipOperator.from_desc(desc, vals)
    bd = torch.ones(1024, dtype=torch.complex128, device="cuda:0")
    with pytest.raises(_capi.BfhipError) as e:
        c128.solve_gmres_device(bd, precond=op)
    assert e.value.code == 3 and "complex64" in str(e.value)
    with pytest.raises(ValueError, match="complex64"):
        op.apply_device(bd)
    with pytest.raises(ValueError, match="complex64"):
        op.apply_transpose_device(bd)
    with pytest.raises(_capi.BfhipError):
        op.cov_sample_device(None, None, torch.ones(1024, dtype=torch.complex64, device="cuda:0"))
    c128.close(); op.close()


def test_c64_apply_is_faster_than_c128_at_n65536():
    """Alternated applies of the two compiles of the headline layout (synthetic, seed 1234) at N = 65536: the complex64 one
    reads half the bytes; its median is <= 0.75 of the complex128 median (expected ~0.55)."""
    import torch
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.operator import HipOperator
    n = 65536
    desc, perm = hs.native_multilevel_structure(hs.circle_points(n), n / 16.0)
    ops = [HipOperator.from_desc(desc, None, seed=1234, demote_to_f32=d) for d in (False, True)]
    xs = [torch.randn(n, dtype=t, device="cuda:0") for t in (torch.complex128, torch.complex64)]
    for o, x in zip(ops, xs):
        for _ in range(5):
            o.apply_device(x)
    torch.cuda.synchronize()
    times = [[], []]
    for _ in range(15):
        for i in (0, 1):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            ops[i].apply_device(xs[i])
            e.record()
            e.synchronize()
            times[i].append(s.elapsed_time(e))
    med = [float(np.median(t)) for t in times]
    assert med[1] <= 0.75 * med[0], med
    for o in ops:
        o.close()
