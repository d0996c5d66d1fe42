"""The complex64 block kernels (bfhipSetRhsBlocks, bfStageKernelC64Mfma*) on the GPU.

* every catalogue case as a complex64 operand with the switch on, forward, at nrhs across every tile edge: the componentwise
  bound of tests/highprec.py (unchanged), the device entry into a NaN-filled dY, determinism, NaN taint;
* nrhs below minRhs, the switch off again, and the transposed apply: bit-identical to an operator whose switch was never touched;
* the two bounds of tests/test_gpu_c64.py with the switch on: the N = 2048 multilevel golden and that file's graph shapes;
* the callers: extract equals the apply on unit panels bit for bit, refinement takes the same outer steps, a loaded operator
  takes the switch, and a captured apply replays to the same bits."""
import os

import numpy as np
import pytest

import kernel_catalogue as kc
from test_gpu_c64 import TOL_OP, TOL_ROUNDED, _SHAPES, _crandn, _round, rel

pytestmark = pytest.mark.gpu

NRHS = (2, 3, 16, 17, 20, 33, 64, 70, 80)
C64 = kc.C64


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _device_apply(op, x, t=False):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    m, n = op.shape
    yd = torch.full(((n if t else m), x.shape[1]), float("nan"), dtype=torch.complex64, device="cuda:0")
    if t:
        op.apply_transpose_device(xd, yd)
    else:
        op.apply_device(xd, yd)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_catalogue_on_the_block_kernels(name):
    from butterfly_amd.operator import HipOperator
    from highprec import Reference
    case = kc.BY_NAME[name]
    desc, vals, demote = kc.materialize(case, C64)
    ref = Reference(desc, vals, C64)
    rng = np.random.default_rng(case.seed + 11)
    for flags in kc.flag_sets(case, C64):
        op = HipOperator.from_desc(desc, vals, flags=flags, max_rhs=max(NRHS), demote_to_f32=demote, device=0, rhs_blocks=2)
        plain = HipOperator.from_desc(desc, vals, flags=flags, max_rhs=max(NRHS), demote_to_f32=demote, device=0)
        m, n = op.shape
        first = {}
        for nrhs in NRHS:
            where = f"flags {flags:#x} nrhs {nrhs}"
            x = ref.rounded(kc.draw_x(case, C64, n, nrhs, rng))
            host = op.apply_host(x)
            try:
                ref.check(host, x, transpose=False)
            except AssertionError as e:
                raise AssertionError(f"{where}: {e}") from None
            y1 = _device_apply(op, x)
            assert np.isfinite(y1).all(), f"{where}: {int((~np.isfinite(y1)).sum())} outputs never written"
            assert np.array_equal(_bits(y1), _bits(host.astype(np.complex64))), f"{where}: device entry != host entry"
            y2 = _device_apply(op, x)
            assert np.array_equal(_bits(y1), _bits(y2)), f"{where}: two applies differ"
            first[nrhs] = (x, y1)
            # NaN taint: one input entry of the last right-hand side
            j = int(rng.integers(n))
            xn = x.copy()
            xn[j, nrhs - 1] = np.nan
            bad = ~np.isfinite(_device_apply(op, xn))
            want = np.zeros_like(bad)
            want[:, nrhs - 1] = ref.structural(j, transpose=False)
            assert np.array_equal(bad, want), (f"{where}: NaN at input {j} reached {int((bad & ~want).sum())} outputs it does not feed "
                                               f"and missed {int((want & ~bad).sum())}")
            assert np.array_equal(_bits(_device_apply(op, x)), _bits(y1)), f"{where}: state carried over from the NaN apply"
        # below minRhs, with the switch off again, and transposed: the bits of an operator whose switch was never touched
        x1 = ref.rounded(kc.draw_x(case, C64, n, 1, rng))
        assert np.array_equal(_bits(_device_apply(op, x1)), _bits(_device_apply(plain, x1))), f"flags {flags:#x}: nrhs 1 changed"
        for nrhs in (2, 17, 80):
            xt = ref.rounded(kc.draw_x(case, C64, m, nrhs, rng))
            assert np.array_equal(_bits(_device_apply(op, xt, True)), _bits(_device_apply(plain, xt, True))), f"flags {flags:#x}: transposed nrhs {nrhs} changed"
        op.set_rhs_blocks(17)
        x16 = first[16][0]
        assert np.array_equal(_bits(_device_apply(op, x16)), _bits(_device_apply(plain, x16))), f"flags {flags:#x}: nrhs 16 < minRhs 17 changed"
        assert np.array_equal(_bits(_device_apply(op, first[17][0])), _bits(first[17][1]))
        op.set_rhs_blocks(0)
        for nrhs in NRHS:
            x = first[nrhs][0]
            assert np.array_equal(_bits(_device_apply(op, x)), _bits(_device_apply(plain, x))), f"flags {flags:#x}: switch off, nrhs {nrhs} changed"
        op.close(); plain.close()


def _check_bounds(desc, vals, nrhs_list, rng):
    from butterfly_amd.operator import HipOperator
    mx = max(nrhs_list)
    op = HipOperator.from_desc(desc, vals, max_rhs=mx, demote_to_f32=True, rhs_blocks=2)
    ref = HipOperator.from_desc(desc, vals, max_rhs=mx)
    ref_r = HipOperator.from_desc(desc, {k: _round(v) for k, v in vals.items()}, max_rhs=mx)
    m, n = op.shape
    for nrhs in nrhs_list:
        x = _crandn(rng, n, nrhs)
        y = op.apply_host(x)
        print(f"nrhs={nrhs} vs c128 {rel(y, ref.apply_host(x)):.3e} vs rounded {rel(y, ref_r.apply_host(_round(x))):.3e}")
        assert rel(y, ref.apply_host(x)) <= TOL_OP, nrhs
        assert rel(y, ref_r.apply_host(_round(x))) <= TOL_ROUNDED, nrhs
    for o in (op, ref, ref_r):
        o.close()


def test_golden_multilevel_bounds(helm2_cases):
    from butterfly_amd.operator import HipOperator
    from oracle import bfref
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "helm2_multilevel_n2048_k128_vectors.npz"))
    desc, tp, vals = helm2_cases(int(z["n"]), float(z["k"]))
    _check_bounds(desc, vals, [2, 3, 17, 64], np.random.default_rng(1))
    op = HipOperator.from_desc(desc, vals, demote_to_f32=True, max_rhs=3, rhs_blocks=2)
    x = np.stack([z["x"], 2.0 * z["x"], -z["x"]], axis=1)
    y = op.apply_host(x)
    want_r = bfref.mat_mul(bfref.from_desc(desc, {k: _round(v) for k, v in vals.items()}), _round(z["x"]))
    for q, s in enumerate((1.0, 2.0, -1.0)):
        assert rel(y[:, q], s * z["y_oracle"]) <= TOL_OP
        assert rel(y[:, q], s * want_r) <= TOL_ROUNDED
    op.close()


@pytest.mark.parametrize("case", range(len(_SHAPES)), ids=[c[0] for c in _SHAPES])
def test_graph_shapes_bounds(case):
    _, d, v = _SHAPES[case]
    _check_bounds(d, v, [2, 3, 17, 64], np.random.default_rng(case))


def test_extract_equals_the_apply_on_unit_panels(helm2_cases):
    import torch
    from butterfly_amd.operator import HipOperator
    desc, tp, vals = helm2_cases(2048, 128)
    op = HipOperator.from_desc(desc, vals, demote_to_f32=True, max_rhs=64, rhs_blocks=2)
    plain = HipOperator.from_desc(desc, vals, demote_to_f32=True, max_rhs=64)
    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, 2048, size=200), rng.integers(0, 2048, size=300)
    blk = op.extract(rows, cols).cpu().numpy()
    assert blk.shape == (200, 300)
    differs = False
    for c0 in range(0, 300, 64):
        idx = cols[c0:c0 + 64]
        x = np.zeros((2048, len(idx)), dtype=np.complex64)
        x[idx, np.arange(len(idx))] = 1.0
        y = _device_apply(op, x)
        assert np.array_equal(_bits(blk[:, c0:c0 + 64]), _bits(y[rows])), c0
        differs = differs or not np.array_equal(_bits(y), _bits(_device_apply(plain, x)))
    assert rel(blk, plain.extract(rows, cols).cpu().numpy()) <= TOL_ROUNDED
    print("block path differs from the default path in some bit:", differs)
    op.close(); plain.close()


def test_refinement_takes_the_same_outer_steps():
    import torch
    import bie
    from butterfly_amd.operator import HipOperator
    N = 2048
    desc, root, vals, dense = bie.second_kind_case(N, 128)
    op = HipOperator.from_desc(desc, vals, root=root, max_rhs=8)
    low = HipOperator.from_desc(desc, vals, root=root, max_rhs=8, demote_to_f32=True)
    rng = np.random.default_rng(7)
    b = torch.from_numpy(rng.standard_normal((N, 8)) + 1j * rng.standard_normal((N, 8))).to("cuda:0")
    x0, k0, inner0, res0, hist0 = op.solve_gmres_refine_device(b, low, tol=1e-12)
    low.set_rhs_blocks(2)
    x1, k1, inner1, res1, hist1 = op.solve_gmres_refine_device(b, low, tol=1e-12)
    print(f"switch off: outer {k0} inner {inner0} res {res0:.3e}; on: outer {k1} inner {inner1} res {res1:.3e}")
    assert res0 <= 1e-12 and res1 <= 1e-12 and k1 == k0
    assert rel(x1.cpu().numpy(), np.linalg.solve(dense, b.cpu().numpy())) <= 1e-10
    op.close(); low.close()


def test_a_loaded_operator_takes_the_switch(helm2_cases, tmp_path):
    from butterfly_amd.operator import HipOperator
    desc, tp, vals = helm2_cases(2048, 128)
    op = HipOperator.from_desc(desc, vals, max_rhs=20, demote_to_f32=True, rhs_blocks=2)
    op.save(tmp_path / "c64.bfhip")
    back = HipOperator.load(tmp_path / "c64.bfhip", max_rhs=20, rhs_blocks=2)
    off = HipOperator.load(tmp_path / "c64.bfhip", max_rhs=20)
    x = _crandn(np.random.default_rng(3), 2048, 20).astype(np.complex64)
    y = _device_apply(op, x)
    assert np.array_equal(_bits(_device_apply(back, x)), _bits(y))
    op.set_rhs_blocks(0)
    assert np.array_equal(_bits(_device_apply(off, x)), _bits(_device_apply(op, x)))
    for o in (op, back, off):
        o.close()


def test_block_apply_can_be_captured_in_a_hip_graph():
    import torch
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.operator import HipOperator
    n = 8192
    desc, perm = hs.native_multilevel_structure(hs.circle_points(n), n / 16)
    op = HipOperator.from_desc(desc, None, seed=3, max_rhs=20, demote_to_f32=True, rhs_blocks=2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.randn((n, 20), dtype=torch.complex64, device="cuda")
        y = torch.empty_like(x)
        op.apply_device(x, y)
        s.synchronize()
        y0 = y.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            op.apply_device(x, y)
        y.zero_()
        g.replay()
        s.synchronize()
        assert torch.equal(y, y0)
    op.close()
