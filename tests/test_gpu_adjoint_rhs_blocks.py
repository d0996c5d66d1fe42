"""The adjoint plan's block kernels (bfhipSetAdjointRhsBlocks) on the GPU: bfStageKernelTMfma on shared-leaf plans, the forward
block kernels on packed ones.

* every catalogue case in all four element types and under every flag set, switch at 2, transposed, at nrhs across every tile
  edge: the componentwise bound of tests/highprec.py (unchanged), the device entry into a NaN-filled dY, device == host entry,
  determinism, NaN taint;
* nrhs below minRhs, the switch off again, and every forward apply: bit-identical to an operator whose switch was never touched;
* F32 cases whose shared-leaf transposed plan has no reduce (listed by tests/test_adjoint_rhs_blocks_cpu.py) also meet the tight
  bound of item sums formed in double and rounded once per stored level;
* the callers: extract via the adjoint equals the transposed apply on unit panels bit for bit, the saved file does not hold the
  switch, a loaded operator takes it, a captured transposed apply replays to the same bits, and the packed mode meets the bound."""
import functools

import numpy as np
import pytest

import kernel_catalogue as kc
from butterfly_amd import _capi
from test_adjoint_rhs_blocks_cpu import check_tight_T, reduce_free_cases_T

pytestmark = pytest.mark.gpu

NRHS = (2, 3, 16, 17, 20, 33, 64, 70, 80)
_PAIRS = [(c.name, dt) for c in kc.CASES for dt in kc.DTYPES]
_IDS = [f"{n}-{kc.DTYPE_NAMES[d]}" for n, d in _PAIRS]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _torch_dtype(dtype):
    import torch
    return {kc.C128: torch.complex128, kc.F64: torch.float64, kc.F32: torch.float32, kc.C64: torch.complex64}[dtype]


def _device_apply(op, x, dtype, t=True):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    m, n = op.shape
    yd = torch.full(((n if t else m), x.shape[1]), float("nan"), dtype=_torch_dtype(dtype), device="cuda:0")
    if t:
        op.apply_transpose_device(xd, yd)
    else:
        op.apply_device(xd, yd)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reduce_free():
    return frozenset(reduce_free_cases_T())


@pytest.mark.parametrize("name,dtype", _PAIRS, ids=_IDS)
def test_catalogue_on_the_adjoint_block_kernels(name, dtype):
    from butterfly_amd.operator import HipOperator
    from highprec import Reference
    case = kc.BY_NAME[name]
    st = kc.STORAGE_NP[dtype]
    desc, vals, demote = kc.materialize(case, dtype)
    ref = Reference(desc, vals, dtype)
    rng = np.random.default_rng(case.seed + 13)
    for flags in kc.flag_sets(case, dtype):
        tight = dtype == kc.F32 and flags & _capi.FLAG_ADJOINT and name in _reduce_free()
        op = HipOperator.from_desc(desc, vals, flags=flags, max_rhs=max(NRHS), demote_to_f32=demote, device=0, adjoint_rhs_blocks=2)
        plain = HipOperator.from_desc(desc, vals, flags=flags, max_rhs=max(NRHS), demote_to_f32=demote, device=0)
        assert op.stats()["dtype"] == dtype
        m, n = op.shape
        first = {}
        for nrhs in NRHS:
            where = f"flags {flags:#x} nrhs {nrhs}"
            x = ref.rounded(kc.draw_x(case, dtype, m, nrhs, rng))
            host = op.apply_transpose_host(x)
            try:
                worst = ref.check(host, x, transpose=True)
                if tight:
                    print(f"{where}: worst / bound {worst:.3g}, worst / tight bound {check_tight_T(ref, host, x):.3g}")
            except AssertionError as e:
                raise AssertionError(f"{where}: {e}") from None
            y1 = _device_apply(op, x, dtype)
            assert np.isfinite(y1).all(), f"{where}: {int((~np.isfinite(y1)).sum())} outputs never written"
            assert np.array_equal(_bits(y1), _bits(host.astype(st))), f"{where}: device entry != host entry"
            y2 = _device_apply(op, x, dtype)
            assert np.array_equal(_bits(y1), _bits(y2)), f"{where}: two applies differ"
            first[nrhs] = (x, y1)
            # NaN taint: one input entry of the last right-hand side
            j = int(rng.integers(m))
            xn = x.copy()
            xn[j, nrhs - 1] = np.nan
            bad = ~np.isfinite(_device_apply(op, xn, dtype))
            want = np.zeros_like(bad)
            want[:, nrhs - 1] = ref.structural(j, transpose=True)
            assert np.array_equal(bad, want), (f"{where}: NaN at input {j} reached {int((bad & ~want).sum())} outputs it does not feed "
                                               f"and missed {int((want & ~bad).sum())}")
            assert np.array_equal(_bits(_device_apply(op, x, dtype)), _bits(y1)), f"{where}: state carried over from the NaN apply"
        # below minRhs, with the switch off again, and forward: the bits of an operator whose switch was never touched
        x1 = ref.rounded(kc.draw_x(case, dtype, m, 1, rng))
        assert np.array_equal(_bits(_device_apply(op, x1, dtype)), _bits(_device_apply(plain, x1, dtype))), f"flags {flags:#x}: nrhs 1 changed"
        for nrhs in (1, 2, 17, 80):
            xf = ref.rounded(kc.draw_x(case, dtype, n, nrhs, rng))
            assert np.array_equal(_bits(_device_apply(op, xf, dtype, False)), _bits(_device_apply(plain, xf, dtype, False))), f"flags {flags:#x}: forward nrhs {nrhs} changed"
        op.set_adjoint_rhs_blocks(17)
        x16 = first[16][0]
        assert np.array_equal(_bits(_device_apply(op, x16, dtype)), _bits(_device_apply(plain, x16, dtype))), f"flags {flags:#x}: nrhs 16 < minRhs 17 changed"
        assert np.array_equal(_bits(_device_apply(op, first[17][0], dtype)), _bits(first[17][1]))
        op.set_adjoint_rhs_blocks(0)
        for nrhs in NRHS:
            x = first[nrhs][0]
            assert np.array_equal(_bits(_device_apply(op, x, dtype)), _bits(_device_apply(plain, x, dtype))), f"flags {flags:#x}: switch off, nrhs {nrhs} changed"
        op.close(); plain.close()


def test_the_tight_bound_covers_the_expected_cases():
    free = _reduce_free()
    assert "absorb_chain_70" in free and "coop_chain_97" in free, sorted(free)


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=[kc.DTYPE_NAMES[d] for d in kc.DTYPES])
def test_extract_via_adjoint_equals_the_transposed_apply_on_unit_panels(dtype):
    from butterfly_amd.operator import HipOperator
    case = kc.BY_NAME["randgraph5"]
    st = kc.STORAGE_NP[dtype]
    desc, vals, demote = kc.materialize(case, dtype)
    op = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_ADJOINT, demote_to_f32=demote, max_rhs=64, device=0, adjoint_rhs_blocks=2)
    m, n = op.shape
    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, m, size=150), rng.integers(0, n, size=min(n, 90))
    blk = op.extract(rows, cols, via_adjoint=True).cpu().numpy()
    assert blk.shape == (150, len(cols)) and blk.dtype == st
    for r0 in range(0, 150, 64):
        idx = rows[r0:r0 + 64]
        x = np.zeros((m, len(idx)), dtype=st)
        x[idx, np.arange(len(idx))] = 1.0
        y = _device_apply(op, x, dtype)                       # column k = row idx[k] of A
        assert np.array_equal(_bits(blk[r0:r0 + 64]), _bits(np.ascontiguousarray(y[cols].T))), r0
    op.close()


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=[kc.DTYPE_NAMES[d] for d in kc.DTYPES])
def test_the_file_does_not_hold_the_switch_and_a_loaded_operator_takes_it(dtype, tmp_path):
    from butterfly_amd.operator import HipOperator
    case = kc.BY_NAME["randgraph1"]
    desc, vals, demote = kc.materialize(case, dtype)
    kw = dict(flags=_capi.FLAG_ADJOINT, max_rhs=20, demote_to_f32=demote, device=0)
    op = HipOperator.from_desc(desc, vals, adjoint_rhs_blocks=2, **kw)
    plain = HipOperator.from_desc(desc, vals, **kw)
    op.save(tmp_path / "on.bfhip")
    plain.save(tmp_path / "plain.bfhip")
    assert (tmp_path / "on.bfhip").read_bytes() == (tmp_path / "plain.bfhip").read_bytes()
    back = HipOperator.load(tmp_path / "on.bfhip", max_rhs=20, device=0, adjoint_rhs_blocks=2)
    off = HipOperator.load(tmp_path / "on.bfhip", max_rhs=20, device=0)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((op.shape[0], 20))
    if dtype in (kc.C128, kc.C64):
        x = x + 1j * rng.standard_normal(x.shape)
    x = x.astype(kc.STORAGE_NP[dtype])
    y = _device_apply(op, x, dtype)
    assert np.array_equal(_bits(_device_apply(back, x, dtype)), _bits(y))
    assert np.array_equal(_bits(_device_apply(off, x, dtype)), _bits(_device_apply(plain, x, dtype)))
    op.set_adjoint_rhs_blocks(0)
    assert np.array_equal(_bits(_device_apply(off, x, dtype)), _bits(_device_apply(op, x, dtype)))
    for o in (op, plain, back, off):
        o.close()


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=[kc.DTYPE_NAMES[d] for d in kc.DTYPES])
def test_transposed_block_apply_can_be_captured_in_a_hip_graph(dtype):
    import torch
    from butterfly_amd.operator import HipOperator
    case = kc.BY_NAME["randgraph5"]
    desc, vals, demote = kc.materialize(case, dtype)
    op = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_ADJOINT, max_rhs=20, demote_to_f32=demote, device=0, adjoint_rhs_blocks=2)
    m, n = op.shape
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                  # one stream, no parallel branches
        x = torch.randn((m, 20), dtype=_torch_dtype(dtype), device="cuda")
        y = torch.empty((n, 20), dtype=_torch_dtype(dtype), device="cuda")
        op.apply_transpose_device(x, y)
        s.synchronize()
        y0 = y.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            op.apply_transpose_device(x, y)
        y.zero_()
        g.replay()
        s.synchronize()
        assert torch.equal(y, y0)
    op.close()


@pytest.mark.parametrize("dtype", (kc.C64, kc.F32), ids=["c64", "f32"])
def test_packed_adjoint_runs_the_forward_block_kernels_within_the_bound(dtype):
    from butterfly_amd.operator import HipOperator
    from highprec import Reference
    case = kc.BY_NAME["randgraph5"]
    desc, vals, demote = kc.materialize(case, dtype)
    ref = Reference(desc, vals, dtype)
    kw = dict(flags=_capi.FLAG_ADJOINT_PACKED, max_rhs=33, demote_to_f32=demote, device=0)
    op = HipOperator.from_desc(desc, vals, adjoint_rhs_blocks=2, **kw)
    plain = HipOperator.from_desc(desc, vals, **kw)
    x = ref.rounded(kc.draw_x(case, dtype, op.shape[0], 33, np.random.default_rng(9)))
    y, y0 = _device_apply(op, x, dtype), _device_apply(plain, x, dtype)
    print("worst / bound: on", ref.check(y, x, transpose=True), "off", ref.check(y0, x, transpose=True))
    lim = 2 * (np.longdouble(ref.gamma(True)) * ref.apply_abs(x, True) + np.longdouble(ref.tiny(True)))
    assert (np.abs(y.astype(np.clongdouble) - y0.astype(np.clongdouble)) <= lim).all()
    op.close(); plain.close()
