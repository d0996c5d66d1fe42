"""The block kernels of the real element types (bfhipSetRealRhsBlocks, bfStageKernelRealMfma*) on the GPU.

* every catalogue case as an F64 and an F32 operand with the switch on, forward, at nrhs across every tile edge: the
  componentwise bound of tests/highprec.py (unchanged), the device entry into a NaN-filled dY, determinism, NaN taint;
* nrhs below minRhs, the switch off again, and the transposed apply: bit-identical to an operator whose switch was never touched;
* F32 cases whose forward plan has no reduce (listed by tests/test_real_rhs_blocks_cpu.py) also meet the tight bound of item
  sums formed in double and rounded once per stored level;
* the callers: extract equals the apply on unit panels bit for bit, a loaded operator takes the switch, and a captured apply
  replays to the same bits."""
import functools

import numpy as np
import pytest

import kernel_catalogue as kc
from test_real_rhs_blocks_cpu import check_tight, reduce_free_cases

pytestmark = pytest.mark.gpu

NRHS = (2, 3, 16, 17, 20, 33, 64, 70, 80)
REAL = (kc.F64, kc.F32)
_PAIRS = [(c.name, dt) for c in kc.CASES for dt in REAL]
_IDS = [f"{n}-{kc.DTYPE_NAMES[d]}" for n, d in _PAIRS]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _torch_dtype(dtype):
    import torch
    return {kc.F64: torch.float64, kc.F32: torch.float32}[dtype]


def _device_apply(op, x, dtype, t=False):
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
    return frozenset(reduce_free_cases())


@pytest.mark.parametrize("name,dtype", _PAIRS, ids=_IDS)
def test_catalogue_on_the_block_kernels(name, dtype):
    from butterfly_amd.operator import HipOperator
    from highprec import Reference
    case = kc.BY_NAME[name]
    st = kc.STORAGE_NP[dtype]
    desc, vals, demote = kc.materialize(case, dtype)
    ref = Reference(desc, vals, dtype)
    tight = dtype == kc.F32 and name in _reduce_free()
    rng = np.random.default_rng(case.seed + 11)
    for flags in kc.flag_sets(case, dtype):
        op = HipOperator.from_desc(desc, vals, flags=flags, max_rhs=max(NRHS), demote_to_f32=demote, device=0, real_rhs_blocks=2)
        plain = HipOperator.from_desc(desc, vals, flags=flags, max_rhs=max(NRHS), demote_to_f32=demote, device=0)
        assert op.stats()["dtype"] == dtype
        m, n = op.shape
        first = {}
        for nrhs in NRHS:
            where = f"flags {flags:#x} nrhs {nrhs}"
            x = ref.rounded(kc.draw_x(case, dtype, n, nrhs, rng))
            host = op.apply_host(x)
            try:
                worst = ref.check(host, x, transpose=False)
                if tight:
                    print(f"{where}: worst / bound {worst:.3g}, worst / tight bound {check_tight(ref, host, x):.3g}")
            except AssertionError as e:
                raise AssertionError(f"{where}: {e}") from None
            y1 = _device_apply(op, x, dtype)
            assert np.isfinite(y1).all(), f"{where}: {int((~np.isfinite(y1)).sum())} outputs never written"
            assert np.array_equal(_bits(y1), _bits(host.astype(st))), f"{where}: device entry != host entry"
            y2 = _device_apply(op, x, dtype)
            assert np.array_equal(_bits(y1), _bits(y2)), f"{where}: two applies differ"
            first[nrhs] = (x, y1)
            # NaN taint: one input entry of the last right-hand side
            j = int(rng.integers(n))
            xn = x.copy()
            xn[j, nrhs - 1] = np.nan
            bad = ~np.isfinite(_device_apply(op, xn, dtype))
            want = np.zeros_like(bad)
            want[:, nrhs - 1] = ref.structural(j, transpose=False)
            assert np.array_equal(bad, want), (f"{where}: NaN at input {j} reached {int((bad & ~want).sum())} outputs it does not feed "
                                               f"and missed {int((want & ~bad).sum())}")
            assert np.array_equal(_bits(_device_apply(op, x, dtype)), _bits(y1)), f"{where}: state carried over from the NaN apply"
        # below minRhs, with the switch off again, and transposed: the bits of an operator whose switch was never touched
        x1 = ref.rounded(kc.draw_x(case, dtype, n, 1, rng))
        assert np.array_equal(_bits(_device_apply(op, x1, dtype)), _bits(_device_apply(plain, x1, dtype))), f"flags {flags:#x}: nrhs 1 changed"
        for nrhs in (2, 17, 80):
            xt = ref.rounded(kc.draw_x(case, dtype, m, nrhs, rng))
            assert np.array_equal(_bits(_device_apply(op, xt, dtype, True)), _bits(_device_apply(plain, xt, dtype, True))), f"flags {flags:#x}: transposed nrhs {nrhs} changed"
        op.set_real_rhs_blocks(17)
        x16 = first[16][0]
        assert np.array_equal(_bits(_device_apply(op, x16, dtype)), _bits(_device_apply(plain, x16, dtype))), f"flags {flags:#x}: nrhs 16 < minRhs 17 changed"
        assert np.array_equal(_bits(_device_apply(op, first[17][0], dtype)), _bits(first[17][1]))
        op.set_real_rhs_blocks(0)
        for nrhs in NRHS:
            x = first[nrhs][0]
            assert np.array_equal(_bits(_device_apply(op, x, dtype)), _bits(_device_apply(plain, x, dtype))), f"flags {flags:#x}: switch off, nrhs {nrhs} changed"
        op.close(); plain.close()


def test_the_tight_bound_covers_the_expected_cases():
    free = _reduce_free()
    assert len(free) >= 16 and "absorb_chain_70" in free and "forward_both" in free, sorted(free)


@pytest.mark.parametrize("dtype", REAL, ids=[kc.DTYPE_NAMES[d] for d in REAL])
def test_extract_equals_the_apply_on_unit_panels(dtype):
    from butterfly_amd.operator import HipOperator
    from highprec import Reference
    case = kc.BY_NAME["randgraph5"]
    st = kc.STORAGE_NP[dtype]
    desc, vals, demote = kc.materialize(case, dtype)
    ref = Reference(desc, vals, dtype)
    op = HipOperator.from_desc(desc, vals, demote_to_f32=demote, max_rhs=64, device=0, real_rhs_blocks=2)
    plain = HipOperator.from_desc(desc, vals, demote_to_f32=demote, max_rhs=64, device=0)
    m, n = op.shape
    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, m, size=min(m, 90)), rng.integers(0, n, size=150)
    blk = op.extract(rows, cols).cpu().numpy()
    assert blk.shape == (len(rows), 150) and blk.dtype == st
    differs = False
    for c0 in range(0, 150, 64):
        idx = cols[c0:c0 + 64]
        x = np.zeros((n, len(idx)), dtype=st)
        x[idx, np.arange(len(idx))] = 1.0
        y = _device_apply(op, x, dtype)
        assert np.array_equal(_bits(blk[:, c0:c0 + 64]), _bits(y[rows])), c0
        differs = differs or not np.array_equal(_bits(y), _bits(_device_apply(plain, x, dtype)))
    # the default path's extract: both meet the componentwise bound against the exact entries, so they differ by at most twice it
    e = np.zeros((n, 150))
    e[cols, np.arange(150)] = 1.0
    lim = 2 * (np.longdouble(ref.gamma()) * ref.apply_abs(e)[rows] + np.longdouble(ref.tiny()))
    off = plain.extract(rows, cols).cpu().numpy()
    assert (np.abs(blk.astype(np.longdouble) - off.astype(np.longdouble)) <= lim).all()
    print("block path differs from the default path in some bit:", differs)
    op.close(); plain.close()


@pytest.mark.parametrize("dtype", REAL, ids=[kc.DTYPE_NAMES[d] for d in REAL])
def test_a_loaded_operator_takes_the_switch(dtype, tmp_path):
    from butterfly_amd.operator import HipOperator
    case = kc.BY_NAME["randgraph1"]
    desc, vals, demote = kc.materialize(case, dtype)
    op = HipOperator.from_desc(desc, vals, max_rhs=20, demote_to_f32=demote, device=0, real_rhs_blocks=2)
    plain = HipOperator.from_desc(desc, vals, max_rhs=20, demote_to_f32=demote, device=0)
    op.save(tmp_path / "real.bfhip")
    plain.save(tmp_path / "plain.bfhip")
    assert (tmp_path / "real.bfhip").read_bytes() == (tmp_path / "plain.bfhip").read_bytes()      # the file does not hold the switch
    back = HipOperator.load(tmp_path / "real.bfhip", max_rhs=20, device=0, real_rhs_blocks=2)
    off = HipOperator.load(tmp_path / "real.bfhip", max_rhs=20, device=0)
    x = np.random.default_rng(3).standard_normal((op.shape[1], 20)).astype(kc.STORAGE_NP[dtype])
    y = _device_apply(op, x, dtype)
    assert np.array_equal(_bits(_device_apply(back, x, dtype)), _bits(y))
    assert np.array_equal(_bits(_device_apply(off, x, dtype)), _bits(_device_apply(plain, x, dtype)))
    op.set_real_rhs_blocks(0)
    assert np.array_equal(_bits(_device_apply(off, x, dtype)), _bits(_device_apply(op, x, dtype)))
    for o in (op, plain, back, off):
        o.close()


@pytest.mark.parametrize("dtype", REAL, ids=[kc.DTYPE_NAMES[d] for d in REAL])
def test_block_apply_can_be_captured_in_a_hip_graph(dtype):
    import torch
    from butterfly_amd.operator import HipOperator
    case = kc.BY_NAME["randgraph5"]
    desc, vals, demote = kc.materialize(case, dtype)
    op = HipOperator.from_desc(desc, vals, max_rhs=20, demote_to_f32=demote, device=0, real_rhs_blocks=2)
    n = op.shape[1]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.randn((n, 20), dtype=_torch_dtype(dtype), device="cuda")
        y = torch.empty((op.shape[0], 20), dtype=_torch_dtype(dtype), device="cuda")
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
