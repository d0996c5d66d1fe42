"""Which kernels the apply path runs, without a GPU (BFHIP_FLAG_PLAN_ONLY + bfhipPlanStageKernels).

* The kernel catalogue (tests/kernel_catalogue.py) reaches every BfhipKernelId but the named few the dispatch cannot emit,
  and each case reaches the ids it declares.
* The plan emulator's result for every catalogue case, element type and direction meets the componentwise bound of the
  extended-precision reference (tests/highprec.py): the reference and its bounds are checked here before a GPU runs them."""
import numpy as np
import pytest

from butterfly_amd import _capi
from butterfly_amd.operator import HipOperator
import kernel_catalogue as kc
from highprec import Reference
from plan_emulator import run_plan

PLAN = _capi.FLAG_PLAN_ONLY


def _reached(case, dtype):
    desc, vals, demote = kc.materialize(case, dtype)
    seen = set()
    for flags in kc.flag_sets(case, dtype):
        op = HipOperator.from_desc(desc, vals, flags=PLAN | flags, demote_to_f32=demote)
        assert op.stats()["dtype"] == dtype
        for nrhs in case.nrhs:
            for ids in op.stage_kernels(nrhs):
                seen.update(ids)
        op.close()
    return seen


def test_kernel_ids_have_names():
    names = [_capi.kernel_name(i) for i in range(_capi.KERNEL_COUNT)]
    assert all(names) and len(set(names)) == _capi.KERNEL_COUNT
    ext = [_capi.kernel_name(i) for i in range(_capi.KERNEL_EXT_BASE, _capi.KERNEL_EXT_END)]
    assert all(ext) and len(set(names + ext)) == len(names) + len(ext)
    assert ext[_capi.KERNEL_C64_MFMA2 - _capi.KERNEL_EXT_BASE] == "bfStageKernelC64Mfma<2 tiles>"
    for i in (*range(_capi.KERNEL_COUNT, _capi.KERNEL_EXT_BASE), _capi.KERNEL_EXT_END):      # neither range: no name
        assert _capi.kernel_name(i) is None
    assert names[kc.k_t(kc.C64, True, True, True)] == "bfStageKernelT<C64, wide, coop, nrhs=1>"
    assert names[kc.k_reduce(kc.F32, True)] == "bfReduceKernel<F32, long>"
    assert names[kc.k_tboth(kc.F64, False)] == "bfStageKernelTBoth<F64, nrhs>1>"


def test_catalogue_reaches_every_kernel():
    seen = set()
    for case in kc.CASES:
        for dt in kc.DTYPES:
            seen |= _reached(case, dt)
    assert not seen & set(kc.UNREACHABLE), "an id named unreachable is reached: take it off the list"
    missing = sorted(set(range(_capi.KERNEL_COUNT)) - set(kc.UNREACHABLE) - seen)
    assert not missing, "kernels no catalogue case reaches: " + ", ".join(_capi.kernel_name(i) for i in missing)
    assert seen <= set(range(_capi.KERNEL_COUNT))


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_case_reaches_what_it_declares(name):
    case = kc.BY_NAME[name]
    for dt, ids in case.reaches.items():
        missing = sorted(set(ids) - _reached(case, dt))
        assert not missing, f"{name} / {kc.DTYPE_NAMES[dt]} no longer reaches " + ", ".join(_capi.kernel_name(i) for i in missing)


def test_stage_kernels_follow_nrhs_and_flags():
    """the complex128 forward choice at every tile edge: GEMV at 1, matrix cores of 1 / 2 / 4 tiles up to 16 / 32 / more"""
    desc, vals, _ = kc.materialize(kc.BY_NAME["mfma_tiles"], kc.C128)
    for exact in (0, _capi.FLAG_EXACT_COMPLEX):
        op = HipOperator.from_desc(desc, vals, flags=PLAN | exact)
        base = kc.K_MFMA1_EXACT if exact else kc.K_MFMA1
        for nrhs in kc.NRHS_ALL:
            want = kc.K_C128 if nrhs == 1 else base + (0 if nrhs <= 16 else 1 if nrhs <= 32 else 2)
            for ids in op.stage_kernels(nrhs):
                assert ids[0] == want and all(i == kc.k_reduce(kc.C128) for i in ids[1:]), (nrhs, exact, ids)
        op.close()


def _emulator_cases():
    for case in kc.CASES:
        for dt in kc.DTYPES:
            yield f"{case.name}-{kc.DTYPE_NAMES[dt]}", case.name, dt


_EMU = list(_emulator_cases())


@pytest.mark.parametrize("name,dtype", [(c[1], c[2]) for c in _EMU], ids=[c[0] for c in _EMU])
def test_emulator_meets_the_highprec_bound(name, dtype):
    case = kc.BY_NAME[name]
    desc, vals, demote = kc.materialize(case, dtype)
    ref = Reference(desc, vals, dtype)
    rng = np.random.default_rng(case.seed)
    for flags in kc.flag_sets(case, dtype):
        op = HipOperator.from_desc(desc, vals, flags=PLAN | flags, demote_to_f32=demote)
        m, n = op.shape
        nrhs = max(case.nrhs[:2])
        for t in (False, True):
            x = ref.rounded(kc.draw_x(case, dtype, m if t else n, nrhs, rng))
            y = run_plan(op, x, transpose=t)
            assert y.dtype == kc.STORAGE_NP[dtype]
            ref.check(y, x, transpose=t)
        op.close()


def test_highprec_bound_is_tight_enough_to_fail_float_accumulation():
    """The C64 bound must reject float accumulation over a long contraction (the absorb case: 33791 terms below half an ulp
    of the first are dropped) and accept the same sum in double rounded once."""
    case = kc.BY_NAME["absorb_reduce_33"]
    desc, vals, _ = kc.materialize(case, kc.C64)
    ref = Reference(desc, vals, kc.C64)
    x = ref.rounded(kc.draw_x(case, kc.C64, desc.cols[desc.root], 1, np.random.default_rng(0))[:, 0])
    a = np.asarray(vals[desc.root]).astype(np.complex64)
    y = np.zeros(a.shape[0], dtype=np.complex64)
    for j0 in range(0, a.shape[1], 1024):     # sequential float accumulation
        for j in range(j0, j0 + 1024):
            y += a[:, j] * x[j]
    with pytest.raises(AssertionError, match="componentwise bound violated"):
        ref.check(y, x)
    # and the same sum in double, rounded once, passes
    ref.check((a.astype(np.complex128) @ x.astype(np.complex128)).astype(np.complex64), x)
