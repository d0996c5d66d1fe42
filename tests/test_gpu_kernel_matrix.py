"""Every stage and reduce kernel of the apply path on the GPU, against the extended-precision reference.

For each catalogue case (tests/kernel_catalogue.py: together they reach every BfhipKernelId the dispatch can emit) and
element type, under each adjoint mode (and FLAG_EXACT_COMPLEX where the case asks), forward and transposed, at each of the
case's nrhs:
* reference bound: the host entry meets the componentwise bound of tests/highprec.py;
* device entry: with dY prefilled with NaN every output is finite (no row left unwritten) and bit-identical to the host
  entry's result;
* determinism: a second device apply is bit-identical;
* NaN taint: a NaN in one entry of x makes exactly the outputs that depend on it structurally non-finite (leaves have no
  exact zeros), in its own right-hand side only; a clean apply after it is bit-identical to the operator's first result
  (no temp or vector-arena state carries over)."""
import numpy as np
import pytest

import kernel_catalogue as kc

pytestmark = pytest.mark.gpu

_PAIRS = [(c.name, dt) for c in kc.CASES for dt in kc.DTYPES]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _torch_dtype(dtype):
    import torch
    return {kc.C128: torch.complex128, kc.F64: torch.float64, kc.F32: torch.float32, kc.C64: torch.complex64}[dtype]


def _device_apply(op, x, t, dtype):
    """op applied to host array x (storage dtype) through the device entry, into a NaN-filled dY."""
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


@pytest.mark.parametrize("name,dtype", _PAIRS, ids=[f"{n}-{kc.DTYPE_NAMES[d]}" for n, d in _PAIRS])
def test_kernel_matrix(name, dtype):
    from butterfly_amd.operator import HipOperator
    from highprec import Reference
    case = kc.BY_NAME[name]
    desc, vals, demote = kc.materialize(case, dtype)
    ref = Reference(desc, vals, dtype)
    rng = np.random.default_rng(case.seed + 7)
    for flags in kc.flag_sets(case, dtype):
        op = HipOperator.from_desc(desc, vals, flags=flags, max_rhs=max(case.nrhs), demote_to_f32=demote, device=0)
        assert op.stats()["dtype"] == dtype
        m, n = op.shape
        for t in (False, True):
            first = {}
            for nrhs in case.nrhs:
                where = f"flags {flags:#x} transposed {t} nrhs {nrhs}"
                x = ref.rounded(kc.draw_x(case, dtype, m if t else n, nrhs, rng))
                host = op.apply_transpose_host(x) if t else op.apply_host(x)
                try:
                    ref.check(host, x, transpose=t)
                except AssertionError as e:
                    raise AssertionError(f"{where}: {e}") from None
                y1 = _device_apply(op, x, t, dtype)
                assert np.isfinite(y1).all(), f"{where}: {int((~np.isfinite(y1)).sum())} outputs never written"
                assert np.array_equal(_bits(y1), _bits(host.astype(kc.STORAGE_NP[dtype]))), f"{where}: device entry != host entry"
                y2 = _device_apply(op, x, t, dtype)
                assert np.array_equal(_bits(y1), _bits(y2)), f"{where}: two applies differ"
                first.setdefault(nrhs, (x, y1))
            # NaN taint on the case's first nrhs: one input entry of the last right-hand side
            nrhs = case.nrhs[0]
            x, y_clean = first[nrhs]
            j = int(rng.integers(x.shape[0]))
            xn = x.copy()
            xn[j, nrhs - 1] = np.nan
            yn = _device_apply(op, xn, t, dtype)
            bad = ~np.isfinite(yn)
            want = np.zeros_like(bad)
            want[:, nrhs - 1] = ref.structural(j, transpose=t)
            assert np.array_equal(bad, want), (f"flags {flags:#x} transposed {t}: NaN at input {j} reached "
                                               f"{int((bad & ~want).sum())} outputs it does not feed and missed {int((want & ~bad).sum())}")
            y_again = _device_apply(op, x, t, dtype)
            assert np.array_equal(_bits(y_again), _bits(y_clean)), f"flags {flags:#x} transposed {t}: state carried over from the NaN apply"
        op.close()
