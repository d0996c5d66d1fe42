"""Host-side mirror of the engine's C-ABI (include/bfhip.h) for Python callers.

`HipOperator` owns a `BfhipOperator*`.  It is created either from a reference
`BfMat*` (the drop-in path: `bfhipCompile`) or from a flat structure
descriptor (`bfhipCompileDesc`, used for structure-exact synthetic operands
whose values are generated directly in HBM).  `apply` mirrors `bfMatMul`
(reference src/mat.c:183): Y = A X with X an N x nrhs row-major array.

torch is used for device memory and streams only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import BFHIP_C64, BFHIP_C128, BFHIP_F32, BFHIP_F64, BfhipOptions, BfhipStats, DescArrays, check


def _options(device=-1, flags=0, max_rhs=1, demote_to_f32=False, seed=0, row_blocks=None, row_range=None):
    o = BfhipOptions()
    o.structSize = C.sizeof(BfhipOptions)
    o.device = device
    o.flags = flags
    o.maxRhs = max_rhs
    o.demoteToF32 = 1 if demote_to_f32 else 0
    o.seed = seed
    if row_blocks is not None:
        o.rowBlockBegin, o.rowBlockEnd = row_blocks
    if row_range is not None:
        o.rowBegin, o.rowEnd = row_range
    return o


RHS_BLOCKS_DEFAULT = 2      # what rhs_blocks=True stands for: the block kernels read the operand once where the default path reads it nrhs times
REAL_RHS_BLOCKS_DEFAULT = 2 # what real_rhs_blocks=True stands for (F64 / F32 operators)
ADJOINT_RHS_BLOCKS_DEFAULT = 2   # what adjoint_rhs_blocks=True stands for (any element type)


class HipOperator:
    def __init__(self, handle, keep=()):
        self._h = C.c_void_p(handle)
        self._keep = list(keep)
        self._lib = _capi.load()

    def _with_rhs_blocks(self, rhs_blocks, real_rhs_blocks=None, adjoint_rhs_blocks=None):
        """The constructors' `rhs_blocks=` (complex64), `real_rhs_blocks=` (F64 / F32) and `adjoint_rhs_blocks=` (the adjoint plan
        of any element type) keywords: None / False / 0 leaves the switch off, True = RHS_BLOCKS_DEFAULT / REAL_RHS_BLOCKS_DEFAULT /
        ADJOINT_RHS_BLOCKS_DEFAULT, else min_rhs."""
        try:
            if rhs_blocks:
                self.set_rhs_blocks(RHS_BLOCKS_DEFAULT if rhs_blocks is True else rhs_blocks)
            if real_rhs_blocks:
                self.set_real_rhs_blocks(REAL_RHS_BLOCKS_DEFAULT if real_rhs_blocks is True else real_rhs_blocks)
            if adjoint_rhs_blocks:
                self.set_adjoint_rhs_blocks(ADJOINT_RHS_BLOCKS_DEFAULT if adjoint_rhs_blocks is True else adjoint_rhs_blocks)
        except Exception:
            self.close()
            raise
        return self

    def set_rhs_blocks(self, min_rhs):
        """bfhipSetRhsBlocks (complex64 operators): forward stages of applies with nrhs >= min_rhs run the block kernels
        (bfStageKernelC64Mfma*); 0 = off (the default), otherwise min_rhs >= 2."""
        check(self._lib.bfhipSetRhsBlocks(self._h, int(min_rhs)))

    def set_real_rhs_blocks(self, min_rhs):
        """bfhipSetRealRhsBlocks (F64 / F32 operators): forward stages of applies with nrhs >= min_rhs run the block kernels
        (bfStageKernelRealMfma*); 0 = off (the default), otherwise min_rhs >= 2."""
        check(self._lib.bfhipSetRealRhsBlocks(self._h, int(min_rhs)))

    def set_adjoint_rhs_blocks(self, min_rhs):
        """bfhipSetAdjointRhsBlocks (any element type; the operator needs an adjoint plan): the adjoint plan's stages of applies
        with nrhs >= min_rhs run block kernels (shared leaves: bfStageKernelTMfma; packed: the forward block kernels); 0 = off
        (the default), otherwise min_rhs >= 2."""
        check(self._lib.bfhipSetAdjointRhsBlocks(self._h, int(min_rhs)))

    # ---- construction ------------------------------------------------------
    @classmethod
    def from_bfmat(cls, bfmat_ptr, rhs_blocks=None, real_rhs_blocks=None, adjoint_rhs_blocks=None, **opts):
        """Compile a reference BfMat object graph (bfhipCompile)."""
        lib = _capi.load()
        h = C.c_void_p()
        o = _options(**opts)
        check(lib.bfhipCompile(C.c_void_p(bfmat_ptr), C.byref(o), C.byref(h)))
        return cls(h.value)._with_rhs_blocks(rhs_blocks, real_rhs_blocks, adjoint_rhs_blocks)

    @classmethod
    def from_desc(cls, desc, leaf_values=None, root=None, rhs_blocks=None, real_rhs_blocks=None, adjoint_rhs_blocks=None, **opts):
        """Compile a flat descriptor (bfhipCompileDesc); leaves without values are
        synthesized on the device from `seed`."""
        lib = _capi.load()
        da = DescArrays(desc, root=root, leaf_values=leaf_values)
        h = C.c_void_p()
        o = _options(**opts)
        check(lib.bfhipCompileDesc(da.byref(), C.byref(o), C.byref(h)))
        keep = [da] if (o.flags & _capi.FLAG_PLAN_ONLY) else []
        return cls(h.value, keep=keep)._with_rhs_blocks(rhs_blocks, real_rhs_blocks, adjoint_rhs_blocks)

    @classmethod
    def build_helm2(cls, desc, points, wavenumber, root=None, workspace_bytes=0, layer_pot="S", normals=None,
                    col_weights=None, self_value=0.0, kr_order=0, orig_index=None, alpha=0.0, beta=0.0, tgt_points=None,
                    tgt_normals=None, rhs_blocks=None, real_rhs_blocks=None, adjoint_rhs_blocks=None, out_dtype=None, **opts):
        """bfhipBuildHelm2: lay out `desc` (helm2_structure with recipes=True) and
        compute every leaf on the device from its recipe.  `points` (and
        `normals` for layer_pot="Sp"): [N, 2] in quadtree order.  The operator
        built is  self_value * I + (K o KR) diag(col_weights), KR = Kapur-Rokhlin
        factors of order `kr_order` (needs orig_index = the quadtree permutation).
        out_dtype: None / BFHIP_C128, or BFHIP_C64 for a complex64 operator (the double-precision
        values rounded once; `demote_to_f32` stays refused here).
        Returns (operator, build statistics)."""
        lib = _capi.load()
        da = DescArrays(desc, root=root)
        recipes = getattr(desc, "recipe_array", None)
        prob = _capi.Helm2Problem(points, wavenumber, recipes if recipes is not None else desc.recipe, workspace_bytes, layer_pot, normals,
                                  col_weights, self_value,
                                  kr_order, orig_index, alpha, beta, tgt_points, tgt_normals, out_dtype)
        st = _capi.BfhipBuildStats()
        st.structSize = C.sizeof(st)
        h = C.c_void_p()
        o = _options(**opts)
        check(lib.bfhipBuildHelm2(da.byref(), prob.byref(), C.byref(o), C.byref(h), C.byref(st)))
        return cls(h.value)._with_rhs_blocks(rhs_blocks, real_rhs_blocks, adjoint_rhs_blocks), st.as_dict()

    @classmethod
    def build_helm2_pair(cls, desc, points, wavenumber, root=None, workspace_bytes=0, layer_pot="S", normals=None,
                         col_weights=None, self_value=0.0, kr_order=0, orig_index=None, alpha=0.0, beta=0.0, tgt_points=None,
                         tgt_normals=None, low_opts=None, **opts):
        """bfhipBuildHelm2Pair: one value build, two operators -- the complex128 operator build_helm2(**opts) makes and
        the complex64 one build_helm2(out_dtype=BFHIP_C64, **low_opts) makes (low_opts: a dict of compile options, None =
        opts), e.g. the operand and the inner operator of solve_gmres_refine_device.  Returns (op, low, build statistics)."""
        lib = _capi.load()
        da = DescArrays(desc, root=root)
        recipes = getattr(desc, "recipe_array", None)
        prob = _capi.Helm2Problem(points, wavenumber, recipes if recipes is not None else desc.recipe, workspace_bytes, layer_pot, normals,
                                  col_weights, self_value, kr_order, orig_index, alpha, beta, tgt_points, tgt_normals)
        st = _capi.BfhipBuildStats()
        st.structSize = C.sizeof(st)
        h, hl = C.c_void_p(), C.c_void_p()
        o = _options(**opts)
        ol = None if low_opts is None else _options(**low_opts)
        check(lib.bfhipBuildHelm2Pair(da.byref(), prob.byref(), C.byref(o), None if ol is None else C.byref(ol), C.byref(h), C.byref(hl),
                                      C.byref(st)))
        return cls(h.value), cls(hl.value), st.as_dict()

    @classmethod
    def fac_helm2_make_multilevel(cls, points, wavenumber, normals=None, col_weights=None, layer_pot="S", self_value=0.0,
                                  kr_order=0, alpha=0.0, beta=0.0, workspace_bytes=0, tgt_points=None, tgt_normals=None, rhs_blocks=None, real_rhs_blocks=None, adjoint_rhs_blocks=None,
                                  out_dtype=None, **opts):
        """bfhipFacHelm2MakeMultilevel[2]: points (original order) -> device operator in one native
        call (C layout + device build).  Returns (operator, perm, build statistics), or with
        `tgt_points` (operator, (perm, tgt_perm), statistics); the operator maps x[perm] to
        y[tgt_perm] (quadtree orders).  out_dtype as build_helm2."""
        lib = _capi.load()
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        ptr = lambda a: None if a is None else a.ctypes.data
        pts, nrm, w, tpts, tnrm = f64(points), f64(normals), f64(col_weights), f64(tgt_points), f64(tgt_normals)
        params = _capi.Helm2Problem(pts, wavenumber, None, workspace_bytes, layer_pot, None, None, self_value, kr_order, None, alpha, beta,
                                    out_dtype=out_dtype)
        st = _capi.BfhipBuildStats()
        st.structSize = C.sizeof(st)
        perm = np.empty(len(pts), dtype=np.uint64)
        tperm = np.empty(0 if tpts is None else len(tpts), dtype=np.uint64)
        h = C.c_void_p()
        o = _options(**opts)
        check(lib.bfhipFacHelm2MakeMultilevel2(ptr(pts), ptr(nrm), ptr(w), len(pts), ptr(tpts), ptr(tnrm), len(tperm), params.byref(), C.byref(o),
                                               C.byref(h), perm.ctypes.data, tperm.ctypes.data if len(tperm) else None, C.byref(st)))
        perm = perm.astype(np.int64)
        return cls(h.value)._with_rhs_blocks(rhs_blocks, real_rhs_blocks, adjoint_rhs_blocks), (perm if tpts is None else (perm, tperm.astype(np.int64))), st.as_dict()

    @classmethod
    def load(cls, path, rhs_blocks=None, real_rhs_blocks=None, adjoint_rhs_blocks=None, **opts):
        """bfhipLoad: a previously saved operator, straight into HBM."""
        lib = _capi.load()
        h = C.c_void_p()
        o = _options(**opts)
        check(lib.bfhipLoad(str(path).encode(), C.byref(o), C.byref(h)))
        return cls(h.value)._with_rhs_blocks(rhs_blocks, real_rhs_blocks, adjoint_rhs_blocks)

    def save(self, path):
        """bfhipSave: packed leaf arena + index metadata of the compiled operator."""
        check(self._lib.bfhipSave(self._h, str(path).encode()))

    def close(self):
        if self._h:
            for cond in list(getattr(self, "_conds", ())):      # conditioning objects reference the operator: they go first
                cond.close()
            self._lib.bfhipFree(C.byref(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- introspection -----------------------------------------------------
    @property
    def handle(self):
        return self._h

    @property
    def shape(self):
        return int(self._lib.bfhipGetNumRows(self._h)), int(self._lib.bfhipGetNumCols(self._h))

    def num_bytes(self):
        return int(self._lib.bfhipNumBytes(self._h))

    def stage_kernels(self, nrhs=1):
        """bfhipPlanStageKernels over every stage (forward, then the adjoint plan's): per stage the kernel ids an apply of
        `nrhs` right-hand sides launches, in launch order.  Needs FLAG_PLAN_ONLY (no device is touched)."""
        info = _capi.BfhipPlanInfo()
        info.structSize = C.sizeof(info)
        check(self._lib.bfhipPlanGetInfo(self._h, C.byref(info)))
        out = []
        ids = (C.c_uint32 * 64)()
        for s in range(int(info.numStages) + int(info.numStagesT)):
            cnt = C.c_uint32(0)
            check(self._lib.bfhipPlanStageKernels(self._h, s, nrhs, ids, 64, C.byref(cnt)))
            if cnt.value > 64:
                ids2 = (C.c_uint32 * cnt.value)()
                check(self._lib.bfhipPlanStageKernels(self._h, s, nrhs, ids2, cnt.value, C.byref(cnt)))
                out.append(list(ids2))
            else:
                out.append(list(ids[:cnt.value]))
        return out

    def stats(self):
        st = BfhipStats()
        st.structSize = C.sizeof(BfhipStats)
        check(self._lib.bfhipGetStats(self._h, C.byref(st)))
        return st.as_dict()

    def flow_status(self):
        """(applies of 1 - 2 RHS run as one dependency-driven launch, one of its waits ever gave up) -- bfhipFlowStatus."""
        en, bad = C.c_uint32(0), C.c_uint32(0)
        check(self._lib.bfhipFlowStatus(self._h, C.byref(en), C.byref(bad)))
        return bool(en.value), bool(bad.value)

    @property
    def dtype(self):
        return self.stats()["dtype"]

    def np_dtype(self):
        return {BFHIP_C128: np.complex128, BFHIP_F64: np.float64, BFHIP_F32: np.float32, BFHIP_C64: np.complex64}[self.dtype]

    def _host_dtype(self):
        # the host entries take double precision whatever the operator stores (fp32 / complex64 are demoted on upload)
        return np.complex128 if self.dtype in (BFHIP_C128, BFHIP_C64) else np.float64

    def _torch_dtype(self):
        import torch
        return {BFHIP_C128: torch.complex128, BFHIP_F64: torch.float64, BFHIP_F32: torch.float32, BFHIP_C64: torch.complex64}[self.dtype]

    # ---- apply -------------------------------------------------------------
    def apply_host(self, x: np.ndarray) -> np.ndarray:
        """bfhipApply on host arrays (H2D, all stages, D2H)."""
        m, n = self.shape
        src_dtype = self._host_dtype()
        x2 = np.ascontiguousarray(x, dtype=src_dtype)
        one_d = x2.ndim == 1
        if one_d:
            x2 = x2[:, None]
        if x2.shape[0] != n:
            raise ValueError(f"operator has {n} columns, x has {x2.shape[0]} rows")
        nrhs = x2.shape[1]
        y = np.empty((m, nrhs), dtype=src_dtype)
        check(self._lib.bfhipApply(self._h, x2.ctypes.data, nrhs, nrhs, y.ctypes.data, nrhs))
        return y[:, 0] if one_d else y

    def apply_host_into(self, x: np.ndarray, y: np.ndarray, nrhs=1):
        """bfhipApply on caller-owned, densely packed host arrays (nothing is allocated: what an unmodified caller's loop costs)."""
        check(self._lib.bfhipApply(self._h, x.ctypes.data, nrhs, nrhs, y.ctypes.data, nrhs))
        return y

    def apply_pointers(self, xptr, yptr, nrhs=1):
        """bfhipApply on raw pointers of any kind (device, pinned / registered host, pageable): include/bfhip.h says what each costs."""
        check(self._lib.bfhipApply(self._h, C.c_void_p(xptr), nrhs, nrhs, C.c_void_p(yptr), nrhs))

    @staticmethod
    def host_register(a: np.ndarray):
        check(_capi.load().bfhipHostRegister(C.c_void_p(a.ctypes.data), a.nbytes))

    @staticmethod
    def host_unregister(a: np.ndarray):
        check(_capi.load().bfhipHostUnregister(C.c_void_p(a.ctypes.data)))

    def apply_device(self, x, y=None, stream=None):
        """bfhipApplyDevice on torch tensors resident on the operator's GPU.
        x: [numCols] or [numCols, nrhs], contiguous; returns y (async on the
        current torch stream unless `stream` is given)."""
        import torch
        m, n = self.shape
        tdt = self._torch_dtype()
        if x.dtype != tdt or not x.is_cuda or not x.is_contiguous():
            raise ValueError(f"x must be a contiguous CUDA tensor of dtype {tdt}")
        nrhs = 1 if x.dim() == 1 else x.shape[1]
        if x.shape[0] != n:
            raise ValueError(f"operator has {n} columns, x has {x.shape[0]} rows")
        if y is None:
            y = torch.empty((m,) if x.dim() == 1 else (m, nrhs), dtype=tdt, device=x.device)
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        check(self._lib.bfhipApplyDevice(self._h, C.c_void_p(x.data_ptr()), nrhs, C.c_void_p(y.data_ptr()),
                                         C.c_void_p(s.cuda_stream)))
        return y

    # ---- dense extraction ----------------------------------------------------
    def _extract_args(self, rows, cols, via_adjoint, panel):
        m, n = self.shape
        idx = []
        for sel, ext in ((rows, m), (cols, n)):
            if sel is None:
                idx.append((None, ext, None))
            else:
                a = np.ascontiguousarray(np.asarray(sel).reshape(-1), dtype=np.uint64)
                idx.append((a.ctypes.data_as(C.POINTER(C.c_uint64)), a.size, a))
        o = _capi.BfhipExtractOptions(_capi.BFHIP_EXTRACT_VIA_ADJOINT if via_adjoint else 0, int(panel))
        return idx[0], idx[1], o

    def extract(self, rows=None, cols=None, via_adjoint=False, panel=64, device=True, out=None, stream=None):
        """A[rows, cols] (None = all): bfhipExtractDevice into a torch tensor on the operator's GPU in the compute dtype
        (device=True; async on the current torch stream unless `stream` is given), or bfhipExtract into a double-precision numpy
        array (device=False).  `out` may be given (2-D, its row stride is ldOut)."""
        (rp, nr, ra), (cp, nc, ca), o = self._extract_args(rows, cols, via_adjoint, panel)
        if device:
            import torch
            tdt = self._torch_dtype()
            if out is None:
                ordinal = self._lib.bfhipOperatorDevice(self._h)
                if ordinal < 0:
                    check(self._lib.bfhipExtractDevice(self._h, rp, nr, cp, nc, None, nc, C.byref(o), None))   # the refusal
                out = torch.empty((nr, nc), dtype=tdt, device=torch.device("cuda", ordinal))
            if out.dtype != tdt or not out.is_cuda or out.dim() != 2 or out.stride(1) != 1 or tuple(out.shape) != (nr, nc):
                raise ValueError(f"out must be a CUDA tensor of dtype {tdt}, shape ({nr}, {nc}) and unit column stride")
            s = stream if stream is not None else torch.cuda.current_stream(out.device)
            check(self._lib.bfhipExtractDevice(self._h, rp, nr, cp, nc, C.c_void_p(out.data_ptr()), max(out.stride(0), nc), C.byref(o),
                                               C.c_void_p(s.cuda_stream)))
            return out
        hdt = self._host_dtype()
        if out is None:
            out = np.empty((nr, nc), dtype=hdt)
        if out.dtype != hdt or out.ndim != 2 or out.shape != (nr, nc) or out.strides[1] != out.itemsize:
            raise ValueError(f"out must be a numpy array of dtype {np.dtype(hdt)}, shape ({nr}, {nc}) and unit column stride")
        check(self._lib.bfhipExtract(self._h, rp, nr, cp, nc, C.c_void_p(out.ctypes.data), max(out.strides[0] // out.itemsize, nc), C.byref(o)))
        return out

    def extract_workspace_bytes(self, num_rows, num_cols, via_adjoint=False, panel=64):
        """bfhipExtractWorkspaceBytes: device bytes an extraction of num_rows x num_cols entries may hold beyond the operator."""
        o = _capi.BfhipExtractOptions(_capi.BFHIP_EXTRACT_VIA_ADJOINT if via_adjoint else 0, int(panel))
        b = C.c_uint64()
        check(self._lib.bfhipExtractWorkspaceBytes(self._h, num_rows, num_cols, C.byref(o), C.byref(b)))
        return int(b.value)

    def to_dense(self, device=False):
        """The whole operator as a dense matrix (numpy, double precision; a torch tensor in the compute dtype with device=True)."""
        return self.extract(device=device)

    # ---- block-Jacobi preconditioner ---------------------------------------------
    def block_jacobi_partition(self, max_block=128) -> np.ndarray:
        """bfhipBlockJacobiPartition: the automatic diagonal-block cuts (numBlocks + 1 row offsets from 0 to n).  Works on a
        FLAG_PLAN_ONLY operator."""
        n = self.shape[0]
        cuts = np.zeros(n + 1, dtype=np.uint64)
        nb = C.c_uint64(0)
        check(self._lib.bfhipBlockJacobiPartition(self._h, int(max_block), cuts.ctypes.data_as(C.POINTER(C.c_uint64)), cuts.size, C.byref(nb)))
        return cuts[:nb.value + 1].astype(np.int64)

    def block_jacobi(self, cuts=None, max_block=128, invert=True, dtype=None, **opts):
        """bfhipBlockJacobi: M = blockdiag(B_b^{-1}) over the operator's direct part (blockdiag(B_b) with invert=False), a new
        HipOperator usable as `precond` of the GMRES entries.  `cuts`: None (automatic) or numBlocks + 1 increasing row
        offsets from 0 to n; `dtype`: None (the operator's) or BFHIP_C64 / BFHIP_F32 (the demotion); `opts`: device (of the
        result, -1 = the operator's), max_rhs.  Returns (operator, info); a refusal raises BfhipError with `.info` set."""
        unknown = set(opts) - {"device", "max_rhs"}
        if unknown:
            raise TypeError(f"unknown options {sorted(unknown)}")
        device, max_rhs = opts.get("device", -1), opts.get("max_rhs", 0)
        o = _capi.BfhipBlockJacobiOptions()
        o.structSize = C.sizeof(o)
        o.flags = 0 if invert else _capi.BFHIP_BJ_NO_INVERT
        o.maxBlock = int(max_block)
        o.outDtype = 0 if dtype is None else int(dtype)
        o.device = int(device)
        o.maxRhs = int(max_rhs)
        keep = None
        if cuts is not None:
            keep = np.ascontiguousarray(np.asarray(cuts).reshape(-1), dtype=np.uint64)
            if keep.size < 1:
                raise ValueError("cuts must hold numBlocks + 1 offsets")
            o.cuts = keep.ctypes.data
            o.numBlocks = keep.size - 1
        info = _capi.BfhipBlockJacobiInfo()
        info.structSize = C.sizeof(info)
        h = C.c_void_p()
        rc = self._lib.bfhipBlockJacobi(self._h, C.byref(o), C.byref(h), C.byref(info))
        if rc:
            err = _capi.BfhipError(rc, self._lib.bfhipLastErrorMessage().decode())
            err.info = info.as_dict()
            raise err
        return HipOperator(h.value), info.as_dict()

    def set_host_apply_budget(self, nbytes):
        """bfhipSetHostApplyBudget: device bytes the host-vector applies may use for vectors (0 = automatic)."""
        check(self._lib.bfhipSetHostApplyBudget(self._h, int(nbytes)))

    def apply_transpose_host(self, x: np.ndarray) -> np.ndarray:
        """bfhipApplyTranspose: y = A^T x (plain transpose) on host arrays; the
        operator must have been compiled with FLAG_ADJOINT."""
        m, n = self.shape
        src_dtype = self._host_dtype()
        x2 = np.ascontiguousarray(x, dtype=src_dtype)
        one_d = x2.ndim == 1
        if one_d:
            x2 = x2[:, None]
        if x2.shape[0] != m:
            raise ValueError(f"operator has {m} rows, x has {x2.shape[0]} rows")
        nrhs = x2.shape[1]
        y = np.empty((n, nrhs), dtype=src_dtype)
        check(self._lib.bfhipApplyTranspose(self._h, x2.ctypes.data, nrhs, nrhs, y.ctypes.data, nrhs))
        return y[:, 0] if one_d else y

    def apply_transpose_device(self, x, y=None, stream=None):
        import torch
        m, n = self.shape
        if self.dtype == BFHIP_C64 and x.dtype != torch.complex64:
            raise ValueError(f"a complex64 operator takes complex64 tensors, not {x.dtype}")
        nrhs = 1 if x.dim() == 1 else x.shape[1]
        if y is None:
            y = torch.empty((n,) if x.dim() == 1 else (n, nrhs), dtype=x.dtype, device=x.device)
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        check(self._lib.bfhipApplyTransposeDevice(self._h, C.c_void_p(x.data_ptr()), nrhs, C.c_void_p(y.data_ptr()),
                                                  C.c_void_p(s.cuda_stream)))
        return y

    # ---- GMRES ---------------------------------------------------------------
    def solve_gmres(self, b: np.ndarray, x0=None, tol=1e-12, max_num_iter=100):
        """bfhipSolveGMRES on host arrays; returns (x, num_iter, residual), as the
        reference's bfSolveGMRES(A, B, X0, tol, maxNumIter, &numIter, NULL)."""
        n = self.shape[0]
        b2 = np.ascontiguousarray(b, dtype=np.complex128)
        one_d = b2.ndim == 1
        if one_d:
            b2 = b2[:, None]
        nrhs = b2.shape[1]
        x = np.empty((n, nrhs), dtype=np.complex128)
        x0p = None
        if x0 is not None:
            x02 = np.ascontiguousarray(x0, dtype=np.complex128).reshape(n, nrhs)
            x0p = x02.ctypes.data
        it = C.c_size_t(0)
        res = C.c_double(0)
        check(self._lib.bfhipSolveGMRES(self._h, b2.ctypes.data, nrhs, nrhs, x0p, nrhs, tol, max_num_iter,
                                        C.byref(it), C.byref(res), x.ctypes.data, nrhs))
        return (x[:, 0] if one_d else x), int(it.value), float(res.value)

    def solve_gmres_device(self, b, x0=None, tol=1e-12, max_num_iter=100, precond=None, orth="default"):
        """Device-resident form on torch tensors; returns (x, num_iter, residual).  `precond`: a HipOperator
        applying the action of M^{-1} (the reference's left preconditioner M through bfMatSolve).  `orth`:
        "cgs2" (batched, the default), "mgs" (the reference's order, src/linalg.c:174-184) or "default"
        (cgs2 unless BFHIP_GMRES_MGS=1 is set)."""
        import torch
        nrhs = 1 if b.dim() == 1 else b.shape[1]
        x = torch.empty_like(b)
        it = C.c_size_t(0)
        res = C.c_double(0)
        s = torch.cuda.current_stream(b.device)
        o = _capi.BfhipGmresOptions()
        o.structSize = C.sizeof(o)
        o.orthogonalization = {"default": _capi.GMRES_ORTH_DEFAULT, "cgs2": _capi.GMRES_ORTH_CGS2, "mgs": _capi.GMRES_ORTH_MGS}[orth]
        o.tol, o.maxNumIter = tol, max_num_iter
        o.solveM = precond.handle if precond is not None else None
        check(self._lib.bfhipSolveGMRESOptsDevice(self._h, C.byref(o), C.c_void_p(b.data_ptr()), nrhs,
                                                  C.c_void_p(x0.data_ptr()) if x0 is not None else None,
                                                  C.byref(it), C.byref(res), C.c_void_p(x.data_ptr()), C.c_void_p(s.cuda_stream)))
        return x, int(it.value), float(res.value)

    _ORTH = {"default": _capi.GMRES_ORTH_DEFAULT, "cgs2": _capi.GMRES_ORTH_CGS2, "mgs": _capi.GMRES_ORTH_MGS}

    def _refine_options(self, tol, inner_tol, max_outer, max_inner, precond, orth):
        o = _capi.BfhipGmresRefineOptions()
        o.structSize = C.sizeof(o)
        o.orthogonalization = self._ORTH[orth]
        o.tol, o.innerTol, o.maxOuter, o.maxInner = tol, inner_tol, max_outer, max_inner
        o.solveM = precond.handle if precond is not None else None
        return o

    def solve_gmres_refine_device(self, b, low, x0=None, tol=1e-12, inner_tol=0.0, max_outer=10, max_inner=100, precond=None,
                                  orth="default"):
        """Mixed-precision GMRES refinement (bfhipSolveGMRESRefineDevice): this complex128 operator gives the true residuals,
        `low` (a complex64 HipOperator, e.g. the demote_to_f32 compile of the same operand) the inner correction solves.
        b, x0: complex128 torch tensors on the operator's device ([n] or [n, nrhs]).  `precond`: inner left preconditioner
        (complex64 or complex128 HipOperator).  inner_tol = 0: the library default (1e-6).  Returns
        (x, num_outer, num_inner, residual, history), history = the true residual of x0 and of each step's iterate."""
        import torch
        for name, t in (("b", b), ("x0", x0)):
            if t is not None and t.dtype != torch.complex128:
                raise ValueError(f"refinement takes complex128 tensors ({name} is {t.dtype}); the complex64 work is internal")
        nrhs = 1 if b.dim() == 1 else b.shape[1]
        x = torch.empty_like(b)
        no, ni, res = C.c_size_t(0), C.c_size_t(0), C.c_double(0)
        hist = np.full(max_outer + 1, np.nan)
        s = torch.cuda.current_stream(b.device)
        o = self._refine_options(tol, inner_tol, max_outer, max_inner, precond, orth)
        check(self._lib.bfhipSolveGMRESRefineDevice(self._h, low.handle, C.byref(o), C.c_void_p(b.data_ptr()), nrhs,
                                                    C.c_void_p(x0.data_ptr()) if x0 is not None else None, C.byref(no), C.byref(ni),
                                                    C.byref(res), hist.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(x.data_ptr()),
                                                    C.c_void_p(s.cuda_stream)))
        return x, int(no.value), int(ni.value), float(res.value), hist[:int(no.value) + 1].copy()

    def solve_gmres_refine(self, b: np.ndarray, low, x0=None, tol=1e-12, inner_tol=0.0, max_outer=10, max_inner=100, precond=None,
                           orth="default"):
        """bfhipSolveGMRESRefine on host arrays; same arguments and results as solve_gmres_refine_device."""
        b2 = np.asarray(b)
        if b2.dtype == np.complex64 or (x0 is not None and np.asarray(x0).dtype == np.complex64):
            raise ValueError("refinement takes complex128 arrays; the complex64 work is internal")
        b2 = np.ascontiguousarray(b2, dtype=np.complex128)
        one_d = b2.ndim == 1
        if one_d:
            b2 = b2[:, None]
        n, nrhs = b2.shape
        x = np.empty((n, nrhs), dtype=np.complex128)
        x0p = None
        if x0 is not None:
            x02 = np.ascontiguousarray(x0, dtype=np.complex128).reshape(n, nrhs)
            x0p = x02.ctypes.data
        no, ni, res = C.c_size_t(0), C.c_size_t(0), C.c_double(0)
        hist = np.full(max_outer + 1, np.nan)
        o = self._refine_options(tol, inner_tol, max_outer, max_inner, precond, orth)
        check(self._lib.bfhipSolveGMRESRefine(self._h, low.handle, C.byref(o), b2.ctypes.data, max(nrhs, 1), nrhs, x0p, max(nrhs, 1),
                                              C.byref(no), C.byref(ni), C.byref(res), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                              x.ctypes.data, max(nrhs, 1)))
        return (x[:, 0] if one_d else x), int(no.value), int(ni.value), float(res.value), hist[:int(no.value) + 1].copy()

    def stage_profile(self, reset=False):
        """(ms, launches, bytes) per stage, from hipEvents (needs FLAG_PROFILE)."""
        S = self.stats()["numStages"]
        ms = np.zeros(S, dtype=np.float64)
        launches = np.zeros(S, dtype=np.uint64)
        nbytes = np.zeros(S, dtype=np.uint64)
        check(self._lib.bfhipGetStageProfile(self._h, ms.ctypes.data, launches.ctypes.data, nbytes.ctypes.data,
                                             1 if reset else 0))
        return ms, launches, nbytes

    def cov_sample_device(self, gamma_lam, row_perm, w):
        """z = P A diag(gamma_lam) w on the device (sample_z of examples/covariance/lbo_cov.c:36-45); torch tensors on
        this operator's device, gamma_lam / row_perm (int64, scatter order) may be None."""
        import torch
        z = torch.empty(self.stats()["numRows"], dtype=w.dtype, device=w.device)
        s = torch.cuda.current_stream(w.device)
        check(self._lib.bfhipCovSampleDevice(self._h, C.c_void_p(gamma_lam.data_ptr()) if gamma_lam is not None else None,
                                             C.c_void_p(row_perm.data_ptr()) if row_perm is not None else None,
                                             C.c_void_p(w.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(s.cuda_stream)))
        return z

    def cov_matvec_device(self, gamma_lam, row_perm, rev_row_perm, v):
        """z = P A diag(gamma_lam)^2 A^T P' v on the device (cov_matvec of examples/covariance/lbo_cov.c:48-60)."""
        import torch
        z = torch.empty_like(v)
        s = torch.cuda.current_stream(v.device)
        check(self._lib.bfhipCovMatvecDevice(self._h, C.c_void_p(gamma_lam.data_ptr()) if gamma_lam is not None else None,
                                             C.c_void_p(row_perm.data_ptr()) if row_perm is not None else None,
                                             C.c_void_p(rev_row_perm.data_ptr()) if rev_row_perm is not None else None,
                                             C.c_void_p(v.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(s.cuda_stream)))
        return z

    # ---- batched covariance sampling (bfhip_cov.c): blocks are [rows, nrhs] tensors, row-major ----------------
    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    @staticmethod
    def _cov_device(*tensors):
        # where a call without an input tensor works: with its device arguments, else on the current device
        import torch
        for t in tensors:
            if t is not None:
                return t.device
        return torch.device("cuda", torch.cuda.current_device())

    def cov_sample_block_device(self, gamma_lam, row_perm, W):
        """Z = P A diag(gamma_lam) W for a block W [numCols, nrhs] (bfhipCovSampleBlockDevice): column q is what
        cov_sample_device makes of W[:, q]."""
        import torch
        if W.dim() != 2 or not W.is_contiguous():
            raise ValueError("W must be a contiguous [numCols, nrhs] tensor")
        z = torch.empty((self.shape[0], W.shape[1]), dtype=W.dtype, device=W.device)
        s = torch.cuda.current_stream(W.device)
        check(self._lib.bfhipCovSampleBlockDevice(self._h, self._ptr(gamma_lam), self._ptr(row_perm), self._ptr(W), W.shape[1],
                                                  self._ptr(z), C.c_void_p(s.cuda_stream)))
        return z

    def cov_matvec_block_device(self, gamma_lam, row_perm, rev_row_perm, V):
        """Z = P A diag(gamma_lam)^2 A^T P' V for a block V [numRows, nrhs] (bfhipCovMatvecBlockDevice)."""
        import torch
        if V.dim() != 2 or not V.is_contiguous():
            raise ValueError("V must be a contiguous [numRows, nrhs] tensor")
        z = torch.empty_like(V)
        s = torch.cuda.current_stream(V.device)
        check(self._lib.bfhipCovMatvecBlockDevice(self._h, self._ptr(gamma_lam), self._ptr(row_perm), self._ptr(rev_row_perm),
                                                  self._ptr(V), V.shape[1], self._ptr(z), C.c_void_p(s.cuda_stream)))
        return z

    def cov_draw_device(self, gamma_lam, row_perm, seed, first, nrhs):
        """Z [numRows, nrhs]: samples first .. first + nrhs - 1 of the field, from normals generated on the device
        (bfhipCovDrawDevice): w_s[j] = N(seed, (first + s) * numCols + j), whatever the split into calls."""
        import torch
        dev = self._cov_device(gamma_lam, row_perm)
        z = torch.empty((self.shape[0], int(nrhs)), dtype=self._torch_dtype(), device=dev)
        s = torch.cuda.current_stream(dev)
        check(self._lib.bfhipCovDrawDevice(self._h, self._ptr(gamma_lam), self._ptr(row_perm), int(seed), int(first), int(nrhs),
                                           self._ptr(z), C.c_void_p(s.cuda_stream)))
        return z

    def cov_moments_device(self, gamma_lam, row_perm, seed, first, num, batch=64, sum=None, sumsq=None):
        """Adds the sum and the sum of squares over samples first .. first + num - 1, per point, to the float64 [numRows]
        tensors `sum` / `sumsq` (bfhipCovMomentsDevice; zero them before the first call; None: that moment is not
        formed, one of the two is needed).  The samples are never stored.  Returns (sum, sumsq)."""
        import torch
        for t in (sum, sumsq):
            if t is not None and (t.dtype != torch.float64 or t.numel() != self.shape[0] or not t.is_contiguous()):
                raise ValueError("moments are contiguous float64 [numRows] tensors")
        dev = self._cov_device(sum, sumsq, gamma_lam, row_perm)
        s = torch.cuda.current_stream(dev)
        check(self._lib.bfhipCovMomentsDevice(self._h, self._ptr(gamma_lam), self._ptr(row_perm), int(seed), int(first), int(num),
                                              int(batch), self._ptr(sum), self._ptr(sumsq), C.c_void_p(s.cuda_stream)))
        return sum, sumsq

    def fill_normal(self, tensor, seed, first_idx=0):
        """tensor.flat[i] = N(seed, first_idx + i) (bfhipFillNormalDevice); a contiguous float64 / float32 tensor on the
        device.  Returns it."""
        import torch
        if not tensor.is_contiguous():
            raise ValueError("fill_normal takes a contiguous tensor")
        dt = {torch.float64: BFHIP_F64, torch.float32: BFHIP_F32}.get(tensor.dtype, 0xffffffff)
        s = torch.cuda.current_stream(tensor.device)
        with torch.cuda.device(tensor.device):
            check(self._lib.bfhipFillNormalDevice(self._ptr(tensor), tensor.numel(), int(first_idx), dt, int(seed), C.c_void_p(s.cuda_stream)))
        return tensor

    def cov_condition(self, gamma_lam, row_perm, obs, noise_var=None):
        """A CovCondition: the field z = P A diag(gamma_lam) w conditioned on noisy values at the output indices `obs`
        (bfhipCovCondCreate: observed rows by adjoint panels, Gram matrix, Cholesky factor, all on the device).  gamma_lam /
        row_perm are device tensors (or None) that the object references: keep them unchanged while it lives.  obs: distinct
        indices < numRows (host); noise_var: their noise variances (host, >= 0; None: zeros)."""
        return CovCondition(self, gamma_lam, row_perm, obs, noise_var)

    def set_profile_sampling(self, every):
        """Bracket one apply in `every` with events (bfhipSetProfileSampling)."""
        check(self._lib.bfhipSetProfileSampling(self._h, int(every)))

    # ---- reference-vtable shim ---------------------------------------------
    def as_bfmat(self, owns=False):
        """A BfMat* whose Mul / MulVec / RmulVec run on the device (bfhipMatNew).  With
        owns=False the shim does not own the operator (keep this object alive while it is
        used); with owns=True the operator is handed over to the shim -- its Delete slot frees
        it -- and this object is left closed."""
        p = self._lib.bfhipMatNew(self._h, 1 if owns else 0)
        if not p:
            raise _capi.BfhipError(1, self._lib.bfhipLastErrorMessage().decode())
        if owns:
            self._h = C.c_void_p(None)
        return p


def helm2_build_leaf(points, wavenumber, recipe, device=-1, **problem) -> np.ndarray:
    """One leaf of a Helmholtz butterfly computed on the device (bfhipHelm2BuildLeaf);
    `recipe` as in helm2_structure ("kernel", src, tgt) / ("reexp", src, equiv, tgt);
    `problem`: layer_pot, normals, col_weights, self_value."""
    prob = _capi.Helm2Problem(points, wavenumber, {0: recipe}, **problem)
    r = prob.recipes[0]
    rows = int(r["tgt"]["count"] if r["kind"] == _capi.LEAF_KERNEL else r["equiv"]["count"])
    out = np.empty((rows, int(r["src"]["count"])), dtype=np.complex128)
    check(_capi.load().bfhipHelm2BuildLeaf(prob.byref(), 0, device, out.ctypes.data))
    return out


def helm2_dense_apply(points, wavenumber, x, device=-1, **problem):
    """y = (self_value I + K diag(col_weights)) x with the dense layer-potential
    matrix K evaluated on the fly on the device (bfhipHelm2DenseApply[Device]);
    x: numpy [N] or a CUDA tensor; `problem`: layer_pot, normals, col_weights, self_value."""
    prob = _capi.Helm2Problem(points, wavenumber, None, **problem)
    lib = _capi.load()
    m = len(prob.tgt_points) if prob.tgt_points is not None else len(prob.points)
    if isinstance(x, np.ndarray):
        xs = np.ascontiguousarray(x, dtype=np.complex128)
        y = np.empty(m, dtype=np.complex128)
        check(lib.bfhipHelm2DenseApply(prob.byref(), device, xs.ctypes.data, y.ctypes.data))
        return y
    import torch
    y = torch.empty(m, dtype=x.dtype, device=x.device)
    s = torch.cuda.current_stream(x.device)
    check(lib.bfhipHelm2DenseApplyDevice(prob.byref(), x.device.index, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                         C.c_void_p(s.cuda_stream)))
    return y


def _lstsq_options(qr_min=None, gram_min=None, force_global=None):
    o = _capi.BfhipLstSqOptions()
    o.structSize = C.sizeof(_capi.BfhipLstSqOptions)
    o.qrMin = -1 if qr_min is None else int(qr_min)
    o.gramMin = -1 if gram_min is None else int(gram_min)
    o.forceGlobal = -1 if force_global is None else int(bool(force_global))
    return o


def _lstsq_shapes(shapes):
    sh = np.ascontiguousarray(np.asarray(shapes, dtype=np.uint32).reshape(-1, 3))
    if np.any(sh == 0):
        raise ValueError("every dimension of a least-squares problem must be >= 1")
    return sh


def lstsq_routes(shapes, ranks=None, qr_min=None, gram_min=None, force_global=None):
    """The routes bfhipLstSqTruncated takes for problems of the given (mt, me, n) shapes, without a device
    (bfhipLstSqRoutes); `ranks`: what the QR stage is assumed to leave (default: me).  A list of dicts."""
    sh = _lstsq_shapes(shapes)
    rk = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.uint32)
    out = (_capi.BfhipLstSqRoute * max(len(sh), 1))()
    opts = _lstsq_options(qr_min, gram_min, force_global)
    check(_capi.load().bfhipLstSqRoutes(len(sh), sh.ctypes.data, None if rk is None else rk.ctypes.data, C.byref(opts), out))
    return [out[i].as_dict() for i in range(len(sh))]


def lstsq_truncated(problems, device=-1, qr_min=None, gram_min=None, force_global=None):
    """X = pinv_k(A) B for each (A, B) of `problems` on the device, by the builder's own solve (bfhipLstSqTruncated:
    QR with column pivoting, one-sided Jacobi SVD, the reference's truncation rule).  Returns a list of
    (X, sigma, info): sigma the kept singular values, descending; info a dict with rank, qrRank, sweeps,
    notConverged and the route taken."""
    As = [np.asarray(a, dtype=np.complex128) for a, _ in problems]
    Bs = [np.asarray(b, dtype=np.complex128) for _, b in problems]
    if any(a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0] for a, b in zip(As, Bs)):
        raise ValueError("each problem is (A: mt x me, B: mt x n)")
    sh = _lstsq_shapes([(a.shape[0], a.shape[1], b.shape[1]) for a, b in zip(As, Bs)])
    abuf = np.concatenate([a.ravel(order="F") for a in As]) if As else np.zeros(0, np.complex128)
    bbuf = np.concatenate([b.ravel(order="F") for b in Bs]) if Bs else np.zeros(0, np.complex128)
    xbuf = np.empty(int(np.sum(sh[:, 1].astype(np.uint64) * sh[:, 2])), dtype=np.complex128)
    sbuf = np.empty(int(np.sum(sh[:, 1].astype(np.uint64))), dtype=np.float64)
    info = (_capi.BfhipLstSqInfo * max(len(sh), 1))()
    opts = _lstsq_options(qr_min, gram_min, force_global)
    check(_capi.load().bfhipLstSqTruncated(len(sh), sh.ctypes.data, abuf.ctypes.data, bbuf.ctypes.data, xbuf.ctypes.data,
                                           sbuf.ctypes.data, info, C.byref(opts), device))
    out, xo, so = [], 0, 0
    for i, (mt, me, n) in enumerate(sh.tolist()):
        X = xbuf[xo:xo + me * n].reshape((me, n), order="F").copy()
        f = info[i]
        rank = int(f.rank)
        out.append((X, sbuf[so:so + rank].copy(), {"rank": rank, "qrRank": int(f.qrRank), "sweeps": int(f.sweeps),
                                                   "notConverged": int(f.notConverged), "route": f.route.as_dict()}))
        xo += me * n
        so += me
    return out


class CovCondition:
    """Kriging means and posterior samples given observations (bfhipCovCond*, include/bfhip.h "conditioning on
    observations").  y: float64 [numObs] device tensor; blocks are contiguous [rows, nrhs] device tensors."""

    def __init__(self, op, gamma_lam, row_perm, obs, noise_var=None):
        import torch
        import weakref
        self._op, self._lib, self._h = op, op._lib, C.c_void_p()
        self._gamma, self._perm = gamma_lam, row_perm          # referenced by the C object
        obs = np.ascontiguousarray(np.asarray(obs, dtype=np.uint64))
        nv = None if noise_var is None else np.ascontiguousarray(np.asarray(noise_var, dtype=np.float64))
        if obs.ndim != 1 or (nv is not None and nv.shape != obs.shape):
            raise ValueError("obs and noise_var are one-dimensional and of one length")
        for name, t in (("gamma_lam", gamma_lam), ("row_perm", row_perm)):
            if t is not None and t.device.type != "cuda":
                raise ValueError(f"{name} must be a tensor on the operator's GPU (it is on {t.device})")
        self._dev = HipOperator._cov_device(gamma_lam, row_perm)
        s = torch.cuda.current_stream(self._dev)
        check(self._lib.bfhipCovCondCreate(op.handle, HipOperator._ptr(gamma_lam), HipOperator._ptr(row_perm), obs.ctypes.data, obs.size,
                                           nv.ctypes.data if nv is not None else None, C.byref(self._h), C.c_void_p(s.cuda_stream)))
        self.num_obs = int(obs.size)
        if not hasattr(op, "_conds"):
            op._conds = weakref.WeakSet()
        op._conds.add(self)

    def close(self):
        if self._h:
            self._lib.bfhipCovCondFree(C.byref(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def info(self):
        i = _capi.BfhipCovCondInfo()
        i.structSize = C.sizeof(i)
        check(self._lib.bfhipCovCondGetInfo(self._h, C.byref(i)))
        return i.as_dict()

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)

    def _check_y(self, y):
        import torch
        if y.dtype != torch.float64 or y.numel() != self.num_obs or not y.is_contiguous():
            raise ValueError("y is a contiguous float64 [numObs] tensor")

    def sample_block(self, y, W, eps=None, return_alpha=False):
        """Z [numRows, nrhs] = P A Gamma (W + B^T alpha), alpha = (G + D)^-1 (y 1^T - B W - eps); eps float64 [numObs, nrhs]
        or None (zeros).  With return_alpha: (Z, alpha [numObs, nrhs] float64)."""
        import torch
        self._check_y(y)
        if W.dim() != 2 or not W.is_contiguous() or W.dtype != self._op._torch_dtype():
            raise ValueError("W must be a contiguous [numCols, nrhs] tensor of the operator's element type")
        q = W.shape[1]
        if eps is not None and (eps.dtype != torch.float64 or tuple(eps.shape) != (self.num_obs, q) or not eps.is_contiguous()):
            raise ValueError("eps is a contiguous float64 [numObs, nrhs] tensor")
        z = torch.empty((self._op.shape[0], q), dtype=W.dtype, device=W.device)
        alpha = torch.empty((self.num_obs, q), dtype=torch.float64, device=W.device) if return_alpha else None
        ptr = HipOperator._ptr
        check(self._lib.bfhipCovCondSampleBlockDevice(self._h, ptr(y), ptr(W), ptr(eps), q, ptr(z), ptr(alpha), self._stream()))
        return (z, alpha) if return_alpha else z

    def mean(self, y, return_alpha=False):
        """The posterior mean [numRows] (W = 0, eps = 0).  With return_alpha: (mean, alpha [numObs])."""
        import torch
        self._check_y(y)
        z = torch.empty(self._op.shape[0], dtype=self._op._torch_dtype(), device=y.device)
        alpha = torch.empty(self.num_obs, dtype=torch.float64, device=y.device) if return_alpha else None
        ptr = HipOperator._ptr
        check(self._lib.bfhipCovCondMeanDevice(self._h, ptr(y), ptr(z), ptr(alpha), self._stream()))
        return (z, alpha) if return_alpha else z

    def draw(self, y, seed, noise_seed, first, nrhs):
        """Posterior samples first .. first + nrhs - 1, [numRows, nrhs], from normals generated on the device:
        W[j, s] = N(seed, (first + s) numCols + j), eps[a, s] = sqrt(noise_var[a]) N(noise_seed, (first + s) numObs + a)."""
        import torch
        self._check_y(y)
        z = torch.empty((self._op.shape[0], int(nrhs)), dtype=self._op._torch_dtype(), device=y.device)
        check(self._lib.bfhipCovCondDrawDevice(self._h, HipOperator._ptr(y), int(seed), int(noise_seed), int(first), int(nrhs),
                                               HipOperator._ptr(z), self._stream()))
        return z

    def moments(self, y, seed, noise_seed, first, num, batch=64, sum=None, sumsq=None):
        """Adds the sum and the sum of squares of posterior samples first .. first + num - 1, per point, to the float64
        [numRows] tensors `sum` / `sumsq` (None: not formed; one is needed).  The samples are not stored."""
        import torch
        self._check_y(y)
        for t in (sum, sumsq):
            if t is not None and (t.dtype != torch.float64 or t.numel() != self._op.shape[0] or not t.is_contiguous()):
                raise ValueError("moments are contiguous float64 [numRows] tensors")
        ptr = HipOperator._ptr
        check(self._lib.bfhipCovCondMomentsDevice(self._h, ptr(y), int(seed), int(noise_seed), int(first), int(num), int(batch),
                                                  ptr(sum), ptr(sumsq), self._stream()))
        return sum, sumsq

    def log_likelihood(self, y, grad_log_gamma=False, grad_noise=False, workspace_bytes=0):
        """The log marginal likelihood of y ~ N(0, G + D): a float64 [3] device tensor (logLik, quad = y^T K^-1 y, logDet).
        With a gradient asked for: (value, d logLik / d log gamma [numCols] or None, d logLik / d noise_var [numObs] or None),
        float64 device tensors.  workspace_bytes: scratch of the wide triangular solve (0: the default, at most 256 MiB)."""
        import torch
        self._check_y(y)
        value = torch.empty(3, dtype=torch.float64, device=y.device)
        g = torch.empty(self._op.shape[1], dtype=torch.float64, device=y.device) if grad_log_gamma else None
        h = torch.empty(self.num_obs, dtype=torch.float64, device=y.device) if grad_noise else None
        opt = _capi.BfhipCovCondLikOptions()
        opt.structSize, opt.workspaceBytes = C.sizeof(opt), int(workspace_bytes)
        ptr = HipOperator._ptr
        check(self._lib.bfhipCovCondLogLikelihoodDevice(self._h, ptr(y), ptr(value), ptr(g), ptr(h), C.byref(opt), self._stream()))
        return (value, g, h) if (grad_log_gamma or grad_noise) else value

    def variance(self, query, prior=False, post=True):
        """Exact kriging variances of the latent field at the output indices `query` (distinct, any order): the posterior
        variance [numQuery] float64; with prior=True (posterior, prior); with post=False the prior variance alone."""
        import torch
        q = np.ascontiguousarray(np.asarray(query, dtype=np.uint64))
        if q.ndim != 1:
            raise ValueError("query is one-dimensional")
        if not (prior or post):
            raise ValueError("one of prior / post is needed")
        vpost = torch.empty(q.size, dtype=torch.float64, device=self._dev) if post else None
        vprior = torch.empty(q.size, dtype=torch.float64, device=self._dev) if prior else None
        ptr = HipOperator._ptr
        check(self._lib.bfhipCovCondVarianceDevice(self._h, q.ctypes.data if q.size else None, q.size, ptr(vprior), ptr(vpost), self._stream()))
        return (vpost, vprior) if (prior and post) else (vpost if post else vprior)


class ChebCovCondition(CovCondition):
    """The CovCondition of the Chebyshev route (bfhipChebCovCondCreate): the field z = D p(S) w of a ChebCovariance given noisy
    values at the mesh vertices `obs`.  Every method of CovCondition works on it, on float64 [n, q] blocks in mesh order;
    log_likelihood(grad_log_gamma=True) raises the library's refusal (this route has no per-column weights), and so does every
    method but info and close once set_coefficients has been called on the ChebCovariance: make a new one then.  The object
    keeps its ChebCovariance alive.  On this route alone: log_likelihood_grad, the exact gradient of the likelihood in the
    parameters of the spectral density, and grad_log_scale."""

    def __init__(self, cheb, obs, noise_var=None):
        import torch
        self._op, self._lib, self._h = cheb, cheb._lib, C.c_void_p()       # _op: the shape and element type of the blocks
        self._gamma = self._perm = None
        obs = np.ascontiguousarray(np.asarray(obs, dtype=np.uint64))
        nv = None if noise_var is None else np.ascontiguousarray(np.asarray(noise_var, dtype=np.float64))
        if obs.ndim != 1 or (nv is not None and nv.shape != obs.shape):
            raise ValueError("obs and noise_var are one-dimensional and of one length")
        self._dev = torch.device("cuda", cheb._dev)
        s = torch.cuda.current_stream(self._dev)
        check(self._lib.bfhipChebCovCondCreate(cheb.handle, obs.ctypes.data, obs.size, nv.ctypes.data if nv is not None else None,
                                               C.byref(self._h), C.c_void_p(s.cuda_stream)))
        self.num_obs = int(obs.size)
        self._noise_var = nv

    def log_likelihood_grad(self, y, density_grads, order=None, value=False):
        """The exact gradient of log_likelihood(y)[0] in the parameters of the spectral density
        (bfhipChebCovCondLogLikGradDevice): density_grads is a sequence of callables of lambda, d g / d theta_t (for the Matern
        family: matern_density_grad).  Each is fitted with cheb_fit on [0, lamMax] at the order of the ChebCovariance's
        polynomial (or at `order`: an int, or one per parameter): at that order the result is the derivative of the value the
        library returns.  Returns a float64 [numParams] device tensor; with value=True (gradient, value [3])."""
        import torch
        from .cheb import cheb_fit
        self._check_y(y)
        grads = list(density_grads)
        info = self._op.info()
        if order is None:
            orders = [int(info["order"])] * len(grads)
        elif np.ndim(order) == 0:
            orders = [int(order)] * len(grads)
        else:
            orders = [int(o) for o in order]
        if not grads or len(orders) != len(grads):
            raise ValueError("density_grads is a non-empty sequence of callables, with one order each")
        ld = max(max(orders), 1)
        coef = np.zeros((len(grads), ld), dtype=np.float64)
        for t, (f, o) in enumerate(zip(grads, orders)):
            coef[t, :o] = cheb_fit(f, o, 0.0, info["lamMax"])
        return self.log_likelihood_grad_coef(y, coef, orders, value=value)

    def log_likelihood_grad_coef(self, y, coef, orders=None, value=False):
        """log_likelihood_grad for derivative polynomials given by their Chebyshev coefficients on [0, lamMax]: coef is
        [numParams, ld] float64 on the host, of row t the first orders[t] (None: ld) entries are read."""
        import torch
        self._check_y(y)
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.ndim != 2:
            raise ValueError("coef is [numParams, ld]")
        num, ld = coef.shape
        ords = np.full(num, ld, dtype=np.uintp) if orders is None else np.ascontiguousarray(orders, dtype=np.uintp)
        if ords.shape != (num,):
            raise ValueError("orders has one entry per parameter")
        g = torch.empty(num, dtype=torch.float64, device=y.device)
        v = torch.empty(3, dtype=torch.float64, device=y.device) if value else None
        opt = _capi.BfhipCovCondLikOptions()
        opt.structSize = C.sizeof(opt)
        ptr = HipOperator._ptr
        check(self._lib.bfhipChebCovCondLogLikGradDevice(self._h, ptr(y), coef.ctypes.data, ords.ctypes.data, num, ld, ptr(g), ptr(v), C.byref(opt),
                                                         self._stream()))
        return (g, v) if value else g

    def grad_log_scale(self, y):
        """d logLik / d log s for the covariance s X^T X + N at s = 1, in closed form from outputs the library already has:
        (quad - k) / 2 - sum_a noiseVar[a] gradNoise[a].  A float64 scalar device tensor.  It is what log_likelihood_grad
        returns for the derivative polynomial p / 2."""
        value, _, h = self.log_likelihood(y, grad_noise=True)
        g = (value[1] - self.num_obs) / 2
        if self._noise_var is not None:
            import torch
            g = g - (torch.from_numpy(self._noise_var).to(h.device) * h).sum()
        return g
