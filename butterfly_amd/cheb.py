"""Matrix-free Chebyshev covariance on a sparse FEM operator (bfhipChebCov*, include/bfhip.h): from a triangle mesh
(or any CSR stiffness matrix with a lumped mass) to samples z = D p(S) w and covariance products C v = D p(S)^2 D v on the
GPU, with no eigenpairs and no butterfly.  Blocks are contiguous float64 [n, q] device tensors, in mesh order."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check


def cheb_fit(f, order, a, b):
    """Coefficients of the Chebyshev interpolant of the Python callable f on [a, b] at `order` points (bfhipChebFit)."""
    lib = _capi.load()
    coef = np.zeros(int(order), dtype=np.float64)
    cb = _capi.CHEB_DENSITY_FN(lambda x, _ctx: float(f(x)))
    check(lib.bfhipChebFit(int(order), float(a), float(b), cb, None, coef.ctypes.data))
    return coef


def cheb_eval(coef, a, b, x):
    """The interpolant with coefficients `coef` on [a, b] at x, scalar or array (bfhipChebEval: Clenshaw)."""
    lib = _capi.load()
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    xs = np.asarray(x, dtype=np.float64)
    out = np.array([lib.bfhipChebEval(coef.size, float(a), float(b), coef.ctypes.data, float(v)) for v in xs.ravel()])
    return float(out[0]) if xs.ndim == 0 else out.reshape(xs.shape)


def matern_density(kappa, nu):
    """The spectral density of the reference's covariance examples: exp(-kappa lambda^2) for nu == 0 (squared
    exponential), else the Matern density |1 + kappa^2 lambda|^(-nu / 4 - 1 / 2), normalised to 1 at lambda = 0."""
    kappa, nu = float(kappa), float(nu)
    if nu == 0:
        return lambda lam: np.exp(-kappa * lam * lam)
    return lambda lam: np.abs(1 + kappa * kappa * lam) ** (-nu / 4 - 0.5)


def matern_density_grad(kappa, nu):
    """The derivatives of matern_density(kappa, nu) in its parameters, as callables of lambda >= 0: (d g / d kappa, d g / d nu)
    of the Matern density, and the 1-tuple (d g / d kappa,) of the squared exponential (nu == 0).  What
    ChebCovCondition.log_likelihood_grad takes as `density_grads`."""
    kappa, nu = float(kappa), float(nu)
    if nu == 0:
        return (lambda lam: -lam * lam * np.exp(-kappa * lam * lam),)
    e = -nu / 4 - 0.5
    d_kappa = lambda lam: e * (1 + kappa * kappa * lam) ** (e - 1) * (2 * kappa * lam)
    d_nu = lambda lam: -0.25 * np.log1p(kappa * kappa * lam) * (1 + kappa * kappa * lam) ** e
    return d_kappa, d_nu


def trimesh_lbo_fem(verts, faces):
    """(rowptr, colind, L, mass_lumped) of the P1 stiffness matrix of a triangle mesh (bfhipTrimeshLboFem), host arrays."""
    lib = _capi.load()
    verts = np.ascontiguousarray(verts, dtype=np.float64)
    faces = np.ascontiguousarray(faces, dtype=np.uint64)
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError("verts is [numVerts, 3], faces is [numFaces, 3]")
    nv, nf = verts.shape[0], faces.shape[0]
    nnz = C.c_uint64()
    check(lib.bfhipTrimeshLboFemCount(nv, nf, faces.ctypes.data, C.byref(nnz)))
    rowptr = np.zeros(nv + 1, dtype=np.uint64)
    colind = np.zeros(nnz.value, dtype=np.uint64)
    data = np.zeros(nnz.value, dtype=np.float64)
    mass = np.zeros(nv, dtype=np.float64)
    check(lib.bfhipTrimeshLboFem(nv, verts.ctypes.data, nf, faces.ctypes.data, rowptr.ctypes.data, colind.ctypes.data, data.ctypes.data,
                                 mass.ctypes.data))
    return rowptr, colind, data, mass


def trimesh_lbo_fem_mass(verts, faces, rowptr, colind):
    """The P1 consistent mass M of the mesh on the pattern trimesh_lbo_fem returned (bfhipTrimeshLboFemMass): host [nnz]."""
    lib = _capi.load()
    verts = np.ascontiguousarray(verts, dtype=np.float64)
    faces = np.ascontiguousarray(faces, dtype=np.uint64)
    rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
    colind = np.ascontiguousarray(colind, dtype=np.uint64)
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError("verts is [numVerts, 3], faces is [numFaces, 3]")
    if rowptr.shape != (verts.shape[0] + 1,) or colind.ndim != 1 or int(rowptr[-1]) != colind.size:
        raise ValueError("rowptr [numVerts + 1], colind [nnz] with rowptr[-1] == nnz")
    mdata = np.zeros(colind.size, dtype=np.float64)
    check(lib.bfhipTrimeshLboFemMass(verts.shape[0], verts.ctypes.data, faces.shape[0], faces.ctypes.data, rowptr.ctypes.data, colind.ctypes.data,
                                     mdata.ctypes.data))
    return mdata


class ChebCovariance:
    """S = D L D on the device and a Chebyshev polynomial p of it (include/bfhip.h, "matrix-free Chebyshev covariance")."""

    def __init__(self, handle, n, device):
        self._lib, self._h, self.n, self._dev = _capi.load(), handle, int(n), int(device)

    @classmethod
    def from_csr(cls, rowptr, colind, data, mass_lumped=None, lam_max=None, device=0):
        """rowptr [n + 1], colind, data: host CSR arrays of the stiffness matrix L; mass_lumped [n] positive (None: ones);
        lam_max: an upper bound of the spectrum of S (None: the Gershgorin bound)."""
        lib = _capi.load()
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        colind = np.ascontiguousarray(colind, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=np.float64)
        if rowptr.ndim != 1 or rowptr.size < 1 or colind.ndim != 1 or data.shape != colind.shape or (rowptr.size > 1 and int(rowptr[-1]) != colind.size):
            raise ValueError("rowptr [n + 1], colind [nnz], data [nnz] with rowptr[-1] == nnz")
        n = rowptr.size - 1
        mass = None if mass_lumped is None else np.ascontiguousarray(mass_lumped, dtype=np.float64)
        if mass is not None and mass.shape != (n,):
            raise ValueError("mass_lumped is [n]")
        h = C.c_void_p()
        check(lib.bfhipChebCovCreate(int(device), n, rowptr.ctypes.data, colind.ctypes.data, data.ctypes.data,
                                     mass.ctypes.data if mass is not None else None, 0.0 if lam_max is None else float(lam_max), C.byref(h)))
        obj = cls(h, n, device)
        obj._nnz = int(colind.size)
        return obj

    @classmethod
    def from_trimesh(cls, verts, faces, lam_max=None, device=0, consistent_mass=False):
        """consistent_mass: also set the P1 consistent mass of the mesh (set_consistent_mass with the P1 bounds)."""
        rowptr, colind, data, mass = trimesh_lbo_fem(verts, faces)
        obj = cls.from_csr(rowptr, colind, data, mass, lam_max=lam_max, device=device)
        if consistent_mass:
            obj.set_consistent_mass(trimesh_lbo_fem_mass(verts, faces, rowptr, colind))
        return obj

    def set_consistent_mass(self, mdata, lo=None, hi=None):
        """The consistent mass M for eigs(..., consistent_mass=True): its nnz values on the object's pattern, host
        (bfhipChebCovSetConsistentMass).  [lo, hi] must enclose the spectrum of D M D; None, None asks for the P1 bounds
        [1/4, 1], accepted when the rows of M sum to the lumped mass."""
        mdata = np.ascontiguousarray(mdata, dtype=np.float64)
        nnz = getattr(self, "_nnz", None)
        if nnz is None:
            nnz = self.info()["nnz"]
        if mdata.shape != (nnz,):
            raise ValueError("mdata is [nnz] on the object's pattern")
        if (lo is None) != (hi is None):
            raise ValueError("give both bounds or neither")
        check(self._lib.bfhipChebCovSetConsistentMass(self._h, mdata.ctypes.data, 0.0 if lo is None else float(lo), 0.0 if hi is None else float(hi)))

    def close(self):
        if self._h:
            self._lib.bfhipChebCovFree(C.byref(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def info(self):
        i = _capi.BfhipChebCovInfo()
        i.structSize = C.sizeof(i)
        check(self._lib.bfhipChebCovGetInfo(self._h, C.byref(i)))
        return i.as_dict()

    def set_coefficients(self, coef):
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.ndim != 1:
            raise ValueError("coef is one-dimensional")
        check(self._lib.bfhipChebCovSetCoefficients(self._h, coef.ctypes.data, coef.size))

    def set_density(self, f, order):
        """Fit the spectral density f (a Python callable of lambda) on [0, lamMax] at `order` points in numpy and set it.
        Returns the coefficients."""
        order = int(order)
        lam_max = self.info()["lamMax"]
        j = np.arange(order)
        x = np.sin(np.pi * (2 * j + 1 - order) / (2 * order))
        y = np.array([float(f(lam_max * (t + 1) / 2)) for t in x])
        k = np.arange(order)[:, None]
        coef = (2.0 / order) * (np.cos(k * np.arccos(x)[None, :]) @ y)
        coef[0] /= 2
        self.set_coefficients(coef)
        return coef

    # ---- what a CovCondition asks of the thing it conditions ----
    @property
    def shape(self):
        return (self.n, self.n)

    def _torch_dtype(self):
        import torch
        return torch.float64

    def condition(self, obs, noise_var=None):
        """A CovCondition for the field z = D p(S) w given noisy values at the vertices `obs` (bfhipChebCovCondCreate):
        kriging means, posterior samples and their moments, the log marginal likelihood and exact kriging variances, with
        the coefficients in force now.  set_coefficients afterwards makes it refuse: condition again."""
        from .operator import ChebCovCondition
        return ChebCovCondition(self, obs, noise_var)

    # ---- device entries: contiguous float64 [n, q] tensors on the object's GPU ----
    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)

    def _block(self, t, name):
        import torch
        if t.dim() != 2 or t.shape[0] != self.n or t.dtype != torch.float64 or not t.is_contiguous() or t.device.type != "cuda":
            raise ValueError(f"{name} must be a contiguous float64 [n, q] tensor on the GPU")
        return t

    def _product(self, fn, x):
        import torch
        x = self._block(x, "the input")
        z = torch.empty_like(x)
        check(fn(self._h, C.c_void_p(x.data_ptr()), x.shape[1], C.c_void_p(z.data_ptr()), self._stream()))
        return z

    def apply_block_device(self, W):
        """X = p(S) W (bfhipChebCovApplyBlockDevice)."""
        return self._product(self._lib.bfhipChebCovApplyBlockDevice, W)

    def sample_block_device(self, W):
        """Z = D p(S) W (bfhipChebCovSampleBlockDevice): a sample per standard normal column of W."""
        return self._product(self._lib.bfhipChebCovSampleBlockDevice, W)

    def matvec_block_device(self, V):
        """Z = D p(S) p(S) D V (bfhipChebCovMatvecBlockDevice): the covariance applied to the columns of V."""
        return self._product(self._lib.bfhipChebCovMatvecBlockDevice, V)

    def draw_device(self, seed, first, q):
        """Z [n, q]: samples first .. first + q - 1 from normals generated on the device (bfhipChebCovDrawDevice):
        w_s[j] = N(seed, (first + s) * n + j), whatever the split into calls."""
        import torch
        z = torch.empty((self.n, int(q)), dtype=torch.float64, device=torch.device("cuda", self._dev))
        check(self._lib.bfhipChebCovDrawDevice(self._h, int(seed), int(first), int(q), C.c_void_p(z.data_ptr()), self._stream()))
        return z

    def moments_device(self, seed, first, num, batch=64, sum=None, sumsq=None):
        """Adds the sum and the sum of squares over samples first .. first + num - 1, per point, to the float64 [n] tensors
        `sum` / `sumsq` (bfhipChebCovMomentsDevice; None: that moment is not formed).  Returns (sum, sumsq)."""
        import torch
        for t in (sum, sumsq):
            if t is not None and (t.dtype != torch.float64 or t.numel() != self.n or not t.is_contiguous()):
                raise ValueError("moments are contiguous float64 [n] tensors")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        check(self._lib.bfhipChebCovMomentsDevice(self._h, int(seed), int(first), int(num), int(batch), ptr(sum), ptr(sumsq), self._stream()))
        return sum, sumsq

    def eigs(self, nev, guard=None, degree=None, tol=None, max_iter=None, seed=0, mass_normalised=False, ldu=None, raise_on_limit=True,
             consistent_mass=False, mass_steps=None):
        """The nev lowest eigenpairs of the lumped-mass pencil L phi = lambda M phi (bfhipChebCovEigsDevice): Chebyshev-filtered
        subspace iteration on the device, synchronous.  Returns (lam: numpy [nev] ascending, U: float64 [n, nev] on the GPU,
        info: dict with the residuals under "residual" and the return code under "code").  U has orthonormal columns
        (eigenvectors of S = D L D); with mass_normalised it is Phi = D U, Phi^T M Phi = I.  guard: extra block columns
        (None: the default, 0: none, legal only when nev == n).  ldu > nev returns U as the leading columns of a zero-filled
        [n, ldu] tensor.  raise_on_limit=False returns the best pairs found instead of raising when max_iter was reached.
        consistent_mass: the pencil of set_consistent_mass, L phi = lambda M phi with the consistent M; U then satisfies
        U^T B U = I, B = D M D, and Phi^T M Phi = I as before; mass_steps: steps of every mass solve (None: the default)."""
        import torch
        nev = int(nev)
        opt = _capi.BfhipEigsOptions()
        opt.structSize = C.sizeof(opt)
        opt.guard = 0 if guard is None else int(guard)
        opt.degree = 0 if degree is None else int(degree)
        opt.maxIter = 0 if max_iter is None else int(max_iter)
        opt.tol = 0.0 if tol is None else float(tol)
        opt.seed = int(seed)
        opt.flags = (_capi.EIGS_MASS_NORMALISED if mass_normalised else 0) | (_capi.EIGS_NO_GUARD if guard is not None and int(guard) == 0 else 0)
        opt.flags |= _capi.EIGS_CONSISTENT_MASS if consistent_mass else 0
        opt.massSteps = 0 if mass_steps is None else int(mass_steps)
        info = _capi.BfhipEigsInfo()
        info.structSize = C.sizeof(info)
        ldu = max(nev, 1) if ldu is None else int(ldu)
        lam, res = np.zeros(max(nev, 1)), np.zeros(max(nev, 1))
        full = torch.zeros((self.n, ldu), dtype=torch.float64, device=torch.device("cuda", self._dev))
        rc = self._lib.bfhipChebCovEigsDevice(self._h, C.byref(opt), nev, lam.ctypes.data, res.ctypes.data, C.c_void_p(full.data_ptr()), ldu,
                                              C.byref(info), self._stream())
        if rc != 0 and (raise_on_limit or info.blockColumns == 0):
            check(rc)
        out = info.as_dict()
        out["residual"], out["code"] = res[:nev], rc
        return lam[:nev], full[:, :nev], out

    def eigs_band(self, nev, locked=None, guard=None, degree=None, tol=None, max_iter=None, seed=0, out=None, raise_on_limit=True,
                  consistent_mass=False, mass_steps=None):
        """The nev eigenpairs of S that follow the locked ones (bfhipChebCovEigsBandDevice), with what eigs returns.  locked:
        None, (U_all, lam_all, m) -- a float64 [n, total] tensor on this GPU whose first m columns are the locked vectors, and at
        least m eigenvalues -- or (U, lam) with U an [n, m] tensor or view (unit column stride; any row stride).  The locked vectors
        must be orthonormal eigenvectors of S, not mass-normalised.  out: an [n, nev] view to write into (unit column stride),
        e.g. U_all[:, m:m + nev]; None allocates.  consistent_mass, mass_steps: as in eigs; the locked vectors are then
        B-orthonormal eigenvectors of the consistent pencil."""
        import torch
        nev = int(nev)
        opt = _capi.BfhipEigsOptions()
        opt.structSize = C.sizeof(opt)
        opt.guard = 0 if guard is None else int(guard)
        opt.degree = 0 if degree is None else int(degree)
        opt.maxIter = 0 if max_iter is None else int(max_iter)
        opt.tol = 0.0 if tol is None else float(tol)
        opt.seed = int(seed)
        opt.flags = _capi.EIGS_NO_GUARD if guard is not None and int(guard) == 0 else 0
        opt.flags |= _capi.EIGS_CONSISTENT_MASS if consistent_mass else 0
        opt.massSteps = 0 if mass_steps is None else int(mass_steps)
        info = _capi.BfhipEigsInfo()
        info.structSize = C.sizeof(info)
        dev = torch.device("cuda", self._dev)

        def view(t, cols, what):
            if t.dtype != torch.float64 or t.device != dev or t.dim() != 2 or t.shape[0] != self.n or t.shape[1] < cols:
                raise ValueError(f"{what}: a float64 tensor [n, >= {cols}] on cuda:{self._dev}")
            if cols and (t.stride(1) != 1 or (self.n > 1 and t.stride(0) < cols)):
                raise ValueError(f"{what}: rows must be contiguous (column stride 1)")
            return t.stride(0) if self.n > 1 else max(cols, 1)

        lk, keep = None, None
        if locked is not None:
            U_l, lam_l = locked[0], np.ascontiguousarray(locked[1], dtype=np.float64)
            m = int(locked[2]) if len(locked) > 2 else int(U_l.shape[1])
            if m:
                if lam_l.size < m:
                    raise ValueError("locked: fewer eigenvalues than vectors")
                lk = _capi.BfhipEigsLocked()
                lk.structSize, lk.count, lk.dVectors, lk.ld, lk.lam = C.sizeof(lk), m, U_l.data_ptr(), view(U_l, m, "locked"), lam_l.ctypes.data
                keep = (U_l, lam_l)
        if out is None:
            out = torch.zeros((self.n, max(nev, 1)), dtype=torch.float64, device=dev)
        ldu = view(out, nev, "out")
        lam, res = np.zeros(max(nev, 1)), np.zeros(max(nev, 1))
        rc = self._lib.bfhipChebCovEigsBandDevice(self._h, C.byref(opt), C.byref(lk) if lk is not None else None, nev, lam.ctypes.data, res.ctypes.data,
                                                  C.c_void_p(out.data_ptr()), ldu, C.byref(info), self._stream())
        del keep
        if rc != 0 and (raise_on_limit or info.blockColumns == 0):
            check(rc)
        d = info.as_dict()
        d["residual"], d["code"] = res[:nev], rc
        return lam[:nev], out[:, :nev], d

    def eigs_bands(self, total, band=64, guard=None, degree=None, tol=None, max_iter=None, seed=0, mass_normalised=False, consistent_mass=False,
                   mass_steps=None):
        """The `total` lowest eigenpairs in successive bands of `band` (the last one ragged), each deflated against all the
        earlier ones: (lam [total] ascending, U [n, total] on the GPU, the list of per-band info dicts).  A guard that no longer
        fits the space left is clipped.  mass_normalised scales the rows by d once at the end (Phi = D U)."""
        import torch
        total, band = int(total), int(band)
        if not 1 <= total <= self.n or not 1 <= band <= 255:
            raise ValueError("total in 1 .. n and band in 1 .. 255")
        U = torch.zeros((self.n, total), dtype=torch.float64, device=torch.device("cuda", self._dev))
        lam, infos, m = np.zeros(total), [], 0
        while m < total:
            nev = min(band, total - m)
            left = self.n - m - nev
            g = 0 if left == 0 else None if guard is None else min(int(guard), left, 256 - nev)
            lam_b, _, info = self.eigs_band(nev, (U, lam, m), guard=g, degree=degree, tol=tol, max_iter=max_iter, seed=seed, out=U[:, m:m + nev],
                                          consistent_mass=consistent_mass, mass_steps=mass_steps)
            lam[m:m + nev] = lam_b
            infos.append(info)
            m += nev
        if mass_normalised:
            check(self._lib.bfhipChebCovEigsMassNormaliseDevice(self._h, C.c_void_p(U.data_ptr()), total, total, self._stream()))
        return lam, U, infos

    def eigs_butterfly(self, points, total, band=64, tol=1e-3, eigs_tol=None, consistent_mass=False, return_info=False, batched=False, **kw):
        """The `total` lowest eigenpairs as the operator the rest of the library applies: eigs_bands(total, band,
        mass_normalised=True), then streamer_build.stream_butterfly with freqs = sqrt(max(lam, 0)) over [0, 1.0001 freqs[-1]]
        (kw: freq_depth, wmin, wmax, min_rows, min_cols, factorizer, dtype, check_columns and the compile options; batched=True
        is stream_butterfly's: one batched device call per frontier of the row tree, the same operator bit for bit).  points
        [n, 3]: the mesh vertices, in the order of the object's rows.  Returns (HipOperator, row_perm, lam): the operator
        ~ Phi in tree order to the relative tolerance `tol`, row_perm an int64 tensor on the GPU and lam (numpy) -- the
        arguments cov_sample_block_device and cov_condition take, with gamma_lam a density of lam.  return_info=True appends
        stream_butterfly's info with the dense Phi [n, total] on the GPU under "phi" and the per-band dicts under "eigs".  The eigenvectors and the SVDs of the streamer are computed on
        the GPU; the streamer's recursion runs on the host, in Python (streamer_build's docstring)."""
        import torch
        from .streamer_build import stream_butterfly
        lam, phi, infos = self.eigs_bands(total, band=band, tol=eigs_tol, mass_normalised=True, consistent_mass=consistent_mass)
        freqs = np.sqrt(np.maximum(lam, 0.0))
        wmax = kw.pop("wmax", float(freqs[-1]) * 1.0001)
        op, perm, info = stream_butterfly(points, phi, freqs, wmax, tol=tol, device=self._dev, batched=batched, **kw)
        info["phi"], info["eigs"] = phi, infos
        perm = torch.from_numpy(perm).to(torch.device("cuda", self._dev))
        return (op, perm, lam, info) if return_info else (op, perm, lam)
