"""Shared by tests/test_cheb_cov_cpu.py and tests/test_gpu_cheb_cov.py: the meshes and matrices of
the Chebyshev covariance tests, a numpy cotangent assembly, the folding S = D L D restated, and the reference's forward
recurrence (examples/covariance/cheb_cov.c: chebmul) in any numpy float type -- numpy.longdouble is the reference of the
GPU tests, float64 gives the reference algorithm's own error."""
import numpy as np

LD = np.longdouble


# ---- meshes -------------------------------------------------------------------------------------------------------------
def grid_faces(nx, ny):
    """Two triangles per cell of an nx x ny vertex grid, vertex (i, j) = i * ny + j."""
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a, b, c, d = (i * ny + j).ravel(), ((i + 1) * ny + j).ravel(), ((i + 1) * ny + j + 1).ravel(), (i * ny + j + 1).ravel()
    return np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.uint64)


def jittered_grid_mesh(nx=7, ny=9, seed=3):
    """A jittered nx x ny grid lifted out of the plane: nx * ny vertices, rows of 3 - 7 nonzeros."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx, dtype=float), np.arange(ny, dtype=float), indexing="ij")
    x = x + 0.25 * (rng.random(x.shape) - 0.5)
    y = y + 0.25 * (rng.random(y.shape) - 0.5)
    z = 0.3 * np.sin(0.9 * x) * np.cos(0.7 * y) + 0.05 * rng.random(x.shape)
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1), grid_faces(nx, ny)


def structured_mesh_4099():
    """A 64 x 64 grid on a gently curved sheet plus three ears on its boundary: 4099 vertices."""
    nx = ny = 64
    x, y = np.meshgrid(np.arange(nx, dtype=float), np.arange(ny, dtype=float), indexing="ij")
    z = 2.0 * np.sin(0.11 * x) * np.cos(0.07 * y)
    verts = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    faces = [grid_faces(nx, ny)]
    extra = []
    for k, j in enumerate((5, 20, 41)):                 # ear k over the boundary edge (0, j) - (0, j + 1)
        extra.append([-0.8, j + 0.5, 0.1 * k])
        faces.append(np.array([[j + 1, j, nx * ny + k]], dtype=np.uint64))
    return np.concatenate([verts, np.array(extra)]), np.concatenate(faces)


def lat_lon_sphere(nlat, nlon):
    """Unit sphere: two poles and nlat rings of nlon vertices."""
    th = np.pi * (np.arange(nlat) + 1) / (nlat + 1)
    ph = 2 * np.pi * np.arange(nlon) / nlon
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(nlon))], 2).reshape(-1, 3)
    verts = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]])
    f = []
    for j in range(nlon):
        jn = (j + 1) % nlon
        f.append([0, 1 + j, 1 + jn])
        for r in range(nlat - 1):
            a, b, c, d = 1 + r * nlon + j, 1 + (r + 1) * nlon + j, 1 + (r + 1) * nlon + jn, 1 + r * nlon + jn
            f += [[a, b, c], [a, c, d]]
        f.append([1 + (nlat - 1) * nlon + j, 1 + nlat * nlon, 1 + (nlat - 1) * nlon + jn])
    return verts, np.array(f, dtype=np.uint64)


# ---- assembly and folding, restated ------------------------------------------------------------------------------------
def cotan_dense(verts, faces):
    """(L, mass_lumped, area): dense cotangent stiffness matrix, a third of the incident area per vertex, total area."""
    n = len(verts)
    L, mass, area = np.zeros((n, n)), np.zeros(n), 0.0
    for f in faces.astype(np.int64):
        for k in range(3):
            o, i, j = f[k], f[(k + 1) % 3], f[(k + 2) % 3]
            u, v = verts[i] - verts[o], verts[j] - verts[o]
            cr = np.linalg.norm(np.cross(u, v))
            w = 0.5 * np.dot(u, v) / cr
            L[i, j] -= w; L[j, i] -= w; L[i, i] += w; L[j, j] += w
            mass[o] += cr / 6
        area += cr / 2
    return L, mass, area


def csr_to_dense(rowptr, colind, data, n):
    A = np.zeros((n, n), dtype=np.asarray(data).dtype)
    for i in range(n):
        for k in range(int(rowptr[i]), int(rowptr[i + 1])):
            A[i, int(colind[k])] += data[k]
    return A


def dense_to_csr(A, keep=None):
    """CSR of the dense A, storing the entries where `keep` (default: A != 0) holds, columns increasing."""
    keep = (A != 0) if keep is None else keep
    rowptr, colind, data = [0], [], []
    for i in range(A.shape[0]):
        js = np.nonzero(keep[i])[0]
        colind += list(js); data += list(A[i, js]); rowptr.append(len(colind))
    return np.array(rowptr, dtype=np.uint64), np.array(colind, dtype=np.uint64), np.array(data, dtype=np.float64)


def fold(rowptr, colind, data, mass):
    """(S values, d, Gershgorin bound) exactly as bfhipChebCovCreate folds: S[i][j] = (d[i] * L[i][j]) * d[j],
    d = 1 / sqrt(mass), the bound summed in row order."""
    n = len(rowptr) - 1
    d = np.ones(n) if mass is None else 1 / np.sqrt(np.asarray(mass, dtype=np.float64))
    rows = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    val = (d[rows] * data) * d[colind.astype(np.int64)]
    gersh = 0.0
    for i in range(n):
        s = 0.0
        for k in range(int(rowptr[i]), int(rowptr[i + 1])):
            s += abs(val[k])
        gersh = max(gersh, s)
    return val, d, gersh


class Ell:
    """S as padded rows (values of the given float type) for a matvec whose row sums run in CSR order."""
    def __init__(self, rowptr, colind, val, dtype):
        rp = rowptr.astype(np.int64)
        n, deg = len(rp) - 1, np.diff(rp)
        self.n, self.width = n, int(deg.max()) if n and len(colind) else 0
        self.cols = np.zeros((n, max(self.width, 1)), dtype=np.int64)
        self.vals = np.zeros((n, max(self.width, 1)), dtype=dtype)
        for i in range(n):
            self.cols[i, :deg[i]] = colind[rp[i]:rp[i + 1]]
            self.vals[i, :deg[i]] = val[rp[i]:rp[i + 1]]
        self.dtype = dtype

    def mul(self, X):
        Y = np.zeros_like(X)
        for k in range(self.width):
            Y += self.vals[:, k, None] * X[self.cols[:, k], :]
        return Y


def forward_recurrence(ell, lam_max, coef, W):
    """chebmul of cheb_cov.c in ell.dtype: x = sum_k c_k T_k(2 S / lamMax - I) W by the forward three-term recurrence."""
    dt = ell.dtype
    c, lam, W = np.asarray(coef, dtype=dt), dt(lam_max), np.asarray(W, dtype=dt)
    x = c[0] * W
    if len(c) == 1:
        return x
    y2 = W
    y1 = ell.mul(W) * (dt(2) / lam) - W
    x = x + c[1] * y1
    for k in range(2, len(c)):
        y = ell.mul(y1) * (dt(4) / lam) - dt(2) * y1 - y2
        x = x + c[k] * y
        y2, y1 = y1, y
    return x


# ---- matrices of the GPU tests -----------------------------------------------------------------------------------------
def graph_laplacian(n, edges, weights):
    A = np.zeros((n, n))
    for (i, j), w in zip(edges, weights):
        A[i, j] -= w; A[j, i] -= w; A[i, i] += w; A[j, j] += w
    return A


def catalogue():
    """name -> dict(rowptr, colind, data, mass, lam_max (None: Gershgorin), extra): all symmetric positive semidefinite, so
    the spectrum of S lies in [0, lamMax] and |T_k| <= 1 on it."""
    rng = np.random.default_rng(2024)
    out = {}
    from butterfly_amd import trimesh_lbo_fem
    for name, (verts, faces) in (("mesh63", jittered_grid_mesh()), ("mesh4099", structured_mesh_4099())):
        rowptr, colind, data, mass = trimesh_lbo_fem(verts, faces)
        out[name] = dict(rowptr=rowptr, colind=colind, data=data, mass=mass, lam_max=None)
    out["n1"] = dict(rowptr=np.array([0, 1], dtype=np.uint64), colind=np.array([0], dtype=np.uint64), data=np.array([3.0]), mass=np.array([0.7]), lam_max=None)
    r, c, d = dense_to_csr(graph_laplacian(5, [(i, i + 1) for i in range(4)], [1.0, 2.0, 0.5, 1.5]))
    out["path5"] = dict(rowptr=r, colind=c, data=d, mass=None, lam_max=None)
    # vertex 0 has 69 neighbours (a row of 70 nonzeros: more than a wavefront is wide), vertex 99 none and no stored entry
    n = 100
    edges = [(0, j) for j in range(1, 70)] + [(int(a), int(b)) for a, b in rng.integers(1, 99, (150, 2)) if a != b]
    r, c, d = dense_to_csr(graph_laplacian(n, edges, rng.random(len(edges)) + 0.2))
    assert r[1] - r[0] == 70 and r[100] == r[99]
    out["wide_and_empty"] = dict(rowptr=r, colind=c, data=d, mass=rng.random(n) + 0.5, lam_max=None)
    Q, _ = np.linalg.qr(rng.standard_normal((48, 48)))
    lam = np.sort(np.concatenate([[0.0, 1.0], rng.random(46)]))
    S = (Q * lam) @ Q.T
    S = (S + S.T) / 2
    r, c, d = dense_to_csr(S, keep=np.ones_like(S, dtype=bool))
    out["dense48"] = dict(rowptr=r, colind=c, data=d, mass=None, lam_max=None, Q=Q, lam=lam)
    return out
