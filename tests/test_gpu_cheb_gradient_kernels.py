"""The two kernels of the likelihood's gradient in the density's parameters (bfhip_likgrad.hip) on the
device, one launch at a time through bfdevLikGradContract and bfdevLikGradDot (and the owner's sum, bfdevLikGradSum): torch
tensors as device memory, torch's current stream, a synchronisation before anything is read.

  contract  Y [n x 64] = X [n x k] Mp [k x 64] on the FP64 matrix cores; columns >= pc of Mp are never read (they hold NaN
            here), columns >= pc of Y are written as exact zeros
  dot       part[chunk] = sum over the chunk's 1024 rows and c < pc of Y[r, c] Xp[r, c]; columns >= pc of Y are never read
            (NaN here); `part` holds NaN before the launch

Two designs per shape.  "int": entries in [-3, 3], every product and partial sum an integer far below 2^53, so the device has
to return numpy's float64 result bit for bit whatever its order of summation.  "float": standard normals against
numpy.longdouble under the componentwise bounds of the operation count, u = 2^-53: (k + 2) u |X| |Mp| for Y and
(rows pc + 2) u sum |Y| |Xp| for a chunk of the dot; launched twice into fresh outputs with equal bytes.  Every allocation is
16 rows longer than its block: NaN after an input (a guard that lets row n or index k through turns the result NaN), a sentinel
after an output, intact afterwards.

Shapes: every k in {1, 3, 4, 5, 15, 16, 17, 33, 64, 65, 130, 257} (k mod 4 and k mod 16 of every kind, under and over one block
of 16) at n in {17, 1025}; every n in {1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049, 4099} (the 16-row tile and the
1024-row chunk, the last chunk of 1 and of 3 rows) at k in {33, 130}; pc in {1, 15, 16, 17, 48, 63, 64} (one to four live tile
columns, whole and ragged) at (1025, 33)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
NAN, SENT = float("nan"), -7.25
GUARD_ROWS, TAIL, CHUNK, PANEL = 16, 64, 1024, 64

KS = (1, 3, 4, 5, 15, 16, 17, 33, 64, 65, 130, 257)
NS = (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049, 4099)
PCS = (1, 15, 16, 17, 48, 63, 64)
SHAPES = ([(n, k, min(k, PANEL)) for k in KS for n in (17, 1025)] + [(n, k, min(k, PANEL)) for n in NS for k in (33, 130)]
          + [(1025, 33, pc) for pc in PCS])
SHAPES = sorted(set(SHAPES))


def shape_id(s):
    return "n%d-k%d-pc%d" % s


def bind(lib):
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    for name, args in (("bfdevLikGradContract", [vp, vp, u64, u32, vp, u32, vp]), ("bfdevLikGradDot", [vp, vp, vp, u64, u32, vp]),
                       ("bfdevLikGradSum", [vp, vp, u64, u32, C.c_int, vp])):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    return lib


def design(n, k, pc, kind):
    """X [n x k], Mp [k x 64], Y [n x 64], Xp [n x pc]; the columns >= pc of Mp and Y are NaN: never to be read."""
    rng = np.random.default_rng([n, k, pc, kind == "int"])
    draw = (lambda *s: rng.integers(-3, 4, s).astype(np.float64)) if kind == "int" else (lambda *s: rng.standard_normal(s))
    X, Mp, Y, Xp = draw(n, k), draw(k, PANEL), draw(n, PANEL), draw(n, pc)
    Mp[:, pc:] = NAN
    Y[:, pc:] = NAN
    return X, Mp, Y, Xp


class Device:
    def __init__(self):
        import torch
        from butterfly_amd import _capi
        assert torch.cuda.is_available()
        self.torch, self.lib = torch, bind(_capi.load())
        self.dev = torch.device("cuda", 0)

    @property
    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(0).cuda_stream)

    def block(self, a):
        """The array at the start of an allocation of 16 more rows of NaN."""
        t = self.torch.full((a.shape[0] + GUARD_ROWS,) + a.shape[1:], NAN, dtype=self.torch.float64, device=self.dev)
        t[:a.shape[0]] = self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)
        return t

    def contract(self, dX, dM, n, k, pc):
        out = self.torch.full((n + GUARD_ROWS, PANEL), SENT, dtype=self.torch.float64, device=self.dev)
        assert self.lib.bfdevLikGradContract(out.data_ptr(), dX.data_ptr(), n, k, dM.data_ptr(), pc, self.stream) == 0
        self.torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[n:] == SENT).all()
        return o[:n]

    def dot(self, dY, dXp, n, pc):
        chunks = -(-n // CHUNK)
        part = self.torch.full((chunks + TAIL,), SENT, dtype=self.torch.float64, device=self.dev)
        part[:chunks] = NAN
        assert self.lib.bfdevLikGradDot(part.data_ptr(), dY.data_ptr(), dXp.data_ptr(), n, pc, self.stream) == 0
        self.torch.cuda.synchronize()
        p = part.cpu().numpy()
        assert (p[chunks:] == SENT).all()
        return p[:chunks]


@pytest.fixture(scope="module")
def dev():
    return Device()


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_contract(dev, shape):
    n, k, pc = shape
    for kind in ("int", "float"):
        X, Mp, _, _ = design(n, k, pc, kind)
        dX, dM = dev.block(X), dev.block(Mp)
        y = dev.contract(dX, dM, n, k, pc)
        assert same_bytes(y[:, pc:], np.zeros((n, PANEL - pc)))                    # exact zeros, +0
        if kind == "int":
            ref = X @ Mp[:, :pc]
            print(f"contract {shape_id(shape)} int: {np.count_nonzero(y[:, :pc] != ref)} entries differ")
            assert same_bytes(y[:, :pc] + 0.0, ref + 0.0)
        else:
            ref = X.astype(LD) @ Mp[:, :pc].astype(LD)
            bound = (k + 2) * U * (np.abs(X) @ np.abs(Mp[:, :pc]))
            r = float((np.abs(y[:, :pc].astype(LD) - ref) / bound).max())
            print(f"contract {shape_id(shape)} float: largest error / bound {r:.3e}")
            assert np.isfinite(y).all() and r <= 1
            assert same_bytes(y, dev.contract(dX, dM, n, k, pc))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_dot(dev, shape):
    n, k, pc = shape
    for kind in ("int", "float"):
        _, _, Y, Xp = design(n, k, pc, kind)
        dY, dXp = dev.block(Y), dev.block(Xp)
        got = dev.dot(dY, dXp, n, pc)
        rows = [slice(r0, min(r0 + CHUNK, n)) for r0 in range(0, n, CHUNK)]
        if kind == "int":
            ref = np.array([(Y[r, :pc] * Xp[r]).sum() for r in rows])
            print(f"dot {shape_id(shape)} int: {np.count_nonzero(got != ref)} chunks differ")
            assert same_bytes(got + 0.0, ref + 0.0)
        else:
            ref = np.array([(Y[r, :pc].astype(LD) * Xp[r].astype(LD)).sum() for r in rows])
            bound = np.array([((r.stop - r.start) * pc + 2) * U * (np.abs(Y[r, :pc]) * np.abs(Xp[r])).sum() for r in rows])
            q = float((np.abs(got.astype(LD) - ref) / bound).max())
            print(f"dot {shape_id(shape)} float: largest error / bound {q:.3e}")
            assert np.isfinite(got).all() and q <= 1
            assert same_bytes(got, dev.dot(dY, dXp, n, pc))


def test_the_owner_sums_chunks_then_panels(dev):
    """grad[t] = sum_chunk part[t][chunk], written for the first panel and added to for the next; integers, so bit for bit."""
    torch = dev.torch
    rng = np.random.default_rng(7)
    for chunks, T in ((1, 1), (5, 3), (1025, 64)):
        p0, p1 = rng.integers(-3, 4, (T, chunks)).astype(np.float64), rng.integers(-3, 4, (T, chunks)).astype(np.float64)
        grad = torch.full((T + TAIL,), SENT, dtype=torch.float64, device=dev.dev)
        grad[:T] = NAN
        for first, part in ((1, p0), (0, p1)):
            dP = dev.block(part)
            assert dev.lib.bfdevLikGradSum(grad.data_ptr(), dP.data_ptr(), chunks, T, first, dev.stream) == 0
        torch.cuda.synchronize()
        g = grad.cpu().numpy()
        assert (g[T:] == SENT).all() and same_bytes(g[:T] + 0.0, p0.sum(axis=1) + p1.sum(axis=1) + 0.0)
