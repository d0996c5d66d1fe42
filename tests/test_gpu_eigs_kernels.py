"""The eigensolver's kernels (bfhip_eigs.hip) on the device, one launch at a time through bfdevEigsStep,
bfdevEigsGram, bfdevEigsRotate, bfdevEigsResidual and bfdevEigsStore, on the designs of tests/eigs_kernel_cases.py (whose
claims tests/test_eigs_kernels_cpu.py checks without a GPU): torch tensors as device memory, torch's current stream, a
synchronisation before anything is read.

Per launch: the integer design bit for bit against numpy, the float design under its componentwise bound against the
long-double reference (the largest error / bound is printed first), the float design launched twice into fresh outputs with
equal bytes.  Every block is the start of an allocation 16 rows longer: NaN after an input (a guard that lets row n through
turns the result NaN), a sentinel after an output, and after part, G, sumSq and dst, all intact afterwards; `part` is NaN
before every launch, so the reduction can only have read what the kernels wrote.  Where p < ld the padding of G, of the
rotation and of the residual is exactly zero.

Shapes: tile-column groups <1>; <3>; <4>,<2>; <4>,<3>; <4>,<4>,<1>; four <4> (ld = 16 ... 256) at row counts on the Gram
kernel's 16-row window and on the 1024-row chunk edge; chunks of 1040 rows at (131089, 256); the store's second pass at
70001 x 240; the step at every lane count, one to four panels, rows of 0 to 70 nonzeros, out == b2 and column by column."""
import ctypes as C
import time

import numpy as np
import pytest

import eigs_kernel_cases as ek

pytestmark = pytest.mark.gpu

NAN, SENT = float("nan"), ek.SENTINEL
DENSE_SHAPES = ek.dense_shapes()


class Device:
    def __init__(self):
        import torch
        from butterfly_amd import _capi
        assert torch.cuda.is_available()
        self.torch, self.lib = torch, ek.bind(_capi.load())
        self.dev = torch.device("cuda", 0)

    @property
    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(0).cuda_stream)

    def sync(self):
        self.torch.cuda.synchronize()

    def block(self, a, fill=NAN):
        """The [n, ld] array at the start of an allocation of n + 16 rows, the rest `fill`."""
        t = self.torch.full((a.shape[0] + ek.GUARD_ROWS,) + a.shape[1:], fill, dtype=self.torch.float64, device=self.dev)
        t[:a.shape[0]] = self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)
        return t

    def out_block(self, n, ld):
        return self.torch.full((n + ek.GUARD_ROWS, ld), SENT, dtype=self.torch.float64, device=self.dev)

    def buf(self, count, fill):
        """count doubles of `fill` and a tail of the sentinel."""
        t = self.torch.full((count + ek.TAIL,), SENT, dtype=self.torch.float64, device=self.dev)
        t[:count] = fill
        return t

    def ints(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).to(self.dev)

    def host(self, t, count):
        """(the first `count` entries along axis 0, True when everything after them is still the sentinel)."""
        h = t.cpu().numpy()
        return h[:count], bool((h[count:] == SENT).all())

    # ---- the launches: each returns host arrays after a synchronisation and asserts that every tail is intact -----------------
    def gram(self, dX, dY, n, ld):
        chunks = len(ek.chunks_of(n, ld))
        part, G = self.buf(chunks * ld * ld, NAN), self.buf(ld * ld, SENT)
        assert self.lib.bfdevEigsGram(dX.data_ptr(), dY.data_ptr(), n, ld, part.data_ptr(), G.data_ptr(), self.stream) == 0
        self.sync()
        g, ok = self.host(G, ld * ld)
        assert ok and bool((part[chunks * ld * ld:] == SENT).all())
        return g.reshape(ld, ld)

    def rotate(self, dX, dW, n, ld):
        out = self.out_block(n, ld)
        assert self.lib.bfdevEigsRotate(dX.data_ptr(), dW.data_ptr(), out.data_ptr(), n, ld, self.stream) == 0
        self.sync()
        o, ok = self.host(out, n)
        assert ok
        return o

    def residual(self, dX, dY, dTheta, n, ld):
        chunks = len(ek.chunks_of(n, ld))
        part, s = self.buf(chunks * ld, NAN), self.buf(ld, SENT)
        assert self.lib.bfdevEigsResidual(dX.data_ptr(), dY.data_ptr(), dTheta.data_ptr(), n, ld, part.data_ptr(), s.data_ptr(), self.stream) == 0
        self.sync()
        r, ok = self.host(s, ld)
        assert ok and bool((part[chunks * ld:] == SENT).all())
        return r

    def store(self, dX, n, ld, nev, dD, ldu):
        dst = self.buf(n * ldu, SENT)
        assert self.lib.bfdevEigsStore(dX.data_ptr(), n, ld, nev, dD.data_ptr() if dD is not None else None, dst.data_ptr(), ldu, self.stream) == 0
        self.sync()
        d, ok = self.host(dst, n * ldu)
        assert ok
        return d.reshape(n, ldu)

    def step(self, csr, n, p, ld, b1, b2, out, scalars):
        """One launch, not synchronised; out is a device block the caller made (it may be b2)."""
        rowptr, colind, val = csr
        a = ek.BfEigsStep(rowptr.data_ptr(), colind.data_ptr(), val.data_ptr(), n, p, ld, b1.data_ptr(), b2.data_ptr() if b2 is not None else None,
                          out.data_ptr(), *scalars)
        assert self.lib.bfdevEigsStep(C.byref(a), self.stream) == 0


@pytest.fixture(scope="module")
def dev():
    return Device()


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def held(tag, got, ref_bound, kind):
    """Print the figure, then assert: bit-equal for the integer design, within the bound for the float one."""
    ref, bound = ref_bound
    if kind == "int":
        same = same_bytes(got, ref.astype(np.float64))
        print(f"{tag} int: {'bit-equal' if same else 'DIFFERS in %d entries' % np.count_nonzero(got != ref.astype(np.float64))}")
        assert same
    else:
        r = ek.ratio(got, ref, bound)
        print(f"{tag} float: largest error / bound {r:.3e}")
        assert r <= 1


# ---------------------------------------------------------------------------
# Gram, rotation, residual
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=ek.shape_id)
def test_gram(dev, shape):
    n, ld, p = shape
    for kind in ("int", "float"):
        d = ek.dense(n, ld, p, kind)
        dX, dY = dev.block(d.X), dev.block(d.Y)
        g = dev.gram(dX, dY, n, ld)
        held(f"Gram {ek.shape_id(shape)}", g, d.gram(), kind)
        assert not g[p:].any() and not g[:, p:].any()
        if kind == "float":
            assert same_bytes(g, dev.gram(dX, dY, n, ld))
        if shape in ek.gram_xx_shapes():
            gx = dev.gram(dX, dX, n, ld)
            held(f"Gram(X, X) {ek.shape_id(shape)}", gx, d.gram(True), kind)
            assert not gx[p:].any() and not gx[:, p:].any()


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=ek.shape_id)
def test_rotate(dev, shape):
    n, ld, p = shape
    for kind in ("int", "float"):
        d = ek.dense(n, ld, p, kind)
        dX, dW = dev.block(d.X), dev.block(d.W)
        o = dev.rotate(dX, dW, n, ld)
        held(f"rotate {ek.shape_id(shape)}", o, d.rotate(), kind)
        assert not o[:, p:].any()
        if kind == "float":
            assert same_bytes(o, dev.rotate(dX, dW, n, ld))


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=ek.shape_id)
def test_residual(dev, shape):
    n, ld, p = shape
    for kind in ("int", "float"):
        d = ek.dense(n, ld, p, kind)
        dX, dY, dT = dev.block(d.X), dev.block(d.Y), dev.block(d.theta)
        r = dev.residual(dX, dY, dT, n, ld)
        held(f"residual {ek.shape_id(shape)}", r, d.residual(), kind)
        assert not r[p:].any()
        if kind == "float":
            assert same_bytes(r, dev.residual(dX, dY, dT, n, ld))


# ---------------------------------------------------------------------------
# chunks that are no longer 1024 rows
# ---------------------------------------------------------------------------
def test_chunk_growth_integer_design_bit_for_bit(dev):
    """(131089, 256): 127 chunks of 1040 rows, the last of 49.  Exact in any order, so numpy's float64 result is the reference."""
    t0 = time.perf_counter()
    n, ld = ek.BIG
    d = ek.Dense(n, ld, ld, "int", operands_only=True)
    d.theta = np.arange(ld, dtype=np.float64) % 7 - 3
    assert ek.chunk_rows(n, ld) == dev.lib.bfdevEigsChunkRows(n, ld) == 1040 and len(ek.chunks_of(n, ld)) == 127
    t1 = time.perf_counter()
    dX, dY, dT = dev.block(d.X), dev.block(d.Y), dev.block(d.theta)
    g = dev.gram(dX, dY, n, ld)
    r = dev.residual(dX, dY, dT, n, ld)
    t2 = time.perf_counter()
    g_ref, r_ref = d.gram64(), ((d.Y - d.theta * d.X) ** 2).sum(axis=0)
    t3 = time.perf_counter()
    print(f"(131089, 256) int: design {t1 - t0:.2f} s, upload and both launches {t2 - t1:.2f} s, numpy references {t3 - t2:.2f} s; "
          f"Gram differs in {np.count_nonzero(g != g_ref)} entries, residual in {np.count_nonzero(r != r_ref)}; max |G| {np.abs(g_ref).max():.0f}")
    assert same_bytes(g, g_ref)
    assert same_bytes(r, r_ref)


def test_chunk_growth_float_design_reads_only_what_was_written(dev):
    """The same shape in standard normals, `part` NaN before the launch as everywhere here.  No long-double reference at this
    size: the results are finite, repeat bit for bit, and every 5th column of G and of sumSq lies within twice the bound of
    numpy's float64 result (each side is within one bound of the exact value)."""
    t0 = time.perf_counter()
    n, ld = ek.BIG
    rng = np.random.default_rng(131089)
    X, Y, theta = rng.standard_normal((n, ld)), rng.standard_normal((n, ld)), rng.standard_normal(ld)
    dX, dY, dT = dev.block(X), dev.block(Y), dev.block(theta)
    g, r = dev.gram(dX, dY, n, ld), dev.residual(dX, dY, dT, n, ld)
    assert np.isfinite(g).all() and np.isfinite(r).all()
    assert same_bytes(g, dev.gram(dX, dY, n, ld)) and same_bytes(r, dev.residual(dX, dY, dT, n, ld))
    cols = np.arange(0, ld, 5)
    Yc = np.ascontiguousarray(Y[:, cols])
    g64, gb = X.T @ Yc, 2 * (n + 2) * ek.U * (np.abs(X).T @ np.abs(Yc))
    hi, lo = ek.two_prod(theta[cols], np.ascontiguousarray(X[:, cols]))          # theta X = hi + lo exactly: d without the fma the host lacks
    r64 = (((Yc - hi) - lo) ** 2).sum(axis=0)
    rb = 2 * (n + 8) * ek.U * r64
    rg, rr = float((np.abs(g[:, cols] - g64) / gb).max()), float((np.abs(r[cols] - r64) / rb).max())
    print(f"(131089, 256) float, {time.perf_counter() - t0:.2f} s: Gram against float64 at {rg:.3e} of twice the bound, residual at {rr:.3e}")
    assert rg <= 1 and rr <= 1


# ---------------------------------------------------------------------------
# store
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ek.STORE_SHAPES, ids=lambda s: "n%d-ld%d-nev%d-ldu%d" % s)
def test_store(dev, shape):
    t0 = time.perf_counter()
    n, ld, nev, ldu = shape
    X, d = ek.store_design(*shape)
    dX, dD = dev.block(X), dev.block(d)
    for scale in (None, d):
        got = dev.store(dX, n, ld, nev, dD if scale is not None else None, ldu)
        want = X[:, :nev] if scale is None else scale[:, None] * X[:, :nev]
        bad = np.count_nonzero(got[:, :nev] != want)
        print(f"store {shape} d={'yes' if scale is not None else 'no'}: {bad} entries differ, padding intact {bool((got[:, nev:] == SENT).all())}")
        assert same_bytes(got[:, :nev], want)
        assert (got[:, nev:] == SENT).all()
    print(f"store {shape}: {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------
# step
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def csr(dev):
    made = {}

    def get(name, kind):
        if (name, kind) not in made:
            s = ek.step_design(name, kind)
            made[name, kind] = (dev.ints(s.rowptr, np.int64), dev.ints(s.colind, np.int32), dev.block(s.val))
        return made[name, kind]
    return get


def padded(a, p, ld):
    out = np.zeros((a.shape[0], ld))
    out[:, :p] = a[:, :p]
    return out


@pytest.mark.parametrize("name", ek.STEP_MATRICES)
@pytest.mark.parametrize("p", ek.STEP_PS)
def test_step(dev, csr, name, p):
    ld = -(-p // 16) * 16
    for kind in ("int", "float"):
        s = ek.step_design(name, kind)
        n, scal, mat = s.n, (s.alpha, s.beta, s.gamma), csr(name, kind)
        b1, b2 = dev.block(padded(s.b1, p, ld)), dev.block(padded(s.b2, p, ld))

        def launch(form):
            """form: "null" (b2 NULL), "b2" (out of place), "inplace" (out == b2: a copy of b2 whose padding is the sentinel)."""
            out = dev.out_block(n, ld)
            if form == "inplace":
                out[:n, :p] = b2[:n, :p]
            dev.step(mat, n, p, ld, b1, None if form == "null" else out if form == "inplace" else b2, out, scal)
            dev.sync()
            o = out.cpu().numpy()
            assert (o[n:] == SENT).all() and (o[:n, p:] == SENT).all()            # rows from n on and columns from p on: never written
            return o[:n, :p]

        tag = f"step {name} p={p}"
        for form in ("null", "b2"):
            ref, bound = s.reference(form == "b2")
            o = launch(form)
            held(f"{tag} {form}", o, (ref[:, :p], bound[:, :p]), kind)
            if kind == "float":
                assert same_bytes(o, launch(form))
        assert same_bytes(o, launch("inplace"))
        if kind == "float" and p in ek.STEP_COLUMNWISE_PS:
            # column c alone as a one-column block of ld = 16: the same bits
            B1 = dev.torch.zeros((p, n + ek.GUARD_ROWS, 16), dtype=dev.torch.float64, device=dev.dev)
            B1[:, n:] = NAN
            B2, O = B1.clone(), dev.torch.full_like(B1, SENT)
            B1[:, :n, 0], B2[:, :n, 0] = b1[:n, :p].T, b2[:n, :p].T
            for c in range(p):
                dev.step(mat, n, 1, 16, B1[c], B2[c], O[c], scal)
            dev.sync()
            O = O.cpu().numpy()
            assert (O[:, n:] == SENT).all() and (O[:, :n, 1:] == SENT).all()
            diff = np.count_nonzero(O[:, :n, 0].T != o)
            print(f"{tag}: column by column, {diff} entries differ")
            assert same_bytes(O[:, :n, 0].T, o)
