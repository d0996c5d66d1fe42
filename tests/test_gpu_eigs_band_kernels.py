"""The two deflation kernels (bfEigsCrossGramKernel, bfEigsDeflateKernel; bfhip_eigs.hip) on the device, one
launch at a time through bfdevEigsCrossGram and bfdevEigsDeflate, and the panel walk bfdevEigsProject, on the designs of
tests/eigsband_cases.py, in the manner of tests/test_gpu_eigs_kernels.py: torch tensors as device memory, torch's current
stream, a synchronisation before anything is read.

Per launch: the integer design bit for bit against numpy, the float design under its componentwise bound against the
long-double reference (the largest error / bound is printed first), the float design launched twice into fresh outputs with
equal bytes.  Q lies in a flat buffer that is NaN wherever the panel is not (before it, between its rows, 16 rows after it); X
is followed by 16 rows of NaN as an input and of the sentinel as an output; `part` is NaN before every launch and followed,
like C, by sentinels that must survive.  The padding rows of C (from mq to mq16) must be exact +0, sign included; the padding
columns of X hold zeros that must stay zeros, also when X is a view into a wider allocation whose neighbours are sentinels.

Shapes: mq in {1, 15, 16, 17, 64, 100, 255, 256}, ld in {16, 48, 112, 256} with p < ld in half, n from 1 to 2049 across the
16-row window and the 1024-row chunk, ldq in {mq, mq + 1, mq + 3, a multiple of 4}, column offsets {0, 1, 4, 255} and a base
offset of one double, so that both A-operand paths of the deflation run; the walk at m = 257 and 300 (two panels)."""
import ctypes as C

import numpy as np
import pytest

import eigs_kernel_cases as ek
import eigsband_cases as eb

pytestmark = pytest.mark.gpu

NAN, SENT = float("nan"), ek.SENTINEL
SHAPES = eb.kernel_shapes()


class Device:
    def __init__(self):
        import torch
        from butterfly_amd import _capi
        assert torch.cuda.is_available()
        self.torch, self.lib = torch, eb.bind(_capi.load())
        self.dev = torch.device("cuda", 0)

    @property
    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(0).cuda_stream)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def block(self, a, fill):
        """The [n, ld] array at the start of an allocation 16 rows longer, the rest `fill`."""
        t = self.torch.full((a.shape[0] + ek.GUARD_ROWS,) + a.shape[1:], fill, dtype=self.torch.float64, device=self.dev)
        t[:a.shape[0]] = self.up(a)
        return t

    def buf(self, count, fill):
        t = self.torch.full((count + ek.TAIL,), SENT, dtype=self.torch.float64, device=self.dev)
        t[:count] = fill
        return t

    def q(self, design):
        """(the flat buffer on the device, the address of the panel's column 0 minus m0 columns: what the launch takes as dQ)."""
        flat, base = design.flat_q()
        t = self.up(flat)
        assert t.data_ptr() % 32 == 0
        return t, t.data_ptr() + 8 * base

    def cross(self, dQ, shape, dX):
        n, mq, ld, p, ldq, m0, base = shape
        mq16, chunks = -(-mq // 16) * 16, len(eb.cross_chunks_of(n, ld))
        part, Cd = self.buf(chunks * mq16 * ld, NAN), self.buf(mq16 * ld, SENT)
        assert self.lib.bfdevEigsCrossGram(dQ, ldq, m0, mq, dX.data_ptr(), n, ld, part.data_ptr(), Cd.data_ptr(), self.stream) == 0
        self.torch.cuda.synchronize()
        c = Cd.cpu().numpy()
        assert (c[mq16 * ld:] == SENT).all() and bool((part[chunks * mq16 * ld:] == SENT).all())
        return c[:mq16 * ld].reshape(mq16, ld)

    def deflate(self, dQ, shape, dC, X):
        """X is uploaded into a fresh block followed by sentinel rows; returns the block's first n rows after the launch."""
        n, mq, ld, p, ldq, m0, base = shape
        dX = self.block(X, SENT)
        assert self.lib.bfdevEigsDeflate(dQ, ldq, m0, mq, dC.data_ptr(), dX.data_ptr(), n, ld, self.stream) == 0
        self.torch.cuda.synchronize()
        x = dX.cpu().numpy()
        assert (x[n:] == SENT).all()
        return x[:n]


@pytest.fixture(scope="module")
def dev():
    return Device()


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def held(tag, got, ref_bound, kind):
    ref, bound = ref_bound
    if kind == "int":
        same = same_bytes(got, ref.astype(np.float64))
        print(f"{tag} int: {'bit-equal' if same else 'DIFFERS in %d entries' % np.count_nonzero(got != ref.astype(np.float64))}")
        assert same
    else:
        r = ek.ratio(got, ref, bound)
        print(f"{tag} float: largest error / bound {r:.3e}")
        assert r <= 1


def test_the_chunk_rule_is_the_restated_one(dev):
    for n, ld in ((1, 16), (4221, 80), (1 << 20, 64), (1 << 20, 256), (1 << 24, 256), (10 ** 6 + 1, 48), (131089, 256)):
        assert dev.lib.bfdevEigsCrossChunkRows(n, ld) == eb.cross_chunk_rows(n, ld)
        assert len(eb.cross_chunks_of(n, ld)) * 256 * ld <= 1 << 23


@pytest.mark.parametrize("shape", SHAPES, ids=eb.kshape_id)
def test_cross_gram(dev, shape):
    n, mq, ld, p, ldq, m0, base = shape
    for kind in ("int", "float"):
        d = eb.band_design(shape, kind)
        keep, dQ = dev.q(d)
        dX = dev.block(d.X, NAN)
        c = dev.cross(dQ, shape, dX)
        held(f"cross-Gram {eb.kshape_id(shape)}", c, d.cross(), kind)
        assert not c[mq:].any() and not np.signbit(c[mq:]).any()                  # the padding rows: exact +0
        assert not c[:, p:].any()
        if kind == "float":
            assert same_bytes(c, dev.cross(dQ, shape, dX))
        del keep


@pytest.mark.parametrize("shape", SHAPES, ids=eb.kshape_id)
def test_deflate(dev, shape):
    n, mq, ld, p, ldq, m0, base = shape
    for kind in ("int", "float"):
        d = eb.band_design(shape, kind)
        keep, dQ = dev.q(d)
        dC = dev.block(d.C, NAN)
        x = dev.deflate(dQ, shape, dC, d.X)
        held(f"deflate {eb.kshape_id(shape)} ({'vector' if eb.vector_path(shape) else 'scalar'} A)", x, d.deflate(), kind)
        assert not x[:, p:].any()
        if kind == "float":
            assert same_bytes(x, dev.deflate(dQ, shape, dC, d.X))
        del keep


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] < s[2]][::4], ids=eb.kshape_id)
def test_deflate_on_a_view_keeps_its_zero_padding_and_its_neighbours(dev, shape):
    """X as a row range of a longer allocation (sentinel rows before and after it), its padding columns zeros: they stay +0, the
    neighbours stay sentinels, and the result equals the launch on a block of its own bit for bit."""
    n, mq, ld, p, ldq, m0, base = shape
    d = eb.band_design(shape, "float")
    keep, dQ = dev.q(d)
    dC = dev.block(d.C, NAN)
    wide = dev.torch.full((n + 2 * ek.GUARD_ROWS, ld), SENT, dtype=dev.torch.float64, device=dev.dev)
    wide[ek.GUARD_ROWS:ek.GUARD_ROWS + n] = dev.up(d.X)
    view = wide[ek.GUARD_ROWS:]
    assert dev.lib.bfdevEigsDeflate(dQ, ldq, m0, mq, dC.data_ptr(), view.data_ptr(), n, ld, dev.stream) == 0
    dev.torch.cuda.synchronize()
    w = wide.cpu().numpy()
    x = w[ek.GUARD_ROWS:ek.GUARD_ROWS + n]
    assert (w[:ek.GUARD_ROWS] == SENT).all() and (w[ek.GUARD_ROWS + n:] == SENT).all()
    assert not x[:, p:].any() and not np.signbit(x[:, p:]).any()
    assert same_bytes(x, dev.deflate(dQ, shape, dC, d.X))
    del keep


@pytest.mark.parametrize("m", eb.WALK_MS)
def test_the_panel_walk_is_the_two_launches_per_panel_in_order(dev, m):
    """bfdevEigsProject at m = 257 and 300 (panels of 256 and of 1 or 44), Q [n, ldq] with ldq = m + 3: bit for bit numpy's
    float64 walk on the integer design (exact), and on the float design bit for bit the same panels launched one by one."""
    n, ld, p, ldq = 1025, 48, 33, m + 3
    for kind in ("int", "float"):
        rng = np.random.default_rng([m, int(kind == "int")])
        Q, X = np.full((n + ek.GUARD_ROWS, ldq), np.nan), np.zeros((n, ld))
        Q[:n, :m], X[:, :p] = ek.draw(rng, kind, (n, m)), ek.draw(rng, kind, (n, p))
        dQ = dev.up(Q)
        chunks = len(eb.cross_chunks_of(n, ld))
        part, Cd = dev.buf(chunks * 256 * ld, NAN), dev.buf(256 * ld, SENT)
        dX = dev.block(X, SENT)
        assert dev.lib.bfdevEigsProject(dQ.data_ptr(), ldq, m, dX.data_ptr(), n, ld, part.data_ptr(), Cd.data_ptr(), dev.stream) == 0
        dev.torch.cuda.synchronize()
        x = dX.cpu().numpy()
        assert (x[n:] == SENT).all() and bool((Cd[256 * ld:] == SENT).all()) and bool((part[chunks * 256 * ld:] == SENT).all())
        x = x[:n]
        assert not x[:, p:].any()
        if kind == "int":
            want = eb.project(X, Q[:n, :m], ld=ld) + 0.0
            print(f"walk m={m} int: {np.count_nonzero(x != want)} entries differ, largest |entry| {np.abs(want).max():.3g}")
            assert np.abs(want).max() < 2.0 ** 52 and same_bytes(x, want)
        else:
            dY = dev.block(X, SENT)
            for m0, m1 in eb.panels_of(m):
                part2, C2 = dev.buf(chunks * 256 * ld, NAN), dev.buf(256 * ld, SENT)
                assert dev.lib.bfdevEigsCrossGram(dQ.data_ptr(), ldq, m0, m1 - m0, dY.data_ptr(), n, ld, part2.data_ptr(), C2.data_ptr(), dev.stream) == 0
                assert dev.lib.bfdevEigsDeflate(dQ.data_ptr(), ldq, m0, m1 - m0, C2.data_ptr(), dY.data_ptr(), n, ld, dev.stream) == 0
            dev.torch.cuda.synchronize()
            assert same_bytes(x, dY.cpu().numpy()[:n])
            assert np.isfinite(x).all()
