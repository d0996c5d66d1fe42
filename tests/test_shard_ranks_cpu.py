"""What tests/test_gpu_shard_ranks.py relies on, checked without a GPU:

* the numpy assembly of a sharded step (shard_ranks.place_segments / range_sums / rank_order_sum / gather_rows) applied to
  the ORACLE's per-shard results reproduces the oracle's whole-operator product to 1e-12, for every partition and world
  the GPU tests use -- the reference is right before a GPU runs against it;
* the stand-in for the collectives compiles with -Wall -Werror;
* BFHIP_RCCL_LIBRARY: a path that cannot be loaded is the RUNTIME_ERROR that names it (not a crash, no fallback), and a
  path that can is the library libbfhip.so uses."""
import os
import subprocess
import sys

import numpy as np
import pytest

import shard_ranks as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _assemble(layout, mode, loc_y, loc_z):
    if mode in ("rows", "rowblocks"):
        y = sr.place_segments(layout, loc_y)
    elif mode == "rowsum":
        y = sr.range_sums(layout, loc_y)
    else:
        y = sr.rank_order_sum(loc_y)
    return y, sr.rank_order_sum(loc_z)


@pytest.fixture(scope="module")
def complex_whole():
    from oracle import bfref
    opd = sr.complex_operand()
    A = bfref.from_desc(opd.desc, None, seed=opd.seed)
    dense = np.concatenate([bfref.mat_mul(A, np.eye(opd.n, 256, -c0, dtype=complex)) for c0 in range(0, opd.n, 256)], axis=1)
    return A, dense


@pytest.mark.parametrize("mode", sr.MODES)
def test_assembly_of_the_oracles_shards_is_the_oracles_whole_product(complex_whole, mode):
    """Complex operand, worlds 2, 3 and 5 (and the 3-rank deal that leaves rank 2 without rows), nrhs 1 and 3: each shard
    is its own oracle graph (bfref.from_desc(..., root=shard root)).  A row range has no graph of its own: its "shard" is
    those rows of the whole operator's dense form, so in `rows` mode the forward half only checks that the cuts tile the
    rows; the adjoint half (gather_rows + the rank-order sum) is the check there."""
    from oracle import bfref
    A, dense = complex_whole
    deals = [(w, None) for w in sr.WORLDS] + ([(3, [0, 1] * 6)] if mode == "rowblocks" else [])
    for world, owner in deals:
        opd = sr.complex_operand()
        layout, shards = sr.partition(opd, mode, world, owner=owner)
        if mode == "rows":
            assert layout.cuts == {2: [0, 512, 1024], 3: [0, 342, 682, 1024], 5: [0, 256, 512, 768, 939, 1024]}[world]
            local = [dense[layout.cuts[r]:layout.cuts[r + 1]] for r in range(world)]
        else:
            local = []
            for r in range(world):
                rows = len(sr.my_rows(layout, r, mode))
                if rows == 0:
                    local.append(np.zeros((0, opd.n), dtype=complex))
                    continue
                Ar = bfref.from_desc(opd.desc, None, seed=opd.seed, root=shards[r]["root"])
                assert Ar.shape == (rows, opd.n)
                local.append(np.concatenate([bfref.mat_mul(Ar, np.eye(opd.n, 256, -c0, dtype=complex)) for c0 in range(0, opd.n, 256)], axis=1))
        if mode == "rowblocks" and owner is None and world in (3, 5):
            assert layout.owner == {3: [1, 2, 0, 1, 1, 2, 0, 1, 2, 0, 2, 0], 5: [4, 4, 0, 1, 0, 1, 2, 3, 2, 3, 4, 0]}[world]
        for nrhs in sr.NRHS:
            x, v = sr.vectors(opd, np.complex128, nrhs, 100 + nrhs)
            loc_y = [d @ x for d in local]
            loc_z = [d.T @ sr.gather_rows(layout, r, mode, v) for r, d in enumerate(local)]
            y, z = _assemble(layout, mode, loc_y, loc_z)
            assert sr.rel(y, bfref.mat_mul(A, x)) <= TOL and sr.rel(z, dense.T @ v) <= TOL, (mode, world, nrhs)


@pytest.mark.parametrize("seed", sr.REAL_SEEDS)
def test_assembly_of_real_row_ranges_is_the_oracles_whole_product(seed):
    """The cuts the GPU test relies on, and the adjoint assembly (gather_rows + rank-order sum over the dense rows of each range)
    against the oracle's A^T v.  The forward half places slices of the oracle's own y: it checks that the cuts tile the rows,
    nothing more."""
    import randgraph
    from oracle import bfref
    opd, _ = sr.real_operand(seed)
    A = bfref.from_desc(opd.desc, opd.vals)
    dense = randgraph.densify(opd.desc, opd.vals, opd.root)
    want_cuts = {33: {2: [0, 82, 272], 3: [0, 82, 271, 272]}, 41: {2: [0, 28, 224], 3: [0, 28, 223, 224]}}[seed]
    for world in sr.REAL_WORLDS:
        layout, _ = sr.partition(opd, "rows", world)
        assert layout.cuts == want_cuts[world]
        for nrhs in sr.NRHS:
            x, v = sr.vectors(opd, np.float64, nrhs, 100 + nrhs)
            cols = lambda a: a[:, None] if a.ndim == 1 else a
            y_ref = np.stack([bfref.mat_mul_vec(A, c) for c in cols(x).T], axis=1).reshape((opd.m,) + x.shape[1:])
            z_ref = np.stack([bfref.mat_rmul_vec(A, c) for c in cols(v).T], axis=1).reshape((opd.n,) + v.shape[1:])
            loc_y = [y_ref[layout.cuts[r]:layout.cuts[r + 1]] for r in range(world)]
            loc_z = [dense[layout.cuts[r]:layout.cuts[r + 1]].T @ sr.gather_rows(layout, r, "rows", v) for r in range(world)]
            y, z = _assemble(layout, "rows", loc_y, loc_z)
            assert sr.rel(y, y_ref) <= TOL and sr.rel(z, z_ref) <= TOL, (seed, world, nrhs)


@pytest.mark.parametrize("world", sr.REAL_WORLDS)
def test_assembly_of_real_interleaved_block_rows_is_the_oracles_whole_product(world):
    """The real 6-block-row operand dealt so that no rank owns one run: each shard is its own oracle graph."""
    import randgraph
    from oracle import bfref
    opd = sr.real_block_rows_operand()
    A = bfref.from_desc(opd.desc, opd.vals)
    layout, shards = sr.partition(opd, "rowblocks", world, owner=sr.REAL_BLOCK_OWNERS[world])
    local = [bfref.from_desc(opd.desc, opd.vals, root=sh["root"]) for sh in shards]
    cols = lambda a: a[:, None] if a.ndim == 1 else a
    mul = lambda f, B, a, rows: np.stack([f(B, c) for c in cols(a).T], axis=1).reshape((rows,) + a.shape[1:])
    for nrhs in sr.NRHS:
        x, v = sr.vectors(opd, np.float64, nrhs, 100 + nrhs)
        loc_y = [mul(bfref.mat_mul_vec, local[r], x, layout.rows_of[r]) for r in range(world)]
        loc_z = [mul(bfref.mat_rmul_vec, local[r], sr.gather_rows(layout, r, "rowblocks", v), opd.n) for r in range(world)]
        y, z = _assemble(layout, "rowblocks", loc_y, loc_z)
        dense = randgraph.densify(opd.desc, opd.vals, opd.root)
        assert sr.rel(y, mul(bfref.mat_mul_vec, A, x, opd.m)) <= TOL and sr.rel(z, mul(bfref.mat_rmul_vec, A, v, opd.n)) <= TOL, (world, nrhs)
        assert sr.rel(y, dense @ x) <= TOL and sr.rel(z, dense.T @ v) <= TOL, (world, nrhs)


def test_sums_are_taken_in_the_storage_type_and_in_order():
    """The assembly's additions are float32 additions for float32 / complex64 parts, left to right."""
    a, b, c = (np.array([v], dtype=np.float32) for v in (1.0, 2.0 ** -24, 2.0 ** -24))
    assert sr.rank_order_sum([a, b, c])[0] == np.float32(1.0)                 # (1 + 2^-24) + 2^-24 in float32: both halves-ulp round away
    assert sr.rank_order_sum([b, c, a])[0] == np.float32(1.0) + np.float32(2.0 ** -23)
    z = sr.rank_order_sum([(a + 1j * b).astype(np.complex64), (b + 1j * a).astype(np.complex64)])
    assert z.dtype == np.complex64 and z[0] == np.complex64(1 + 1j)
    assert not sr.same_bits(np.zeros(1), -np.zeros(1)) and not sr.same_bits(np.zeros(1, np.float32), np.zeros(1))


def test_the_collective_stand_in_compiles_without_warnings(tmp_path):
    assert os.path.exists(sr.compile_stub(tmp_path, shared=False))


_PROBE = """
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from butterfly_amd import _capi
lib = _capi.load()
ident = C.create_string_buffer(128)
rc = lib.bfhipCommGetUniqueId(ident)
print(rc)
print(lib.bfhipLastErrorMessage().decode() if rc else ident.raw.split(b"\\0")[0].decode())
"""


def _probe(path):
    env = dict(os.environ, BFHIP_RCCL_LIBRARY=path)
    p = subprocess.run([sys.executable, "-c", _PROBE, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr                              # an error code, not a crash
    rc, msg = p.stdout.strip().split("\n")[-2:]
    return int(rc), msg


def test_a_named_collective_library_is_the_only_one_tried(tmp_path):
    missing = str(tmp_path / "no_such_librccl.so")
    rc, msg = _probe(missing)
    assert rc == 2 and missing in msg and "BFHIP_RCCL_LIBRARY" in msg         # BF_ERROR_RUNTIME_ERROR naming the path; no fallback to librccl
    hollow = str(tmp_path / "libhollow.so")                                   # loads, but exports none of the seven symbols
    (tmp_path / "hollow.c").write_text("int hollow_nothing;\n")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", hollow, str(tmp_path / "hollow.c")])
    rc, msg = _probe(hollow)
    assert rc == 2 and hollow in msg and "lacks ncclGetUniqueId" in msg
    rc, msg = _probe(sr.compile_stub(tmp_path))
    assert rc == 0 and msg.startswith("stub-ccl:")                            # the stand-in's id: it is the library in use
