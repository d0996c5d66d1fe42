"""Test infrastructure: digests of compiled plans, and the operands they are taken of.

digest(op) is a SHA-256 over everything the inspection C-ABI shows of a BFHIP_FLAG_PLAN_ONLY operator's plans, the adjoint
plan included.  tests/test_plan_fingerprint_cpu.py holds the planner to the digests in tests/golden/plan_fingerprints.json:
a change to bfhip_plan.c that alters a plan it did not mean to alter shows there, operand by operand.

The goldens are recorded from the commit BEFORE the change under test, never from the code under test:

    BFHIP_LIB_PATH=<libbfhip.so built from that commit> python tests/plan_fingerprint.py <commit id> [output of that commit's plan_oom]

rewrites the file (the second argument: what tests/native/plan_oom.c printed when linked against that commit's bfhip_plan.c;
without it the native digests already in the file are kept)."""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "plan_fingerprints.json")
NRHS = (1, 2, 17, 64)


def _struct_fields(h, s):
    for name, _ in s._fields_:
        v = getattr(s, name)
        if name not in ("structSize", "items", "pieces", "bundleBegin", "rowInterval", "ivBegin", "srcBias"):      # sizes of the caller's structs, addresses
            h.update(f"{name}={int(v)};".encode())


def _kernels(h, op):
    for nrhs in NRHS:
        h.update(f"nrhs{nrhs}:{op.stage_kernels(nrhs)};".encode())


def digest(op):
    """op: a HipOperator compiled with FLAG_PLAN_ONLY.  The three right-hand-side-block switches are left ON."""
    from butterfly_amd import _capi
    from plan_emulator import _view
    lib = _capi.load()
    h = hashlib.sha256()
    info = _capi.BfhipPlanInfo()
    info.structSize = C.sizeof(info)
    _capi.check(lib.bfhipPlanGetInfo(op.handle, C.byref(info)))
    _struct_fields(h, info)
    st = _capi.BfhipStats()
    st.structSize = C.sizeof(st)
    _capi.check(lib.bfhipGetStats(op.handle, C.byref(st)))
    _struct_fields(h, st)
    for s in range(int(info.numStages) + int(info.numStagesT)):
        sv = _capi.BfhipStageView()
        sv.structSize = C.sizeof(sv)
        _capi.check(lib.bfhipPlanGetStage(op.handle, s, C.byref(sv)))
        _struct_fields(h, sv)
        h.update(_view(sv.items, int(sv.numItems), _capi.ITEM_DTYPE).tobytes())
        h.update(_view(sv.pieces, int(sv.numPieces), _capi.PIECE_DTYPE).tobytes())
        h.update(b"bundles" if sv.bundleBegin else b"none")
        if sv.bundleBegin:
            h.update(_view(sv.bundleBegin, int(sv.numBundles) + 1, np.dtype("<u4")).tobytes())
        for r in range(int(sv.numReduce)):
            rv = _capi.BfhipReduceView()
            rv.structSize = C.sizeof(rv)
            _capi.check(lib.bfhipPlanGetReduce(op.handle, s, r, C.byref(rv)))
            _struct_fields(h, rv)
            h.update(_view(rv.rowInterval, int(rv.numRows), np.dtype("<u4")).tobytes())
            h.update(_view(rv.ivBegin, int(rv.numIntervals) + 1, np.dtype("<u4")).tobytes())
            h.update(_view(rv.srcBias, int(rv.numSrc), np.dtype("<i8")).tobytes())
    # which kernels an apply launches: switches off, then every switch the operator accepts on
    _kernels(h, op)
    for setter in (op.set_rhs_blocks, op.set_real_rhs_blocks, op.set_adjoint_rhs_blocks):
        try:
            setter(2)
            h.update(b"on;")
        except _capi.BfhipError:
            h.update(b"refused;")
    _kernels(h, op)
    # the packed leaves pin where every piece's values come from (pieceSrc)
    dt = {0: np.complex128, 1: np.float64, 2: np.float32, 3: np.complex64}[info.dtype]
    arena = np.zeros(int(info.arenaElems), dtype=dt)
    _capi.check(lib.bfhipPlanPackArena(op.handle, arena.ctypes.data))
    h.update(arena.tobytes())
    if int(info.reserved) == 1:           # packed adjoint: an arena of its own
        arena_t = np.zeros(int(info.arenaElemsT), dtype=dt)
        _capi.check(lib.bfhipPlanPackArenaT(op.handle, arena_t.ctypes.data))
        h.update(arena_t.tobytes())
    return h.hexdigest()


def _compiled(desc, vals, variants):
    """{variant name: digest}; variants: (name, HipOperator.from_desc keywords)"""
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    out = {}
    for name, kw in variants:
        kw = dict(kw)
        kw["flags"] = kw.get("flags", 0) | _capi.FLAG_PLAN_ONLY
        assert name not in out, name
        try:
            op = HipOperator.from_desc(desc, vals, **kw)
        except _capi.BfhipError as e:       # a compile the library refuses is part of its behaviour too
            out[name] = f"refused: {e}"
            continue
        out[name] = digest(op)
        op.close()
    return out


def _partition(desc, world):
    from butterfly_amd import _capi
    cuts = np.zeros(world + 1, dtype=np.uint64)
    loads = np.zeros(world, dtype=np.uint64)
    da = _capi.DescArrays(desc)
    rc = _capi.load().bfhipRowPartition(da.byref(), world, cuts.ctypes.data, loads.ctypes.data)
    return None if rc else [int(c) for c in cuts]


# ---- the operands: name -> function of conftest's helm2_case (or the fixture's getter) returning {variant: digest} ------------------------------------------------------------
def _catalogue(case, dtype):
    def run(helm2_case=None):
        import kernel_catalogue as kc
        desc, vals, demote = kc.materialize(case, dtype)
        return _compiled(desc, vals, [(f"flags{f}", dict(flags=f, demote_to_f32=demote)) for f in [0] + kc.flag_sets(case, dtype)])
    return run


def _random_graph(seed, cplx):
    def run(helm2_case=None):
        from butterfly_amd import _capi
        import randgraph
        if cplx:          # test_random_nested_complex_graphs
            rng = np.random.default_rng(2000 + seed)
            desc, vals = randgraph.random_operand(rng, depth=3, size_hint=int(rng.integers(20, 400)), cplx=True)
        else:             # test_random_nested_real_graphs
            rng = np.random.default_rng(1000 + seed)
            desc, vals = randgraph.random_real_operand(rng, depth=int(rng.integers(1, 5)), size_hint=int(rng.integers(8, 200)))
        return _compiled(desc, vals, [(f"{a}-rhs{r}", dict(flags=f, max_rhs=r))
                                      for a, f in (("plain", 0), ("adjoint", _capi.FLAG_ADJOINT), ("packed", _capi.FLAG_ADJOINT_PACKED)) for r in (1, 64)])
    return run


def _row_ranges(seed):
    def run(helm2_case=None):       # the operands and ranges of test_row_ranges_of_random_nested_graphs (the same draws in the same order)
        from butterfly_amd import _capi
        import randgraph
        rng = np.random.default_rng(4200 + seed)
        cplx = seed % 2 == 1
        desc, vals = randgraph.random_operand(rng, depth=int(rng.integers(2, 5)), size_hint=int(rng.integers(60, 220)), cplx=cplx)
        m, n = desc.rows[desc.root], desc.cols[desc.root]
        rng.standard_normal(n)
        if cplx:
            rng.standard_normal(n)
        variants = []
        for demote in ((False,) if cplx else (False, True)):
            ranges = []
            for _ in range(4):
                a = int(rng.integers(0, m))
                ranges.append((a, int(rng.integers(a + 1, m + 1))))
            for world in (2, 3):
                cuts = _partition(desc, world)
                if cuts:
                    ranges += [(cuts[r], cuts[r + 1]) for r in range(world)]
            for i, rg in enumerate(ranges):
                for a, f in (("plain", 0), ("adjoint", _capi.FLAG_ADJOINT)):
                    variants.append((f"demote{int(demote)}-{i}-rows{rg[0]}_{rg[1]}-{a}", dict(flags=f, demote_to_f32=demote, row_range=rg)))
        return _compiled(desc, vals, variants)
    return run


def _helm2(n, k):
    def run(helm2_case):
        from butterfly_amd import _capi
        desc, tp, vals = helm2_case(n, k)
        adj = _capi.FLAG_ADJOINT
        variants = [("rhs1", dict(flags=adj)), ("rhs64", dict(flags=adj, max_rhs=64)), ("demote", dict(flags=adj, demote_to_f32=True)),
                    ("packed", dict(flags=_capi.FLAG_ADJOINT_PACKED)), ("row_blocks1_3", dict(flags=adj, row_blocks=(1, 3)))]
        cuts = _partition(desc, 3)
        variants += [(f"rank{r}of3", dict(flags=adj, row_range=(cuts[r], cuts[r + 1]))) for r in range(3)]
        variants.append(("unclean_range", dict(flags=adj, row_range=(3, n - 5))))
        return _compiled(desc, vals, variants)
    return run


def _streamer(helm2_case=None):
    from butterfly_amd import _capi
    from test_streamer_structure import sphere_fixture_case      # 500 mesh vertices x 32 eigenvectors: the size its own tests stream
    st, phi, A, desc, vals = sphere_fixture_case()
    return _compiled(desc, vals, [(f"{a}-demote{int(d)}", dict(flags=f, demote_to_f32=d))
                                  for a, f in (("shared", _capi.FLAG_ADJOINT), ("packed", _capi.FLAG_ADJOINT_PACKED)) for d in (False, True)])


def operands():
    import kernel_catalogue as kc
    out = {}
    for case in kc.CASES:
        for dt in kc.DTYPES:
            out[f"catalogue-{case.name}-{kc.DTYPE_NAMES[dt]}"] = _catalogue(case, dt)
    for seed in range(12):
        out[f"random_real-{seed}"] = _random_graph(seed, False)
    for seed in range(6):
        out[f"random_complex-{seed}"] = _random_graph(seed, True)
    for seed in range(8):
        out[f"row_ranges-{seed}"] = _row_ranges(seed)
    for n, k in ((1024, 100), (2048, 128)):
        out[f"helm2-n{n}-k{k}"] = _helm2(n, k)
    out["streamer-sphere500x32"] = _streamer
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    from conftest import helm2_case
    old = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    native = old.get("native", {})
    if len(sys.argv) > 2:
        native = {ln.split()[1]: ln.split()[2] for ln in open(sys.argv[2]) if ln.startswith("digest ")}
    gold = {"recorded_from": sys.argv[1], "numpy": np.__version__, "plans": {name: run(helm2_case) for name, run in operands().items()}, "native": native}
    with open(GOLDEN, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(gold['plans'])} operands, {sum(len(v) for v in gold['plans'].values())} plans, {len(native)} native digests -> {GOLDEN}")
