"""Complex64 against complex128 on the headline operand: the fac_helm2 multilevel layout bench.py --workload helm2 uses
(equispaced points of the unit circle, k = N/16, the native C layout, synthetic values of seed 1234), compiled twice in one
process -- as complex128 and with demoteToF32 as complex64 -- and applied alternately.

    python tools/c64_rate.py --n 262144 --out profiles/r6_c64_n262144.json

Per operator: the median of `--steps` timed applies (hipEvents on the apply stream, the two operators alternating after
`--warmup` applies each), matvec/s, the algorithmic bytes of an apply (leaf bytes + element size x the vector elements each
stage reads and writes) and their rate as a fraction of 8 TB/s; and the rel-l2 of the complex64 result against the complex128
one on the same seeded x.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_BPS = 8.0e12      # MI355X HBM3E peak (MI355X_MICROARCH.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.operator import HipOperator
    if not torch.cuda.is_available():
        raise SystemExit("c64_rate.py measures on a GPU; none is visible")
    n = args.n
    desc, perm = hs.native_multilevel_structure(hs.circle_points(n), n / 16.0)
    ops = {"c128": HipOperator.from_desc(desc, None, seed=args.seed, device=0),
           "c64": HipOperator.from_desc(desc, None, seed=args.seed, device=0, demote_to_f32=True)}
    rng = np.random.default_rng(args.seed)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    xs = {"c128": torch.from_numpy(x).to("cuda:0"), "c64": torch.from_numpy(x.astype(np.complex64)).to("cuda:0")}
    ys = {}
    for name, op in ops.items():
        for _ in range(args.warmup):
            ys[name] = op.apply_device(xs[name])
    torch.cuda.synchronize()
    err = float(np.linalg.norm(ys["c64"].cpu().numpy().astype(np.complex128) - ys["c128"].cpu().numpy()) /
                np.linalg.norm(ys["c128"].cpu().numpy()))
    times = {name: [] for name in ops}
    stream = torch.cuda.current_stream()
    for _ in range(args.steps):
        for name, op in ops.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(stream)
            op.apply_device(xs[name])
            e.record(stream)
            e.synchronize()
            times[name].append(s.elapsed_time(e))
    out = {"n": n, "k": n / 16.0, "seed": args.seed, "steps": args.steps, "warmup": args.warmup,
           "rel_l2_c64_vs_c128": err, "operators": {}}
    for name, op in ops.items():
        st = op.stats()
        es = 16 if name == "c128" else 8
        alg_bytes = int(st["leafBytes"]) + es * (int(st["vecElemsRead"]) + int(st["vecElemsWritten"]))
        med = float(np.median(times[name]))
        out["operators"][name] = {"dtype": int(st["dtype"]), "median_ms": med, "min_ms": float(np.min(times[name])),
                                  "max_ms": float(np.max(times[name])), "matvec_per_s": 1e3 / med,
                                  "leaf_bytes": int(st["leafBytes"]), "arena_bytes": int(st["arenaBytes"]),
                                  "algorithmic_bytes": alg_bytes, "fraction_of_8TBps": alg_bytes / (med * 1e-3) / HBM_PEAK_BPS}
    out["speedup_c64_over_c128"] = out["operators"]["c64"]["matvec_per_s"] / out["operators"]["c128"]["matvec_per_s"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for op in ops.values():
        op.close()


if __name__ == "__main__":
    main()
