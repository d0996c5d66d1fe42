"""Writes tests/golden/helm2_eval_mp.npz: the truth of every case of tests/helm2_eval_cases.py, by mpmath at 50 digits.

    python tests/golden/make_helm2_eval_golden.py

Axis cases: J0, Y0, J1, Y1 at every designed argument ("axis/x", "axis/<fn>_hi" float64 + "axis/<fn>_lo" float32); every
axis entry is one of them times a power of two, so the tests assemble the entries exactly.
Geometry matrices, per name of helm2_eval_cases.geom_matrix_names(): the float64 inputs ("<name>/src", "/tgt": points;
"/nrm": the normals the dipole term uses; "/f", "/w": KR factors and column weights), the truth as "/hi" (complex128)
+ "/lo" (complex64), and "/unit" = the error unit's (scale, kr) (float32: they only scale a bound).
The truth is the exact value of the formula at the float64 inputs: nothing of it is rounded before the last step."""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import helm2_eval_cases as cat  # noqa: E402

mp.mp.dps = 50


def split(v):
    """hi (float64, nearest) and lo (float32) of an mpf."""
    hi = float(v)
    return hi, np.float32(float(v - mp.mpf(hi)))


def axis_truth(x):
    fns = {"j0": lambda t: mp.besselj(0, t), "y0": lambda t: mp.bessely(0, t), "j1": lambda t: mp.besselj(1, t), "y1": lambda t: mp.bessely(1, t)}
    return {name: [split(fn(mp.mpf(float(t)))) for t in x] for name, fn in fns.items()}


def entry_truth(o, i, j):
    """(value, scale, kr) of entry (i, j) of the operands `o` as mpf / mpc: the formula of bfKernelEntry, exactly."""
    if o["self_mask"][i, j]:
        return mp.mpc(o["self_value"].real, o["self_value"].imag), mp.mpf(0), mp.mpf(0)
    g = lambda key: mp.mpf(float(o[key][i, j]))
    dx, dy = g("tx") - g("sx"), g("ty") - g("sy")
    r = mp.sqrt(dx * dx + dy * dy)
    if r == 0:
        return mp.mpc(0), mp.mpf(0), mp.mpf(0)
    k = mp.mpf(o["k"])
    kr = k * r
    fw = g("f") * g("w")
    al, be = mp.mpc(o["alpha"].real, o["alpha"].imag), mp.mpc(o["beta"].real, o["beta"].imag)
    z, scale = mp.mpc(0), mp.mpf(0)
    if al != 0:
        h0 = mp.besselj(0, kr) + 1j * mp.bessely(0, kr)
        z += al * (0.25j * h0)
        scale += abs(al) * abs(h0) / 4
    if be != 0:
        h1 = mp.besselj(1, kr) + 1j * mp.bessely(1, kr)
        nx, ny = g("nx"), g("ny")
        z += be * (0.25j * k * h1 * (nx * dx + ny * dy) / r)
        scale += abs(be) * k * abs(h1) * (abs(nx * dx) + abs(ny * dy)) / (4 * r)
    return z * fw, abs(fw) * scale, kr


def matrix_truth(o):
    m, n = o["f"].shape
    hi, lo = np.zeros((m, n), dtype=np.complex128), np.zeros((m, n), dtype=np.complex64)
    unit = np.zeros((2, m, n), dtype=np.float32)
    for i in range(m):
        for j in range(n):
            z, scale, kr = entry_truth(o, i, j)
            (rh, rl), (ih, il) = split(z.real), split(z.imag)
            hi[i, j], lo[i, j] = complex(rh, ih), complex(rl, il)
            unit[0, i, j], unit[1, i, j] = np.float32(float(scale)), np.float32(float(kr))
    return dict(hi=hi, lo=lo, unit=unit)


def main():
    out = {}
    x = cat.axis_arguments()
    out["axis/x"] = x
    for name, vals in axis_truth(x).items():
        out[f"axis/{name}_hi"] = np.array([v[0] for v in vals], dtype=np.float64)
        out[f"axis/{name}_lo"] = np.array([v[1] for v in vals], dtype=np.float32)
    for name in cat.geom_matrix_names():
        o = cat.geom_operands(name)
        for key, arr in {**cat.matrix_inputs(o), **matrix_truth(o)}.items():
            out[f"{name}/{key}"] = arr
        print(name, o["f"].shape, flush=True)
    np.savez_compressed(cat.FIXTURE, **out)
    print(cat.FIXTURE, os.path.getsize(cat.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
