"""Case catalogue for the Helmholtz kernel-evaluation tests (bfEvalKernel / bfHelm2DenseKernel).

Plain numpy, no device.  Every input is given in closed form, so the committed fixture
(tests/golden/helm2_eval_mp.npz, written by tests/golden/make_helm2_eval_golden.py with mpmath at 50 digits) can be
checked against this file bit for bit.  Also here: the float64 restatement of bfKernelEntry the device is measured
against.  It calls the host C library's j0/y0/j1/y1 (what the reference calls, src/bessel.c), not scipy's, and carries
its own copy of the Kapur-Rokhlin tables: a deliberate duplicate of bfKrWeights (bfhip_build.hip) and of
oracle/helm2_build.py, so that a slip in one copy does not pass unseen.

Error unit.  For entry (i, j), f the KR factor and w the column weight (1 where absent),
    scale = f w [ |alpha| |H0(kr)| / 4 + |beta| k |H1(kr)| (|n_x dx| + |n_y dy|) / (4 r) ]
    err   = |got - truth| / (u (1 + kr) scale),   u = 2^-53,
with the terms the potential has (S: alpha = 1, beta = 0; S', D: alpha = 0, beta = 1).  |n_x dx| + |n_y dy| instead of
|n.d| lets the unit see the cancellation in n.d between neighbours on a smooth curve; 1 + kr is the conditioning of H
with respect to the roundings of k * hypot(dx, dy), which no float64 formula avoids.  On the axis cases kr is exact and
the factor is dropped."""
import ctypes
import math
import os

import numpy as np

U = 2.0 ** -53
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "helm2_eval_mp.npz")

# Kapur & Rokhlin, SIAM J. Numer. Anal. 34 (1997), Tables 6: gamma_1..gamma_p of orders 2, 6, 10 (second copy, see above)
KR_WEIGHTS = {
    2: [1.825748064736159e+00, -1.325748064736159e+00],
    6: [4.967362978287758e+00, -1.620501504859126e+01, 2.585153761832639e+01, -2.222599466791883e+01, 9.930104998037539e+00,
        -1.817995878141594e+00],
    10: [7.832432020568779e+00, -4.565161670374749e+01, 1.452168846354677e+02, -2.901348302886379e+02, 3.870862162579900e+02,
         -3.523821383570681e+02, 2.172421547519342e+02, -8.707796087382991e+01, 2.053584266072635e+01, -2.166984103403823e+00],
}
# the order-10 table as the reference prints it (src/quadrature.c:29-40): the decimal exponents are lost
KR10_AS_PRINTED = [7.832432020568779, -4.565161670374749, 1.452168846354677, -2.901348302886379, 3.870862162579900,
                   -3.523821383570681, 2.172421547519342, -8.707796087382991, 2.053584266072635, -2.166984103403823]

_libm = ctypes.CDLL("libm.so.6")
_BESSEL = {}
for _name in ("j0", "y0", "j1", "y1"):
    _fn = getattr(_libm, _name)
    _fn.restype, _fn.argtypes = ctypes.c_double, [ctypes.c_double]
    _BESSEL[_name] = np.frompyfunc(_fn, 1, 1)


def bessel(name, x):
    """The host C library's j0 / y0 / j1 / y1 on an array."""
    return _BESSEL[name](np.asarray(x, dtype=np.float64)).astype(np.float64)


# --------------------------------------------------------------------------
# axis cases: one source at the origin, targets on the axes, k a power of two
# --------------------------------------------------------------------------
# nearest doubles to the first five positive zeros of J0, Y0, J1, Y1 (Abramowitz & Stegun, Table 9.5)
BESSEL_ZEROS = {
    "j0": [2.404825557695773, 5.520078110286311, 8.653727912911013, 11.791534439014281, 14.930917708487787],
    "y0": [0.8935769662791675, 3.957678419314858, 7.086051060301773, 10.222345043496418, 13.361097473872764],
    "j1": [3.8317059702075125, 7.015586669815619, 10.173468135062722, 13.323691936314223, 16.470630050877634],
    "y1": [2.197141326031017, 5.429681040794135, 8.596005868331169, 11.749154830839881, 14.897442128336726],
}
AXIS_LARGE = [1000.5, 8191.75, 99999.125, 1048575.5]
AXIS_WAVENUMBERS = (1.0, 32.0)


def axis_arguments():
    """The designed arguments x, ascending and distinct (527: the lists overlap)."""
    xs = [2.0 ** (j / 8.0) for j in range(-80, 161)]
    xs += [2.0 ** j for j in range(-40, -10)]
    xs += [0.25 * j for j in range(1, 241)]
    for name in ("j0", "y0", "j1", "y1"):
        xs += BESSEL_ZEROS[name]
    xs += AXIS_LARGE
    return np.unique(np.asarray(xs, dtype=np.float64))


AXIS_DIRECTIONS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0))          # targets (x, 0), (0, x), (-x, 0): blocks of the leaf's rows
# leaf name -> (layer_pot, the one normal every point carries)
AXIS_LEAVES = {"S": ("S", (1.0, 0.0)), "Sp_x": ("Sp", (1.0, 0.0)), "Sp_y": ("Sp", (0.0, 1.0)), "D_x": ("D", (1.0, 0.0))}


def axis_problem(k):
    """(points, recipe): point 0 is the origin, then the targets of the three directions, all divided by k (a power of
    two: exact), so that k * hypot(dx, dy) is the designed argument exactly."""
    x = axis_arguments()
    pts = [np.zeros((1, 2))] + [np.stack([d[0] * x, d[1] * x], axis=1) / k for d in AXIS_DIRECTIONS]
    pts = np.concatenate(pts) + 0.0                                # + 0.0: no negative zeros
    return pts, ("kernel", ("node", 0, 1), ("node", 1, len(pts)))


def axis_normals(leaf, npts):
    return np.tile(np.asarray(AXIS_LEAVES[leaf][1]), (npts, 1))


def axis_dot_signs(leaf):
    """n.d / x per direction block: what the S' / D entries of that block are multiplied by (S: 1)."""
    pot, nrm = AXIS_LEAVES[leaf]
    return [1.0 if pot == "S" else nrm[0] * d[0] + nrm[1] * d[1] for d in AXIS_DIRECTIONS]


def axis_decades(x):
    return np.floor(np.log10(x)).astype(int)


# --------------------------------------------------------------------------
# geometry cases: a kite of 40 points in a permuted (tree) order
# --------------------------------------------------------------------------
GEOM_N, GEOM_K = 40, 16.0
GEOM_SELF = 0.5 - 0.25j
GEOM_ALPHA, GEOM_BETA = 0.5 - 1.0j, 2.0 + 0.25j
POTENTIALS = ("S", "Sp", "D", "combined")
KR_ORDERS = (2, 6, 10)


def kite(t):
    """Points and unit (outward) normals of the kite (cos t + 0.65 cos 2t - 0.65, 1.5 sin t) / 1.5."""
    t = np.asarray(t, dtype=np.float64)
    pts = np.stack([np.cos(t) + 0.65 * np.cos(2 * t) - 0.65, 1.5 * np.sin(t)], axis=1) / 1.5
    tx, ty = -np.sin(t) - 1.3 * np.sin(2 * t), 1.5 * np.cos(t)
    nrm = np.stack([ty, -tx], axis=1) / np.hypot(tx, ty)[:, None]
    return pts, nrm


def geom_curve():
    """points, normals (tree order), orig_index, col_weights: tree position i holds curve point (7 i + 3) % 40."""
    i = np.arange(GEOM_N)
    orig = (7 * i + 3) % GEOM_N
    pts, nrm = kite(2.0 * math.pi * orig / GEOM_N)
    w = 0.5 + ((37 * i * i + 11 * i) % 64) / 64.0
    return pts, nrm, orig.astype(np.uint64), w


def geom_targets():
    """12 separate targets with their normals, on a small ellipse beside the kite."""
    t = 2.0 * math.pi * (np.arange(12) + 0.25) / 12
    pts = np.stack([1.1 + 0.3 * np.cos(t), 0.2 + 0.2 * np.sin(t)], axis=1)
    nx, ny = 0.2 * np.cos(t), 0.3 * np.sin(t)
    return pts, np.stack([nx, ny], axis=1) / np.hypot(nx, ny)[:, None]


TGT_RANGE, SRC_RANGE = (9, 17), (12, 29)               # overlap [12, 17): five self entries inside the leaf; tree positions
# 11 and 28 hold curve points 0 and 39, so the Kapur-Rokhlin distance wraps around at d = 1
CIRCLE_SRC = ("circle", 0.125, -0.0625, 0.1875, 10)
CIRCLE_TGT = ("circle", -1.25, 0.5, 0.25, 10)
REEXP = ("reexp", ("node", 0, 12), ("node", 20, 32), ("node", 24, 40))      # source, equivalent sources, check points


def geom_cases():
    """name -> dict(pot, recipe, deco): deco the keyword arguments of helm2_build_leaf beyond the potential's own.
    The re-expansion cases are in geom_reexp_cases()."""
    node = ("kernel", ("node",) + SRC_RANGE, ("node",) + TGT_RANGE)
    cases = {}
    for pot in POTENTIALS:
        cases[f"{pot}/node_plain"] = dict(pot=pot, recipe=node, deco={})
        for p in KR_ORDERS:
            cases[f"{pot}/node_kr{p}"] = dict(pot=pot, recipe=node, deco=dict(weights=True, self_value=GEOM_SELF, kr_order=p))
        cases[f"{pot}/circle_to_node"] = dict(pot=pot, recipe=("kernel", CIRCLE_SRC, ("node",) + TGT_RANGE), deco=dict(weights=True))
        if pot != "Sp":
            cases[f"{pot}/node_to_circle"] = dict(pot=pot, recipe=("kernel", ("node",) + SRC_RANGE, CIRCLE_TGT), deco=dict(weights=True))
        cases[f"{pot}/node_to_tnode"] = dict(pot=pot, recipe=("kernel", ("node",) + SRC_RANGE, ("tnode", 0, 12)),
                                             deco=dict(weights=True, tgt=True))
    return cases


def geom_reexp_cases():
    """name -> dict(pot, recipe, deco) per proxy potential, and the two kernel matrices each one is made of:
    "<name>/z_equiv" (decorate = 0: no weights, zeros where a check point is an equivalent source) and
    "<name>/z_orig" (column weights)."""
    return {f"{pot}/reexp": dict(pot=pot, recipe=REEXP, deco=dict(weights=True, self_value=GEOM_SELF)) for pot in ("S", "D", "combined")}


def problem_kwargs(pot, deco):
    """The keyword arguments of helm2_build_leaf / Helm2Problem for a geometry case."""
    pts, nrm, orig, w = geom_curve()
    kw = dict(layer_pot=pot)
    if pot != "S":
        kw["normals"] = nrm
    if pot == "combined":
        kw.update(alpha=GEOM_ALPHA, beta=GEOM_BETA)
    if deco.get("weights"):
        kw["col_weights"] = w
    if deco.get("self_value"):
        kw["self_value"] = deco["self_value"]
    if deco.get("kr_order"):
        kw.update(kr_order=deco["kr_order"], orig_index=orig)
    if deco.get("tgt"):
        tp, tn = geom_targets()
        kw.update(tgt_points=tp, tgt_normals=tn)
    return kw


# --------------------------------------------------------------------------
# the operands of one kernel matrix, and its float64 restatement
# --------------------------------------------------------------------------
TWO_PI = 6.283185307179586


def sample_circle(spec):
    """bfPoint / bfNormal for a sampled circle (bfCircle2SamplePoints, src/circle.c:12-35): points and radial normals."""
    _, cx, cy, r, count = spec
    theta = (TWO_PI / float(count)) * np.arange(count, dtype=np.float64)
    return np.stack([r * np.cos(theta) + cx, r * np.sin(theta) + cy], axis=1), np.stack([np.cos(theta), np.sin(theta)], axis=1)


def kr_factors(order, orig_tgt, orig_src, n, table=None):
    """1 + w[d - 1] where the original indices are d = 1..order apart on the closed curve of n points, else 1."""
    fwd = (np.asarray(orig_tgt, dtype=np.int64)[:, None] - np.asarray(orig_src, dtype=np.int64)[None, :]) % n
    d = np.minimum(fwd, n - fwd)
    f = np.ones(d.shape)
    w = KR_WEIGHTS[order] if table is None else table
    for p in range(order):
        f[d == p + 1] += w[p]
    return f


def operands(pot, src_spec, tgt_spec, decorate, points, normals=None, col_weights=None, self_value=0.0, kr_order=0,
             orig_index=None, alpha=0.0, beta=0.0, tgt_points=None, tgt_normals=None, k=None):
    """What bfKernelEntry reads for the matrix `src_spec` -> `tgt_spec` of potential `pot`, as float64 arrays:
    dict(k, sx, sy, tx, ty, nx, ny, f, w, self_mask, self_value, alpha, beta); nx, ny is the normal the dipole term uses
    (target normals for S', source normals for D and the combined field), f the KR factor, w the column weight."""
    def resolve(spec):
        if spec[0] == "circle":
            return sample_circle(spec)
        base, nb = (points, normals) if spec[0] == "node" else (tgt_points, tgt_normals)
        sl = slice(spec[1], spec[2])
        return np.asarray(base)[sl], None if nb is None else np.asarray(nb)[sl]
    (sp, sn), (tp, tn) = resolve(src_spec), resolve(tgt_spec)
    m, n = len(tp), len(sp)
    o = dict(k=float(k), alpha=complex(alpha), beta=complex(beta), self_value=complex(self_value))
    if pot == "S":
        o["alpha"], o["beta"] = 1.0 + 0j, 0j
    elif pot in ("Sp", "D"):
        o["alpha"], o["beta"] = 0j, 1.0 + 0j
    o["sx"], o["sy"] = np.broadcast_to(sp[None, :, 0], (m, n)), np.broadcast_to(sp[None, :, 1], (m, n))
    o["tx"], o["ty"] = np.broadcast_to(tp[:, None, 0], (m, n)), np.broadcast_to(tp[:, None, 1], (m, n))
    if pot == "S":
        o["nx"] = o["ny"] = np.zeros((m, n))
    elif pot == "Sp":
        o["nx"], o["ny"] = np.broadcast_to(tn[:, None, 0], (m, n)), np.broadcast_to(tn[:, None, 1], (m, n))
    else:
        o["nx"], o["ny"] = np.broadcast_to(sn[None, :, 0], (m, n)), np.broadcast_to(sn[None, :, 1], (m, n))
    f, w = np.ones((m, n)), np.ones((m, n))
    mask = np.zeros((m, n), dtype=bool)
    both = src_spec[0] == "node" and tgt_spec[0] == "node"
    if decorate:
        if both:
            mask = np.arange(tgt_spec[1], tgt_spec[2])[:, None] == np.arange(src_spec[1], src_spec[2])[None, :]
            if kr_order:
                f = kr_factors(kr_order, orig_index[tgt_spec[1]:tgt_spec[2]], orig_index[src_spec[1]:src_spec[2]], len(points))
        if col_weights is not None and src_spec[0] == "node":
            w = w * np.asarray(col_weights)[src_spec[1]:src_spec[2]][None, :]
    o["f"], o["w"], o["self_mask"] = f, w, mask
    return o


def restate(o):
    """bfKernelEntry in float64 with the C library's Bessel functions: the complex128 matrix of the operands `o`."""
    dx, dy = o["tx"] - o["sx"], o["ty"] - o["sy"]
    r = np.hypot(dx, dy)
    nz = r != 0
    rr = np.where(nz, r, 1.0)
    kr = o["k"] * rr
    z = np.zeros(r.shape, dtype=np.complex128)
    if o["alpha"] != 0:
        z = z + o["alpha"] * (-0.25 * bessel("y0", kr) + 1j * (0.25 * bessel("j0", kr)))
    if o["beta"] != 0:
        sc = 0.25 * o["k"] * (o["nx"] * dx + o["ny"] * dy) / rr
        z = z + o["beta"] * (-sc * bessel("y1", kr) + 1j * (sc * bessel("j1", kr)))
    z = np.where(nz, z, 0.0) * o["f"] * o["w"]
    return np.where(o["self_mask"], o["self_value"], z)


def hankel_scale(o, h0_abs, h1_abs):
    """The error unit's `scale` (module docstring) from |H0(kr)|, |H1(kr)|, and kr; entries at r == 0 get scale 0."""
    dx, dy = o["tx"] - o["sx"], o["ty"] - o["sy"]
    r = np.hypot(dx, dy)
    rr = np.where(r != 0, r, 1.0)
    s = abs(o["alpha"]) * h0_abs / 4 + abs(o["beta"]) * o["k"] * h1_abs * (np.abs(o["nx"] * dx) + np.abs(o["ny"] * dy)) / (4 * rr)
    return np.where(r != 0, np.abs(o["f"] * o["w"]) * s, 0.0), o["k"] * r


def geom_operands(name):
    """Operands of a geometry matrix: a case of geom_cases(), or "<reexp case>/z_equiv" / "/z_orig"."""
    pts = geom_curve()[0]
    if name.endswith(("/z_equiv", "/z_orig")):
        case = geom_reexp_cases()[name.rsplit("/", 1)[0]]
        src = case["recipe"][2] if name.endswith("/z_equiv") else case["recipe"][1]
        decorate = not name.endswith("/z_equiv")
        # Z_orig is decorated with the column weights; its source and check ranges are disjoint, so no self entries
        kw = problem_kwargs(case["pot"], case["deco"])
        kw.pop("layer_pot")
        return operands(case["pot"], src, case["recipe"][3], decorate, pts, k=GEOM_K, **kw)
    case = geom_cases()[name]
    kw = problem_kwargs(case["pot"], case["deco"])
    kw.pop("layer_pot")
    return operands(case["pot"], case["recipe"][1], case["recipe"][2], True, pts, k=GEOM_K, **kw)


def geom_matrix_names():
    return list(geom_cases()) + [f"{c}/{z}" for c in geom_reexp_cases() for z in ("z_equiv", "z_orig")]


def err_units(got, truth_hi, truth_lo, scale, kr, conditioned=True):
    """|got - truth| / (u (1 + kr) scale) per entry, 0 where scale == 0 and got == truth.  The difference is formed in
    long double, so the float32 tail of the truth counts."""
    LD = np.longdouble
    d = np.hypot((got.real.astype(LD) - truth_hi.real.astype(LD)) - truth_lo.real.astype(LD),
                 (got.imag.astype(LD) - truth_hi.imag.astype(LD)) - truth_lo.imag.astype(LD)).astype(np.float64)
    unit = U * ((1.0 + kr) if conditioned else 1.0) * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(unit > 0, d / unit, np.where(d == 0, 0.0, np.inf))
    return e


# --------------------------------------------------------------------------
# Kapur-Rokhlin end to end: the single layer on the unit circle
# --------------------------------------------------------------------------
KR_CIRCLE_K = 2.0
KR_CIRCLE_NS = (48, 96, 192)
# (i pi / 2) J1(2) H1^(1)(2): the eigenvalue of S on the unit circle for the density e^{i theta}, k = 2 (mpmath, 30 digits)
KR_CIRCLE_EIGENVALUE = complex(0.09696252171783994, 0.5224649285478903)


def kr_circle_problem(n):
    """points, density e^{i theta}, trapezoid weights 2 pi / n."""
    th = 2.0 * math.pi * np.arange(n) / n
    return np.stack([np.cos(th), np.sin(th)], axis=1), np.exp(1j * th), np.full(n, 2.0 * math.pi / n)


def kr_circle_error(n, order, table=None):
    """Relative error of the KR-corrected punctured trapezoid rule, by the numpy restatement."""
    pts, x, w = kr_circle_problem(n)
    o = operands("S", ("node", 0, n), ("node", 0, n), True, pts, col_weights=w, kr_order=0, k=KR_CIRCLE_K)
    a = restate(o) * kr_factors(order, np.arange(n), np.arange(n), n, table)
    return float(np.max(np.abs(a @ x - KR_CIRCLE_EIGENVALUE * x)) / abs(KR_CIRCLE_EIGENVALUE))


def observed_orders(errs):
    return [math.log2(errs[i] / errs[i + 1]) for i in range(len(errs) - 1)]


# --------------------------------------------------------------------------
# dense-apply shapes
# --------------------------------------------------------------------------
DENSE_K = 16.0
DENSE_SHAPES = {"n600_square": (600, 0), "n600_to_m300": (600, 300), "n257_square": (257, 0)}


def dense_problem(name):
    """points, normals, orig_index, col_weights, x, and (tgt_points, tgt_normals) or (None, None)."""
    n, m = DENSE_SHAPES[name]
    i = np.arange(n)
    orig = (7 * i + 3) % n                                          # 7 is coprime to 600 and to 257
    pts, nrm = kite(2.0 * math.pi * orig / n)
    w = (2.0 * math.pi / n) * (0.5 + ((37 * i * i + 11 * i) % 64) / 64.0)
    x = np.cos(3.0 * i + 0.5) + 1j * np.sin(5.0 * i - 0.25)
    tp = tn = None
    if m:
        t = 2.0 * math.pi * (np.arange(m) + 0.25) / m
        tp = np.stack([0.2 + 0.3 * np.cos(t), 0.25 * np.sin(t)], axis=1)          # inside the kite, off the curve
        tn = np.stack([np.cos(t), np.sin(t)], axis=1)
    return pts, nrm, orig.astype(np.uint64), w, x, tp, tn


# --------------------------------------------------------------------------
# the committed fixture and the errors measured against it
# --------------------------------------------------------------------------
_FIXTURE = {}


def fixture():
    """The committed truth (tests/golden/helm2_eval_mp.npz) as a dict of arrays, loaded once."""
    if not _FIXTURE:
        with np.load(FIXTURE) as z:
            _FIXTURE.update({key: z[key] for key in z.files})
    return _FIXTURE


def matrix_inputs(o):
    """The float64 inputs of a matrix as the fixture keeps them (one row / column of the broadcast operands)."""
    src = np.stack([o["sx"][0], o["sy"][0]], axis=1)
    tgt = np.stack([o["tx"][:, 0], o["ty"][:, 0]], axis=1)
    per_src = bool(np.all(o["nx"] == o["nx"][0]) and np.all(o["ny"] == o["ny"][0]))
    nrm = np.stack([o["nx"][0], o["ny"][0]], axis=1) if per_src else np.stack([o["nx"][:, 0], o["ny"][:, 0]], axis=1)
    return dict(src=np.ascontiguousarray(src), tgt=np.ascontiguousarray(tgt), nrm=np.ascontiguousarray(nrm),
                f=np.ascontiguousarray(o["f"]), w=np.ascontiguousarray(o["w"][0]))


def geom_truth(name):
    """(hi, lo, scale, kr) of a geometry matrix: hi + lo the truth (complex128 each), scale and kr in float64."""
    fx = fixture()
    unit = fx[f"{name}/unit"].astype(np.float64)
    return fx[f"{name}/hi"], fx[f"{name}/lo"].astype(np.complex128), unit[0], unit[1]


def geom_err(name, got):
    """err per entry of `got`, a float64 evaluation of the geometry matrix `name`."""
    return err_units(np.asarray(got), *geom_truth(name))


def axis_operands(leaf, k):
    pot, _ = AXIS_LEAVES[leaf]
    pts, recipe = axis_problem(k)
    return operands(pot, recipe[1], recipe[2], True, pts, normals=axis_normals(leaf, len(pts)), k=k)


def axis_blocks(leaf, k, column):
    """The N x 1 axis leaf `column` cut into its three direction blocks and normalised to -Y + i J: divided by the power
    of two the entries carry (1/4 for S, k/4 for S' and D: exact)."""
    pot, _ = AXIS_LEAVES[leaf]
    factor = 0.25 if pot == "S" else 0.25 * k
    return np.asarray(column).reshape(3, -1) / factor


def axis_errors(block, order):
    """(err of J_order, err of Y_order) per argument, in units of u |H_order(x)|, of one normalised block -Y + i J."""
    fx = fixture()
    LD = np.longdouble
    jh, jl, yh, yl = (fx[f"axis/{fn}{order}_{part}"] for fn in ("j", "y") for part in ("hi", "lo"))
    unit = U * np.hypot(jh, yh)
    ej = np.abs((block.imag.astype(LD) - jh.astype(LD)) - jl.astype(LD)).astype(np.float64) / unit
    ey = np.abs((-block.real.astype(LD) - yh.astype(LD)) - yl.astype(LD)).astype(np.float64) / unit
    return ej, ey


def decade_max(err, x):
    """{decade of x: max err}."""
    dec = axis_decades(x)
    return {int(d): float(err[dec == d].max()) for d in np.unique(dec)}
