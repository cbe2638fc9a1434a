"""Plain numpy restatement of the surface-baking stage (csrc/bake.hip), its case generators and the error model of
tests/test_bake_ref.py (CPU) and tests/test_bake.py (device).  Written from the definitions in include/mcpt.h and DESIGN.md section 27.

`rays` takes per point the three fp64 corners in device coordinates (world less the scene's centre, as build_host_scene forms tri_pos64), the
three fp32 vertex normals (as tri_shade holds them), fp32 barycentrics, the side and the two fp32 random numbers of block 0, and works in ONE
floating-point type after that: np.float64 restates the device, one rounding per operation in the device's operation order; np.longdouble is the
same formulas with 11 more bits.

Error model, as section 25's.  S is the worst |float64 restatement - longdouble restatement| over every origin, normal and (unrounded) direction
component of every case of `all_cases`, in units of 2^-52 (1 + |value|): what the formulas themselves lose in float64.  tests/test_bake_ref.py
measures it; the device is allowed S_BOUND = 4 S rounded up to a power of two, a stand-in for its sincos / sqrt / division chain.  A direction
component is rounded to fp32 on the device: it gets half an fp32 ulp of the reference on top.

    S measured on the CPU: 1.87 (family axis +x), 4 S = 7.46, so S_BOUND = 8
    the device on an MI355X: see DESIGN.md section 27
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
PI = 3.14159265358979323846
EPS24 = 2.0 ** -24
S_CPU = 1.87                                                # measured by tests/test_bake_ref.py::test_float64_slack
S_BOUND = 8.0
XI_SET = (0.0, EPS24, 0.5, 1.0 - EPS24)
SEED = 20270


def slack(x):
    """The float64 unit of the error model at value x."""
    return 2.0 ** -52 * (1.0 + np.abs(np.asarray(x, np.float64)))


def half_ulp32(x):
    """Half the spacing of fp32 at |x| (the binade of x itself, 2^-150 in the denormal range): the most that rounding x to fp32 moves it."""
    _, ex = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.ldexp(1.0, np.maximum(ex - 25, -150))


def _len(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def _ok(length):
    return (length > 0) & np.isfinite(length)


def rays(v0, v1, v2, n0, n1, n2, u, v, back, xi, T=np.float64):
    """(origin (N, 3), normal (N, 3), direction (N, 3), dead (N,) bool) in type T.  The direction is what the device rounds to fp32.  A dead
    point has the origin with its non-finite components zeroed, the normal 0 and the direction (0, 0, 1)."""
    v0, v1, v2 = (np.asarray(a, np.float64).reshape(-1, 3).astype(T) for a in (v0, v1, v2))
    n0, n1, n2 = (np.asarray(a, F32).reshape(-1, 3).astype(T) for a in (n0, n1, n2))
    u = np.asarray(u, F32).reshape(-1).astype(T)[:, None]; v = np.asarray(v, F32).reshape(-1).astype(T)[:, None]
    back = np.asarray(back).reshape(-1).astype(bool); xi = np.asarray(xi, F32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        w = (T(1.0) - u) - v
        e1 = v1 - v0; e2 = v2 - v0
        o = (v0 + u * e1) + v * e2
        n = (w * n0 + u * n1) + v * n2
        length = _len(n)
        geo = np.stack([e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2], e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0], e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]], -1)
        use_geo = ~_ok(length)
        n = np.where(use_geo[:, None], geo, n)
        length = np.where(use_geo, _len(geo), length)
        dead = ~_ok(length)
        n = n / np.where(dead, T(1.0), length)[:, None]
        n = np.where(back[:, None], -n, n)
        x0 = xi[:, 0].astype(T); z = np.sqrt(T(1.0) - x0); rad = np.sqrt(x0); th = (T(2.0) * T(PI)) * xi[:, 1].astype(T)
        sn = np.sin(th); cs = np.cos(th)
        s = np.copysign(T(1.0), n[:, 2]); a = T(-1.0) / (s + n[:, 2]); b = (n[:, 0] * n[:, 1]) * a
        t = np.stack([T(1.0) + s * ((n[:, 0] * n[:, 0]) * a), s * b, -s * n[:, 0]], -1)
        bt = np.stack([b, s + (n[:, 1] * n[:, 1]) * a, -n[:, 1]], -1)
        rc = (rad * cs)[:, None]; rs = (rad * sn)[:, None]
        d = (rc * t + rs * bt) + z[:, None] * n
    o = np.where(dead[:, None], np.where(np.isfinite(o), o, T(0.0)), o)
    n = np.where(dead[:, None], T(0.0), n)
    d = np.where(dead[:, None], np.array([0.0, 0.0, 1.0]).astype(T)[None], d)
    return o, n, d, dead


# ------------------------------------------------------------------------------------------------------------------------ cases
# (u, v) of a point family: the three corners, the three edges' midpoints, the centroid and a point 2^-24 off corner 0
UV_SET = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (1.0 / 3.0, 1.0 / 3.0), (EPS24, EPS24))


def _unit(x):
    x = np.asarray(x, np.float64)
    return x / math.sqrt(float((x * x).sum()))


def normal_families():
    """[(family, (n0, n1, n2))]: the normal along each axis both ways, within 2^-24 of -z (the frame's pole) on either side, skewed (three different
    unit normals), the triple that interpolates to zero at (u, v) = (0.5, 0) and the all-zero triple (geometric fallback everywhere)."""
    out = []
    for k, name in enumerate("xyz"):
        for sgn in (1.0, -1.0):
            e = np.zeros(3); e[k] = sgn
            out.append(("axis %s%s" % ("+" if sgn > 0 else "-", name), (e, e, e)))
    for dx, dy in ((EPS24, 0.0), (0.0, -EPS24), (EPS24, EPS24), (0.0, 0.0)):
        p = np.array([dx, dy, -1.0])
        out.append(("pole", (p, p, p)))
    out.append(("pole", (np.array([EPS24, 0.0, -1.0]), np.array([-EPS24, 0.0, -1.0]), np.array([0.0, EPS24, -1.0]))))
    out.append(("skewed", (_unit((0.3, 0.9, 0.2)), _unit((-0.2, 0.8, 0.5)), _unit((0.1, 0.7, -0.6)))))
    out.append(("skewed", (_unit((0.6, -0.1, -0.7)), _unit((0.5, 0.2, -0.8)), _unit((0.7, -0.3, -0.6)))))
    out.append(("cancelling", (np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, -1.0]), np.array([0.0, 1.0, 0.0]))))
    out.append(("zero normals", (np.zeros(3), np.zeros(3), np.zeros(3))))
    return out


def triangle_families():
    """[(family, (v0, v1, v2))]: a triangle in general position, an axis-aligned one away from the origin, a degenerate one (three collinear
    corners: with zero normals the point is dead) and a point triangle."""
    return [("general", (np.array([0.1, -0.2, 0.3]), np.array([0.9, 0.1, 0.25]), np.array([0.2, 0.7, -0.4]))),
            ("axis", (np.array([-0.5, -0.5, 0.125]), np.array([0.5, -0.5, 0.125]), np.array([0.5, 0.5, 0.125]))),
            ("degenerate", (np.array([0.0, 0.0, 0.0]), np.array([0.25, 0.5, -0.25]), np.array([0.5, 1.0, -0.5]))),
            ("degenerate", (np.array([0.25, 0.25, 0.25]),) * 3)]


def xi_cases(n, seed=SEED):
    """(n, 2) fp32 numbers of block 0: every pair of XI_SET first, then random k 2^-24."""
    grid = np.array([(a, b) for a in XI_SET for b in XI_SET], np.float64)
    rng = np.random.default_rng(seed)
    rest = rng.integers(0, 1 << 24, (max(0, n - len(grid)), 2)) / float(1 << 24)
    return np.concatenate([grid, rest])[:n].astype(F32)


def all_cases(n_xi=48, seed=SEED):
    """Every (triangle, normals, (u, v), side) combination with xi_cases' numbers (a different random tail per combination): a dict of arrays
    v0, v1, v2, n0, n1, n2, u, v, back, xi and `family` (the normal family, or "degenerate" for those triangles)."""
    cols = {k: [] for k in ("v0", "v1", "v2", "n0", "n1", "n2", "u", "v", "back", "xi", "family")}
    k = 0
    for tname, tri in triangle_families():
        for nname, nrm in normal_families():
            for uv in UV_SET:
                for back in (False, True):
                    xi = xi_cases(n_xi, seed + k); k += 1
                    m = len(xi)
                    for key, val in zip(("v0", "v1", "v2"), tri): cols[key].append(np.broadcast_to(val, (m, 3)))
                    for key, val in zip(("n0", "n1", "n2"), nrm): cols[key].append(np.broadcast_to(np.asarray(val, np.float64).astype(F32), (m, 3)))
                    cols["u"].append(np.full(m, uv[0], F32)); cols["v"].append(np.full(m, uv[1], F32)); cols["back"].append(np.full(m, back))
                    cols["xi"].append(xi); cols["family"].append(np.full(m, "degenerate" if tname == "degenerate" else nname))
    return {key: np.concatenate(val) for key, val in cols.items()}


def ray_ratio(got_o, got_n, got_d, ref_o, ref_n, ref_d, s_bound=S_BOUND):
    """Per ray the worst |difference| / bound over the nine components: origins and normals against s_bound slack, directions against half an fp32
    ulp of the reference plus s_bound slack."""
    ref_o, ref_n, ref_d = (np.asarray(a, np.float64) for a in (ref_o, ref_n, ref_d))
    with np.errstate(invalid="ignore"):
        ro = np.abs(np.asarray(got_o, np.float64) - ref_o) / (s_bound * slack(ref_o))
        rn = np.abs(np.asarray(got_n, np.float64) - ref_n) / (s_bound * slack(ref_n))
        rd = np.abs(np.asarray(got_d, np.float64) - ref_d) / (half_ulp32(ref_d) + s_bound * slack(ref_d))
    r = np.concatenate([ro, rn, rd], 1)
    return np.where(np.isnan(r), np.inf, r).max(1)


def slack_used(got_o, got_n, got_d, ref_o, ref_n, ref_d):
    """What a set of rays needs of the float64 slack, in its units: (origins, normals, the directions' excess over half an fp32 ulp).  A figure to
    print beside S_BOUND, not a check."""
    ref_o, ref_n, ref_d = (np.asarray(a, np.float64) for a in (ref_o, ref_n, ref_d))
    eo = np.abs(np.asarray(got_o, np.float64) - ref_o) / slack(ref_o); en = np.abs(np.asarray(got_n, np.float64) - ref_n) / slack(ref_n)
    ed = np.maximum(np.abs(np.asarray(got_d, np.float64) - ref_d) - half_ulp32(ref_d), 0.0) / slack(ref_d)
    return float(eo.max()), float(en.max()), float(ed.max())


# ------------------------------------------------------------------------------------------------------------------------ scenes
def scene_inputs(scene, centre, points, vertex=None, normal=None):
    """rays' geometric inputs for bake points (bake_abi.POINT_DTYPE) on `scene` as a context of centre `centre` holds it: corners = vertex - centre
    in float64 (build_host_scene's and rf_triangles_kernel's subtraction), normals rounded to fp32.  vertex / normal: a later pose."""
    vtx = np.asarray(scene.vertex if vertex is None else vertex, np.float64); nrm = np.asarray(scene.normal if normal is None else normal, np.float64)
    f = scene.face[points["face"].astype(np.int64)]
    c = np.asarray(centre, np.float64)
    v = [vtx[f[:, k, 0]] - c for k in range(3)]
    n = [nrm[f[:, k, 1]].astype(F32) for k in range(3)]
    return dict(v0=v[0], v1=v[1], v2=v[2], n0=n[0], n1=n[1], n2=n[2], u=points["u"], v=points["v"], back=(points["flags"] & 1) != 0)


def form_factor_rect(x0, x1, y0, y1, h):
    """The share of cosine-weighted directions about +z from the origin that meet the rectangle [x0, x1] x [y0, y1] in the parallel plane z = h > 0:
    the point-to-rectangle form factor, from the closed form for a corner rectangle (a differential element under one corner of an a x b
    rectangle at distance h: F = 1 / (2 pi) (A / sqrt(1 + A^2) atan(B / sqrt(1 + A^2)) + B / sqrt(1 + B^2) atan(A / sqrt(1 + B^2))), A = a / h,
    B = b / h) by inclusion and exclusion over the four corners.  fp64."""
    def corner(a, b):
        sa, sb = (1.0 if a >= 0 else -1.0), (1.0 if b >= 0 else -1.0)
        A, B = abs(a) / h, abs(b) / h
        f = (A / math.sqrt(1 + A * A) * math.atan(B / math.sqrt(1 + A * A)) + B / math.sqrt(1 + B * B) * math.atan(A / math.sqrt(1 + B * B))) / (2.0 * PI)
        return sa * sb * f
    return corner(x1, y1) - corner(x0, y1) - corner(x1, y0) + corner(x0, y0)
