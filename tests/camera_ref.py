"""Plain numpy restatements of the four camera models of the ray-generation stage (csrc/camera.hip), their case generators
and the error model of tests/test_camera_ref.py (CPU) and tests/test_camera.py (device).  Written from the definitions in include/mcpt.h and
DESIGN.md section 25.

`rays` takes the camera constants the way tests/endpoints_ref.py::camera_constants forms them (float64, camera_constants' operation order; the
device's eye is eye - centre), the fp32 random numbers of the camera block (xi[:, 0:2] the pixel jitter, xi[:, 2:4] the lens sample) and the
polygon's corners as `lens_vertices` forms them on the host's side, and works in ONE floating-point type after that: np.float64 restates the
device, one rounding per operation in the device's operation order; np.longdouble is the same formulas with 11 more bits.  ((float)px + xi) /
(float)width is replayed in np.float32 first, as cast_ref does: both operations are IEEE, the replay is bit-exact.

Error model.  S is the worst |float64 restatement - longdouble restatement| over every origin and (unrounded) direction component of every case of
`all_cases`, in units of 2^-52 (1 + |value|): what the formulas themselves lose in float64.  tests/test_camera_ref.py measures it; the device is
allowed S_BOUND = 4 S rounded up to a power of two, a stand-in for its sincos / sqrt / rsq64 chain (two Newton steps on the hardware seed, about an
ulp), which nobody has measured separately.  A direction component is rounded to fp32 on the device: it gets half an fp32 ulp of the reference on top.

    S measured on the CPU: 1.77 (family random), 4 S = 7.09, so S_BOUND = 8
    the device on an MI355X, 93 600 rays: the origins use 0.63 of those units, the directions none beyond their half fp32 ulp

The device's pixel jitter and lens sample are whatever rng_block gives for (pixel, sample): tests/test_camera.py takes them from probe_rng and feeds
them to `rays`, so the edge values of LENS_XI are reached by the CPU suite only; the pixels, the models and their parameters are the same on both.
"""
from __future__ import annotations

import math

import numpy as np

from tests import endpoints_ref as E

F32 = np.float32
PI = 3.14159265358979323846
PINHOLE, THIN_LENS, ORTHOGRAPHIC, EQUIRECT = 0, 1, 2, 3
S_CPU = 1.77                                                # measured by tests/test_camera_ref.py::test_float64_slack
S_BOUND = 8.0
LENS_XI = (0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24)
BLADES = (0, 3, 5, 16)
LENS_RADII = (0.0, 1e-3, 1.0)
FILMS = tuple(f for f in E.FILMS if f[0] <= 33 and f[1] <= 17) + ((33, 17),)     # (1, 1), (3, 2) of E.FILMS and the suite's own film
CAMERAS = ("fovy 40", "up skewed", "along -x")              # of E.camera_cases: the scene's view, an `up` that is not orthogonal to it, an axis view


def slack(x):
    """The float64 unit of the error model at value x."""
    return 2.0 ** -52 * (1.0 + np.abs(np.asarray(x, np.float64)))


def half_ulp32(x):
    """Half the spacing of fp32 at |x| (the binade of x itself, 2^-150 in the denormal range): the most that rounding x to fp32 moves it."""
    _, ex = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.ldexp(1.0, np.maximum(ex - 25, -150))


def lens_vertices(blades, rotation):
    """(blades, 2) float64: the aperture polygon's corners (cos, sin)(rotation + 2 pi j / blades) as the host forms them."""
    a = [float(rotation) + 2.0 * PI * float(j) / float(blades) for j in range(int(blades))]
    return np.array([[math.cos(x), math.sin(x)] for x in a], np.float64).reshape(-1, 2)


def device_camera(camera, centre):
    """(h, front, right, up, eye - centre) in float64, as camera_constants forms them."""
    h, front, right, up = E.camera_constants(camera)
    eye = np.array([float(x) for x in camera.eye], np.float64) - np.asarray(centre, np.float64)
    return h, front, right, up, eye


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0], a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def lens_point(blades, vertices, xi2, xi3, T=np.float64):
    """(lx, ly) of the thin lens in units of its radius for fp32 lens samples xi2, xi3."""
    x2 = np.asarray(xi2, F32).astype(T); x3 = np.asarray(xi3, F32).astype(T)
    if blades == 0:
        r = np.sqrt(x2); th = (T(2.0) * T(PI)) * x3
        return r * np.cos(th), r * np.sin(th)
    n = int(blades); V = np.asarray(vertices, np.float64).astype(T)
    x = x2 * T(n)
    k = np.minimum(x.astype(np.int64), n - 1); k1 = np.where(k + 1 == n, 0, k + 1)
    s = np.sqrt(x - k.astype(T)); a = s * (T(1.0) - x3); b = s * x3
    return a * V[k, 0] + b * V[k1, 0], a * V[k, 1] + b * V[k1, 1]


def rays(model, cam, width, height, xy, xi, lens_radius=0.0, focus_distance=1.0, blades=0, rotation=0.0, ortho_height=1.0, T=np.float64):
    """(origin (N, 3), direction (N, 3)) in type T for pixels xy (N, 2) and camera-block numbers xi (N, 4) fp32; cam = device_camera(...).  The
    origin is in device coordinates; the direction is what the device rounds to fp32."""
    h, front, right, up, eye = (np.asarray(c, np.float64).astype(T) for c in cam)
    xy = np.asarray(xy, np.int32).reshape(-1, 2); xi = np.asarray(xi, F32).reshape(-1, 4)
    fx = (xy[:, 0].astype(F32) + xi[:, 0]) / F32(width); fy = (xy[:, 1].astype(F32) + xi[:, 1]) / F32(height)      # the fp32 replay: bit-exact
    assert fx.dtype == F32 and fy.dtype == F32
    u0 = fx.astype(T) - T(0.5); v0 = fy.astype(T) - T(0.5)
    n = len(xy); W, H = T(float(width)), T(float(height))
    lup = _cross(right, front)
    if model in (PINHOLE, THIN_LENS):
        u = u0 * h * W / H; v = v0 * h
        D = (front[None] + u[:, None] * right[None]) + v[:, None] * up[None]
        if model == PINHOLE:
            o = np.broadcast_to(eye, (n, 3)).copy(); q = D
        else:
            P = eye[None] + T(focus_distance) * D
            lx, ly = lens_point(blades, lens_vertices(blades, rotation) if blades else None, xi[:, 2], xi[:, 3], T)
            o = eye[None] + T(lens_radius) * (lx[:, None] * right[None] + ly[:, None] * lup[None])
            q = P - o
        inv = T(1.0) / np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        return o, q * inv[:, None]
    if model == ORTHOGRAPHIC:
        su = u0 * T(ortho_height) * W / H; sv = v0 * T(ortho_height)
        o = (eye[None] + su[:, None] * right[None]) + sv[:, None] * up[None]
        return o, np.broadcast_to(front, (n, 3)).copy()
    lam = (T(2.0) * T(PI)) * u0; phi = T(PI) * v0
    a = np.cos(lam)[:, None] * front[None] + np.sin(lam)[:, None] * right[None]
    return np.broadcast_to(eye, (n, 3)).copy(), np.cos(phi)[:, None] * a + np.sin(phi)[:, None] * lup[None]


def model_cases():
    """[(name, model, parameters of `rays`)]: every model; the thin lens with every aperture of BLADES at every radius of LENS_RADII."""
    out = [("pinhole", PINHOLE, {})]
    for b in BLADES:
        for rad in LENS_RADII:
            out.append(("thin_lens blades %d radius %g" % (b, rad), THIN_LENS, dict(lens_radius=rad, focus_distance=1.75, blades=b, rotation=0.3)))
    out.append(("orthographic", ORTHOGRAPHIC, dict(ortho_height=1.25)))
    out.append(("panorama", EQUIRECT, {}))
    return out


def pixel_cases(width, height, seed=E.SEED):
    """E.pixel_cases' pixels, jitter and families for one film, and for the panorama the pole rows and the seam column: (xy, xi (N, 2), family).
    xi_y = 0 on row 0 is the lower pole exactly (phi = -pi / 2); the upper one is approached to 2^-24 of a pixel; xi_x = 0 on column width / 2 of an
    even film is lambda = 0 and column 0 with xi_x = 0 the seam lambda = -pi, which the last column reaches from the other side."""
    xy, xi, fam = E.pixel_cases(width, height, seed)
    cols = np.unique(np.array([0, width // 2, width - 1]))
    extra_xy, extra_xi, extra_f = [], [], []
    for row, b, name in ((0, 0.0, "panorama_pole"), (height - 1, 1.0 - E.EPS24, "panorama_pole")):
        for c in cols:
            for a in E.XI_SET:
                extra_xy.append((c, row)); extra_xi.append((a, b)); extra_f.append(name)
    rows = np.unique(np.array([0, height // 2, height - 1]))
    for c, a in ((0, 0.0), (0, E.EPS24), (width - 1, 1.0 - E.EPS24), (width // 2, 0.0)):
        for r in rows:
            for b in E.XI_SET:
                extra_xy.append((c, r)); extra_xi.append((a, b)); extra_f.append("panorama_seam")
    return (np.concatenate([xy, np.array(extra_xy, np.int32)]), np.concatenate([xi, np.array(extra_xi, np.float64).astype(F32)]),
            np.concatenate([fam, np.array(extra_f)]))


def lens_cases(n, seed=E.SEED):
    """(n, 2) fp32 lens samples: every pair of LENS_XI first, then random k 2^-24."""
    grid = np.array([(a, b) for a in LENS_XI for b in LENS_XI], np.float64)
    rng = np.random.default_rng(seed + 99)
    rest = rng.integers(0, 1 << 24, (max(0, n - len(grid)), 2)) / float(1 << 24)
    return np.concatenate([grid, rest])[:n].astype(F32)


def all_cases(scene_camera, centre):
    """Every (camera, film, model) combination of CAMERAS, FILMS and model_cases with pixel_cases' pixels and lens_cases' lens samples:
    yields (name, family (N,), model, cam, width, height, xy, xi (N, 4), parameters)."""
    cams = {c[1]: c[2] for c in E.camera_cases(scene_camera, centre)}
    for cname in CAMERAS:
        c = cams[cname]
        for w, h in FILMS:
            camera = E.SimpleNamespace(eye=c["eye"], lookat=c["lookat"], up=c["up"], fovy=c["fovy"], width=w, height=h)
            cam = device_camera(camera, centre)
            xy, xi2, fam = pixel_cases(w, h)
            xi = np.concatenate([xi2, lens_cases(len(xy), E.SEED + w)], 1)
            for name, model, kw in model_cases():
                yield "%s, %dx%d, %s" % (cname, w, h, name), fam, model, cam, w, h, xy, xi, kw


def ray_slack_used(got_o, got_d, ref_o, ref_d):
    """What a set of rays needs of the float64 slack, in its units 2^-52 (1 + |x|): (the worst origin error, the worst excess of a direction error
    over half an fp32 ulp).  A figure to print beside S_BOUND, not a check."""
    ref_o = np.asarray(ref_o, np.float64); ref_d = np.asarray(ref_d, np.float64)
    eo = np.abs(np.asarray(got_o, np.float64) - ref_o) / slack(ref_o)
    ed = np.maximum(np.abs(np.asarray(got_d, np.float64) - ref_d) - half_ulp32(ref_d), 0.0) / slack(ref_d)
    return float(eo.max()), float(ed.max())


def ray_ratio(got_o, got_d, ref_o, ref_d, s_bound=S_BOUND):
    """Per ray the worst |difference| / bound over the six components: origins against s_bound slack, directions against half an fp32 ulp of the
    reference plus s_bound slack."""
    ref_o = np.asarray(ref_o, np.float64); ref_d = np.asarray(ref_d, np.float64)
    with np.errstate(invalid="ignore"):
        ro = np.abs(np.asarray(got_o, np.float64) - ref_o) / (s_bound * slack(ref_o))
        rd = np.abs(np.asarray(got_d, np.float64) - ref_d) / (half_ulp32(ref_d) + s_bound * slack(ref_d))
    r = np.concatenate([ro, rd], 1)
    return np.where(np.isnan(r), np.inf, r).max(1)
