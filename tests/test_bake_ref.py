"""CPU: the surface-baking stage's restatement (tests/bake_ref.py) -- the float64 slack S that sizes the device's bound,
the properties of the sampled directions, mcpt_lightmap_points through ctypes and as a sanitized stand-alone program, the structs' layouts.  No
device is touched."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

from tests import bake_ref as R, deform_kit as K, kit

NEW_SYMBOLS = ["mcpt_set_bake_points", "mcpt_bake", "mcpt_clear_bake", "mcpt_read_bake", "mcpt_read_bake_film", "mcpt_get_bake_info", "mcpt_probe_bake_rays",
               "mcpt_lightmap_points"]
METHODS = ["set_bake_points", "bake", "clear_bake", "read_bake", "read_bake_film", "bake_info", "probe_bake_rays"]
INVALID = 1
KEYS = ("v0", "v1", "v2", "n0", "n1", "n2", "u", "v", "back", "xi")


def test_library_exports_the_bake_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, METHODS)
    assert (pkg.BAKE_IRRADIANCE, pkg.BAKE_DIFFUSE, pkg.BAKE_BACK_SIDE) == (0, 1, 1)
    assert callable(pkg.lightmap_points) and callable(pkg.vertex_bake_points)


def test_null_context_is_an_invalid_argument_for_the_bake_calls(pkg):
    lib = pkg.load_library()
    buf = np.zeros(64, np.float64); p = buf.ctypes.data_as(C.c_void_p); info = pkg.BakeInfo()
    assert lib.mcpt_set_bake_points(None, p, 1) == INVALID
    assert lib.mcpt_bake(None, 1, 0, 0) == INVALID
    assert lib.mcpt_clear_bake(None) == INVALID
    assert lib.mcpt_read_bake(None, 0, p) == INVALID
    assert lib.mcpt_read_bake_film(None, p) == INVALID
    assert lib.mcpt_get_bake_info(None, C.byref(info)) == INVALID
    assert lib.mcpt_probe_bake_rays(None, 0, 0, 0, 1, p, p, p, p) == INVALID


def test_bake_structs_have_the_headers_layout(pkg, tmp_path):
    """sizeof and every offsetof of mcpt_bake_point (16 B) and mcpt_bake_info as a C compiler sees include/mcpt.h, against the ctypes classes and
    the numpy record; the constants are the header's."""
    c, py, consts = K.c_layout(pkg.BakePoint, "mcpt_bake_point", tmp_path, ["MCPT_BAKE_BACK_SIDE", "MCPT_BAKE_IRRADIANCE", "MCPT_BAKE_DIFFUSE"])
    assert c == py and c[0] == 16
    assert consts == [pkg.BAKE_BACK_SIDE, pkg.BAKE_IRRADIANCE, pkg.BAKE_DIFFUSE]
    dt = pkg.bake_abi.POINT_DTYPE
    assert dt.itemsize == 16 and [dt.fields[f][1] for f in ("face", "u", "v", "flags")] == c[1:]
    c, py, _ = K.c_layout(pkg.BakeInfo, "mcpt_bake_info", tmp_path)
    assert c == py and c[0] == 56
    assert [f[0] for f in pkg.BakeInfo._fields_] == ["struct_size", "n_points", "n_dead", "bakes", "passes", "last_stage_ms", "device_bytes", "reserved"]


# ------------------------------------------------------------------------------------------------------------------------ the restatement
def test_float64_slack():
    """S: the worst difference between the float64 restatement and the same formulas in np.longdouble over all cases -- every origin, normal and
    unrounded direction component --, in units of 2^-52 (1 + |value|), per family.  S_BOUND, what the device is allowed, is 4 S rounded up to
    a power of two.  Both types flag the same points dead."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no more bits than float64 on this platform: S cannot be measured here"
    c = R.all_cases()
    a = R.rays(*[c[k] for k in KEYS]); b = R.rays(*[c[k] for k in KEYS], T=np.longdouble)
    assert a[0].dtype == np.float64 and b[0].dtype == np.longdouble
    assert np.array_equal(a[3], b[3])
    worst = {}
    for name in np.unique(c["family"]):
        m = c["family"] == name
        worst[name] = max(float((np.abs(x[m].astype(np.longdouble) - y[m]) / (np.longdouble(2.0) ** -52 * (1 + np.abs(y[m])))).max()) for x, y in zip(a[:3], b[:3]))
        print("%-14s %6d rays, %5d dead, S = %.3f" % (name, m.sum(), a[3][m].sum(), worst[name]))
    S = max(worst.values())
    bound = 2.0 ** np.ceil(np.log2(4.0 * S))
    print("S = %.3f (family %s), 4 S = %.2f, S_BOUND = %g" % (S, max(worst, key=worst.get), 4 * S, bound))
    assert len(c["u"]) > 40000
    assert abs(S - R.S_CPU) < 0.01 and bound == R.S_BOUND, "tests/bake_ref.py states S = %.2f and S_BOUND = %g" % (R.S_CPU, R.S_BOUND)


def test_case_families_flag_the_dead_and_fall_back():
    """The degenerate triangles are dead exactly under normals that give no direction (the all-zero triple everywhere, the cancelling triple at
    (0.5, 0)); on proper triangles nothing is dead, and where the vertex normals give nothing the normal is the geometric one."""
    c = R.all_cases(n_xi=16)
    o, n, d, dead = R.rays(*[c[k] for k in KEYS])
    degenerate = c["family"] == "degenerate"
    assert not dead[~degenerate].any() and dead[degenerate].any() and not dead[degenerate].all()
    assert (d[dead] == np.array([0.0, 0.0, 1.0])).all() and (n[dead] == 0).all() and np.isfinite(o).all()
    zero = (c["family"] == "zero normals")
    e1 = c["v1"][zero] - c["v0"][zero]; e2 = c["v2"][zero] - c["v0"][zero]
    g = np.cross(e1, e2); g /= np.linalg.norm(g, axis=1)[:, None]
    g = np.where(c["back"][zero][:, None], -g, g)
    assert np.abs(n[zero] - g).max() < 1e-15
    cancel = (c["family"] == "cancelling") & (c["u"] == 0.5) & (c["v"] == 0.0)
    assert cancel.any() and np.abs(np.abs((n[cancel] * np.cross(c["v1"][cancel] - c["v0"][cancel], c["v2"][cancel] - c["v0"][cancel])).sum(1))
                                   - np.linalg.norm(np.cross(c["v1"][cancel] - c["v0"][cancel], c["v2"][cancel] - c["v0"][cancel]), axis=1)).max() < 1e-15


def test_directions_stay_on_their_side_and_have_unit_length():
    """Every live ray of all_cases, its direction rounded to fp32 as the device stores it: dot(D, N) >= -2^-23 and | |D| - 1 | <= 4 x 2^-24."""
    c = R.all_cases()
    o, n, d, dead = R.rays(*[c[k] for k in KEYS])
    d32 = d.astype(np.float32).astype(np.float64)[~dead]; n = n[~dead]
    dots = (d32 * n).sum(1); lens = np.sqrt((d32 * d32).sum(1))
    print("%d rays: min dot(D, N) = %.3e, worst | |D| - 1 | = %.3e (bound %.3e)" % (len(dots), dots.min(), np.abs(lens - 1).max(), 4 * 2.0 ** -24))
    assert dots.min() >= -2.0 ** -23
    assert np.abs(lens - 1).max() <= 4 * 2.0 ** -24
    assert np.abs((n * n).sum(1) - 1).max() < 1e-15


def test_directions_are_cosine_weighted():
    """On a 64 x 64 stratified grid of (xi0, xi1) (cell centres) the mean of dot(D, N) is within 1e-3 of 2 / 3, the mean cosine of a
    cosine-weighted hemisphere, for an axis normal, a pole normal and a skewed one, on both sides.  The midpoint rule's own error on
    sqrt(1 - x) over 64 cells is 1.14e-4 (measured: the printed figure, the same for every normal)."""
    g = ((np.arange(64) + 0.5) / 64.0).astype(np.float32)
    xi = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    m = len(xi)
    tri = R.triangle_families()[0][1]
    fams = dict((name, nrm) for name, nrm in R.normal_families())
    for name in ("axis +y", "pole", "skewed"):
        for back in (False, True):
            nrm = fams[name]
            args = [np.broadcast_to(t, (m, 3)) for t in tri] + [np.broadcast_to(np.asarray(x, np.float32), (m, 3)) for x in nrm]
            o, n, d, dead = R.rays(*args, np.full(m, 0.25, np.float32), np.full(m, 0.25, np.float32), np.full(m, back), xi)
            mean = float((d * n).sum(1).mean())
            print("%-8s back %d: mean dot(D, N) = %.6f, off 2/3 by %.2e" % (name, back, mean, mean - 2.0 / 3.0))
            assert not dead.any() and abs(mean - 2.0 / 3.0) < 1e-3
            # the azimuth is uniform: the tangential part averages out
            t = d - (d * n).sum(1)[:, None] * n
            assert np.abs(t.mean(0)).max() < 1e-3


def test_form_factor_closed_form_against_quadrature():
    """bake_ref.form_factor_rect, the analytic share the device test holds the baked hit share against, against a brute-force midpoint quadrature
    of cos^2 / (pi r^2) dA ... = h^2 / (pi (x^2 + y^2 + h^2)^2) over the rectangle, for a centred and an off-centre rectangle."""
    for rect, h in (((-0.15, 0.15, -0.15, 0.15), 0.999), ((0.1, 0.6, -0.3, 0.2), 0.5), ((-1.0, 2.0, -0.5, 0.25), 0.3)):
        n = 2000
        x = rect[0] + (np.arange(n) + 0.5) * (rect[1] - rect[0]) / n; y = rect[2] + (np.arange(n) + 0.5) * (rect[3] - rect[2]) / n
        X, Y = np.meshgrid(x, y, indexing="ij")
        q = float((h * h / (np.pi * (X * X + Y * Y + h * h) ** 2)).sum() * (rect[1] - rect[0]) * (rect[3] - rect[2]) / (n * n))
        f = R.form_factor_rect(*rect, h)
        print("rect %s at h = %g: closed form %.9f, quadrature %.9f" % (rect, h, f, q))
        assert abs(f - q) < 1e-6 and 0 < f < 1


# ------------------------------------------------------------------------------------------------------------------------ the rasteriser
def _atlas(pkg, texcoord, faces_vt):
    """A scene description of len(faces_vt) faces over four vertices whose only meaningful part is the texcoords: faces_vt lists per face its three
    texcoord indices."""
    S = pkg.scenes
    vertex = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1]], np.float64); normal = np.array([[0, 1, 0]], np.float64)
    face = np.zeros((len(faces_vt), 3, 4), np.int32)
    for f, vt in enumerate(faces_vt):
        for k in range(3):
            face[f, k] = (k + 1 if k else 0, 0, vt[k], 0)
    return S.SceneData("atlas", vertex, normal, np.asarray(texcoord, np.float64).reshape(-1, 2), face, [S.Material("white", kd=(0.7, 0.7, 0.7))],
                       S.Camera((0.5, 1, 0.5), (0.5, 0, 0.5), (0, 0, 1), 40.0, 4, 4))


SQUARE = [(0, 0), (1, 0), (1, 1), (0, 1)]
QUAD = [(0, 1, 2), (0, 2, 3)]                                # the diagonal (0, 0) - (1, 1) belongs to both


def _texel_centres(tex, w, h):
    return np.stack([((tex % w) + 0.5) / w, ((tex // w) + 0.5) / h], -1)


def _check_square(pkg, scene, pts, tex, w, h, first_face=0):
    tc = scene.texcoord; f = scene.face[pts["face"].astype(np.int64)]
    assert np.array_equal(tex, np.arange(w * h, dtype=np.uint32)), "every texel exactly once, in texel order"
    c = _texel_centres(tex, w, h)
    i, j = (tex % w).astype(np.int64), (tex // w).astype(np.int64)
    on_diagonal = (2 * i + 1) * h == (2 * j + 1) * w                           # the centre's x == its y, in integers
    assert (pts["face"][on_diagonal] == first_face).all()
    assert np.array_equal(pts["face"] == first_face, (2 * i + 1) * h >= (2 * j + 1) * w)     # face 0 = (0,0), (1,0), (1,1): below the diagonal, and on it
    u = pts["u"].astype(np.float64)[:, None]; v = pts["v"].astype(np.float64)[:, None]
    back = tc[f[:, 0, 2]] + u * (tc[f[:, 1, 2]] - tc[f[:, 0, 2]]) + v * (tc[f[:, 2, 2]] - tc[f[:, 0, 2]])
    assert np.abs(back - c).max() <= 1e-6
    assert (pts["u"] >= 0).all() and (pts["v"] >= 0).all() and (pts["u"].astype(np.float64) + pts["v"].astype(np.float64) <= 1.0).all()
    assert (pts["flags"] == 0).all()


@pytest.mark.parametrize("w,h", [(8, 8), (7, 5), (1, 1)])
def test_lightmap_points_on_the_unit_square(pkg, w, h):
    """A two-triangle unit-square atlas: every texel appears exactly once, texels on the diagonal go to face 0, the barycentrics give the texel
    centre back to 1e-6 and pass mcpt_set_bake_points' rule."""
    scene = _atlas(pkg, SQUARE, QUAD)
    pts, tex = pkg.lightmap_points(scene, w, h)
    _check_square(pkg, scene, pts, tex, w, h)
    if (w, h) == (8, 8):
        assert ((tex % w) == (tex // w)).sum() == 8


def test_lightmap_points_skips_flat_faces_and_does_not_wrap(pkg):
    """A face whose three texcoords are one point, or three collinear ones, is skipped -- listed FIRST, it takes nothing from the faces behind it;
    an atlas moved to [2, 3]^2 covers nothing (uv is not wrapped); half an atlas covers half the texels."""
    scene = _atlas(pkg, SQUARE + [(0.5, 0.5)], [(4, 4, 4), (0, 4, 2)] + QUAD)
    pts, tex = pkg.lightmap_points(scene, 8, 8)
    assert set(np.unique(pts["face"])) == {2, 3}
    remap = pts.copy(); remap["face"] -= 2
    _check_square(pkg, _atlas(pkg, SQUARE, QUAD), remap, tex, 8, 8)
    away = _atlas(pkg, np.array(SQUARE, np.float64) + 2.0, QUAD)
    pts, tex = pkg.lightmap_points(away, 8, 8)
    assert len(pts) == 0 and len(tex) == 0
    half = _atlas(pkg, np.array(SQUARE, np.float64) * 0.5, QUAD)
    pts, tex = pkg.lightmap_points(half, 8, 8)
    covered = ((tex % 8) < 4) & ((tex // 8) < 4)
    assert len(tex) == 16 and covered.all()
    nan = _atlas(pkg, [(0, 0), (np.nan, 0), (1, 1), (0, 1)], QUAD)
    pts, tex = pkg.lightmap_points(nan, 4, 4)
    assert (pts["face"] == 1).all() and len(pts) == 10                        # (the face with the NaN corner has no finite area; the other half keeps its texels, the diagonal's too)


def test_lightmap_points_capacity_protocol_and_refusals(pkg):
    """capacity < the count: MCPT_ERR_INVALID_ARG with *out_n set and nothing written, as for mcpt_probe_lights; a full call then fills exactly
    that many.  Refused: no texels, a texcoord index out of range, null arguments."""
    lib = pkg.load_library()
    holder = pkg.DescHolder(_atlas(pkg, SQUARE, QUAD))
    n = C.c_uint32(99)
    big = np.zeros(64, pkg.bake_abi.POINT_DTYPE); tex = np.full(64, 7, np.uint32)
    assert lib.mcpt_lightmap_points(C.byref(holder.desc), 8, 8, 10, big.ctypes.data_as(C.c_void_p), tex.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID
    assert n.value == 64 and (tex == 7).all() and (big["face"] == 0).all() and b"capacity" in lib.mcpt_last_error()
    assert lib.mcpt_lightmap_points(C.byref(holder.desc), 8, 8, 64, big.ctypes.data_as(C.c_void_p), tex.ctypes.data_as(C.c_void_p), C.byref(n)) == 0
    assert n.value == 64 and np.array_equal(tex, np.arange(64))
    assert lib.mcpt_lightmap_points(C.byref(holder.desc), 0, 8, 64, big.ctypes.data_as(C.c_void_p), tex.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID and n.value == 0
    assert lib.mcpt_lightmap_points(C.byref(holder.desc), 8, 8, 64, big.ctypes.data_as(C.c_void_p), tex.ctypes.data_as(C.c_void_p), None) == INVALID
    assert lib.mcpt_lightmap_points(None, 8, 8, 64, big.ctypes.data_as(C.c_void_p), tex.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID
    assert lib.mcpt_lightmap_points(C.byref(holder.desc), 8, 8, 64, None, None, C.byref(n)) == INVALID and n.value == 64
    bad = _atlas(pkg, SQUARE, QUAD); bad.face[1, 2, 2] = 4
    with pytest.raises(pkg.McptError, match="texcoord index out of range"):
        pkg.lightmap_points(bad, 4, 4)


def test_vertex_bake_points(pkg):
    """One point per face corner at that corner, and the vertex it belongs to."""
    scene = pkg.scenes.open_box(8, 8)
    pts, vert = pkg.vertex_bake_points(scene)
    assert len(pts) == 3 * scene.face.shape[0] == len(vert)
    p = scene.vertex[scene.face[:, :, 0]]                                      # (nf, 3 corners, 3)
    f = pts["face"].astype(np.int64); u = pts["u"].astype(np.float64)[:, None]; v = pts["v"].astype(np.float64)[:, None]
    at = p[f, 0] + u * (p[f, 1] - p[f, 0]) + v * (p[f, 2] - p[f, 0])
    assert np.array_equal(at, scene.vertex[vert])
    assert np.array_equal(np.bincount(vert, minlength=scene.vertex.shape[0]) > 0, np.isin(np.arange(scene.vertex.shape[0]), scene.face[:, :, 0]))


def _host_cases(pkg):
    rng = np.random.default_rng(R.SEED)
    soup_tc = rng.uniform(-0.25, 1.25, (40, 2)); soup = [tuple(rng.integers(0, 40, 3)) for _ in range(30)]
    return [(8, 8, SQUARE, QUAD), (7, 5, SQUARE, QUAD), (1, 1, SQUARE, QUAD), (8, 8, SQUARE + [(0.5, 0.5)], [(4, 4, 4), (0, 4, 2)] + QUAD),
            (8, 8, (np.array(SQUARE, np.float64) + 2.0).tolist(), QUAD), (33, 17, soup_tc.tolist(), soup), (5, 3, [(0, 0), (np.nan, 0), (1, 1), (0, 1)], QUAD),
            (16, 16, [(0, 0), (1e308, 0), (1e308, 1e308), (0, 1e308)], QUAD), (4, 4, SQUARE, [])]


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
def test_lightmap_points_as_a_stand_alone_program(pkg, tmp_path, sanitized):
    """The host half of the feature -- bk_lightmap_points and bk_check_points of csrc/bake_plan.h -- built into the stand-alone program
    tests/bake_host_check.cpp (no device is touched), plain and under the host's address and undefined-behaviour sanitizers: the same points and
    texels as mcpt_lightmap_points gives through ctypes, on the atlases above, a random soup of faces reaching outside [0, 1]^2, a NaN and an
    overflowing atlas and a scene without faces; every point passes mcpt_set_bake_points' rule inside the program."""
    exe = K.build_host_check("bake_host_check", [], tmp_path, sanitized)
    cases = _host_cases(pkg)
    blob = struct.pack("<I", len(cases))
    for w, h, tc, faces in cases:
        tc = np.asarray(tc, np.float64).reshape(-1, 2)
        rec = np.zeros((len(faces), 3, 4), np.int32)
        for f, vt in enumerate(faces):
            rec[f, :, 2] = vt
        blob += struct.pack("<4I", w, h, len(tc), len(faces)) + tc.tobytes() + rec.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    K.run_host_check(exe, tmp_path, sanitized)
    out = (tmp_path / "out.bin").read_bytes(); at = 0
    for w, h, tc, faces in cases:
        status, n = struct.unpack_from("<2I", out, at); at += 8
        pts = np.frombuffer(out, pkg.bake_abi.POINT_DTYPE, n, at); at += 16 * n
        tex = np.frombuffer(out, np.uint32, n, at); at += 4 * n
        assert status == 0
        if faces:
            want_p, want_t = pkg.lightmap_points(_atlas(pkg, tc, faces), w, h)
            assert np.array_equal(pts.view(np.uint8), want_p.view(np.uint8)) and np.array_equal(tex, want_t), (w, h)
        else:
            assert n == 0
    assert at == len(out)
