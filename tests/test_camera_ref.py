"""CPU: the ctypes mirrors of the camera-model section against the header, the properties of the aperture sampling and of the thin lens in the
float64 restatement of tests/camera_ref.py, and the measurement of the float64 slack S behind S_BOUND, which tests/test_camera.py allows the device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import camera_ref as R, deform_kit as K, endpoints_ref as E, kit

NEW_SYMBOLS = ["mcpt_set_camera_model", "mcpt_get_camera_model", "mcpt_render_camera", "mcpt_autofocus", "mcpt_probe_camera_rays"]
METHODS = ["set_camera_model", "camera_model", "camera_model_info", "render_camera", "autofocus", "probe_camera_rays"]
INVALID = 1


def test_library_exports_the_camera_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, METHODS)
    assert (pkg.CAMERA_PINHOLE, pkg.CAMERA_THIN_LENS, pkg.CAMERA_ORTHOGRAPHIC, pkg.CAMERA_EQUIRECT) == (R.PINHOLE, R.THIN_LENS, R.ORTHOGRAPHIC, R.EQUIRECT)


def test_null_context_is_an_invalid_argument_for_the_camera_calls(pkg):
    lib = pkg.load_library()
    buf = np.zeros(64, np.float64); p = buf.ctypes.data_as(C.c_void_p); m = pkg.camera_model(); info = pkg.CameraModelInfo(); f = C.c_double()
    assert lib.mcpt_set_camera_model(None, C.byref(m)) == INVALID
    assert lib.mcpt_get_camera_model(None, C.byref(m), C.byref(info)) == INVALID
    assert lib.mcpt_render_camera(None, 1, 0, 0) == INVALID
    assert lib.mcpt_autofocus(None, 0, 0, C.byref(f)) == INVALID
    assert lib.mcpt_probe_camera_rays(None, 1, p, 0, 0, p, p) == INVALID


def test_camera_structs_have_the_headers_layout(pkg, tmp_path):
    """sizeof and every offsetof of mcpt_camera_model and mcpt_camera_model_info as a C compiler sees include/mcpt.h, against the ctypes classes;
    the model constants are the header's."""
    macros = ["MCPT_CAMERA_PINHOLE", "MCPT_CAMERA_THIN_LENS", "MCPT_CAMERA_ORTHOGRAPHIC", "MCPT_CAMERA_EQUIRECT", "MCPT_CAMERA_MAX_BLADES"]
    c, py, consts = K.c_layout(pkg.CameraModel, "mcpt_camera_model", tmp_path, macros)
    assert c == py and c[0] == 64
    assert consts == [pkg.CAMERA_PINHOLE, pkg.CAMERA_THIN_LENS, pkg.CAMERA_ORTHOGRAPHIC, pkg.CAMERA_EQUIRECT, pkg.CAMERA_MAX_BLADES] == [0, 1, 2, 3, 16]
    assert [f[0] for f in pkg.CameraModel._fields_] == ["struct_size", "model", "lens_radius", "focus_distance", "blades", "reserved0", "blade_rotation", "ortho_height",
                                                        "reserved"]
    c, py, _ = K.c_layout(pkg.CameraModelInfo, "mcpt_camera_model_info", tmp_path)
    assert c == py and c[0] == 56
    assert [f[0] for f in pkg.CameraModelInfo._fields_] == ["struct_size", "model", "renders", "reserved0", "passes", "last_stage_ms", "device_bytes", "reserved"]
    assert pkg.camera_model().struct_size == 64


def _inside(vertices, x, y, tol):
    """Every point on the inner side of every edge of the convex polygon, to tol."""
    V = np.asarray(vertices); W = np.roll(V, -1, 0)
    ex, ey = W[:, 0] - V[:, 0], W[:, 1] - V[:, 1]
    side = ex[None] * (y[:, None] - V[None, :, 1]) - ey[None] * (x[:, None] - V[None, :, 0])      # > 0: to the left of the edge (the corners run counter-clockwise)
    return (side >= -tol).all()


@pytest.mark.parametrize("blades", [b for b in R.BLADES if b])
def test_polygon_samples_lie_inside_their_polygon(blades):
    """Every lens sample of lens_cases, the edge values of LENS_XI first, lands inside the regular polygon (its boundary included, to a few ulp),
    and a polygon sample is never farther from the centre than the disk's rim."""
    V = R.lens_vertices(blades, 0.3)
    xi = R.lens_cases(4096)
    lx, ly = R.lens_point(blades, V, xi[:, 0], xi[:, 1])
    assert _inside(V, lx, ly, 8 * 2.0 ** -52)
    assert (lx * lx + ly * ly <= 1 + 8 * 2.0 ** -52).all()
    dx, dy = R.lens_point(0, None, xi[:, 0], xi[:, 1])
    assert (dx * dx + dy * dy <= 1 + 8 * 2.0 ** -52).all()


@pytest.mark.parametrize("blades", [b for b in R.BLADES if b])
def test_polygon_sampling_is_uniform_over_the_triangles(blades):
    """A 64 x 64 stratified grid of (xi2, xi3) puts equal counts, +-1, into each of the n triangles (centre, V_k, V_k+1), and inside a triangle the
    square-root map keeps the strata's share: a quarter of its samples lie in the quarter-area sub-triangle at the centre, +-1 row of the grid."""
    g = (np.arange(64) + 0.5) / 64.0
    x2, x3 = (a.ravel().astype(np.float32) for a in np.meshgrid(g, g, indexing="ij"))
    V = R.lens_vertices(blades, 0.3)
    lx, ly = R.lens_point(blades, V, x2, x3)
    ang = np.mod(np.arctan2(ly, lx) - 0.3, 2 * np.pi)
    k = np.minimum((ang / (2 * np.pi / blades)).astype(int), blades - 1)
    counts = np.bincount(k, minlength=blades)
    assert counts.max() - counts.min() <= 64 and abs(int(counts.sum()) - 4096) == 0      # whole rows of the grid fall into a triangle: 4096 / n, +- one row
    assert np.all(np.abs(counts - 4096 / blades) <= 64)
    apothem = np.cos(np.pi / blades)
    mid = (V + np.roll(V, -1, 0)) / 2; nrm = mid / np.linalg.norm(mid, axis=1, keepdims=True)
    depth = (lx * nrm[k, 0] + ly * nrm[k, 1]) / apothem                      # 0 at the centre, 1 on the edge: sqrt(xi') by construction
    assert abs(int((depth < 0.5).sum()) - 1024) <= 64


def _scene_camera(pkg):
    s = pkg.scenes.open_box(33, 17)
    return s.camera, (0.5, 0.4995, 0.5)                                      # (the centre of open_box's used vertices; any centre serves the CPU suite)


def test_thin_lens_rays_meet_the_plane_in_focus(pkg):
    """In the restatement every thin-lens ray passes through eye + focus D(u, v), to 1e-12 relative, whatever the lens point."""
    cam0, centre = _scene_camera(pkg)
    worst = 0.0
    for name, fam, model, cam, w, h, xy, xi, kw in R.all_cases(cam0, centre):
        if model != R.THIN_LENS:
            continue
        o, d = R.rays(model, cam, w, h, xy, xi, **kw)
        _, D = R.rays(R.PINHOLE, cam, w, h, xy, xi)                          # normalised D
        hh, front, right, up, eye = cam
        u0 = ((xy[:, 0].astype(np.float32) + xi[:, 0]) / np.float32(w)).astype(np.float64) - 0.5
        v0 = ((xy[:, 1].astype(np.float32) + xi[:, 1]) / np.float32(h)).astype(np.float64) - 0.5
        Dr = front[None] + (u0 * hh * w / h)[:, None] * right[None] + (v0 * hh)[:, None] * up[None]
        P = eye[None] + kw["focus_distance"] * Dr
        t = ((P - o) * d).sum(1)                                              # the ray's parameter at its closest approach to P
        miss = np.linalg.norm(o + t[:, None] * d - P, axis=1) / np.linalg.norm(P - o, axis=1)
        worst = max(worst, float(miss.max()))
        assert miss.max() <= 1e-12, (name, miss.max())
        assert np.allclose(np.cross(D, Dr), 0, atol=1e-12)
        if kw["lens_radius"] == 0.0:
            assert np.array_equal(o, np.broadcast_to(eye, o.shape))
    print("thin lens: worst relative miss of the point in focus %.3g" % worst)


def test_float64_slack(pkg):
    """S: the worst difference between the float64 restatement and the same formulas in np.longdouble over all cases, in units of
    2^-52 (1 + |value|), per family.  S_BOUND, what the device is allowed, is 4 S rounded up to a power of two."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no more bits than float64 on this platform: S cannot be measured here"
    cam0, centre = _scene_camera(pkg)
    fams, ratios, n_cases = [], [], 0
    seen_models = set()
    for name, fam, model, cam, w, h, xy, xi, kw in R.all_cases(cam0, centre):
        o, d = R.rays(model, cam, w, h, xy, xi, **kw)
        ol, dl = R.rays(model, cam, w, h, xy, xi, T=np.longdouble, **kw)
        assert o.dtype == np.float64 and ol.dtype == np.longdouble and np.isfinite(o).all() and np.isfinite(d).all()
        ratio = np.concatenate([np.abs(o - ol) / R.slack(ol.astype(np.float64)), np.abs(d - dl) / R.slack(dl.astype(np.float64))], 1).astype(np.float64).max(1)
        fams.append(fam); ratios.append(ratio); n_cases += len(ratio); seen_models.add(model)
        if model == R.EQUIRECT:                                              # the panorama's directions are unit vectors without a normalisation
            assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 8 * 2.0 ** -52
    fams, ratios = np.concatenate(fams), np.concatenate(ratios)
    assert seen_models == {R.PINHOLE, R.THIN_LENS, R.ORTHOGRAPHIC, R.EQUIRECT}
    assert set(fams) == {"corners", "last_column", "xi_edges", "random", "panorama_pole", "panorama_seam"}
    E.print_worst("float64 vs longdouble", fams, ratios, R.S_BOUND)
    s = float(ratios.max())
    print("%d cases; S = %.3f (family %s); S_BOUND = %g" % (n_cases, s, fams[ratios.argmax()], R.S_BOUND))
    assert abs(s - R.S_CPU) <= 0.005 * R.S_CPU + 0.005, "camera_ref.S_CPU is stale: measured %.4f" % s
    assert R.S_BOUND == E.next_pow2(4 * s)
