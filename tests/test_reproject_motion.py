"""Motion-vector reprojection: mcpt_update_vertices_reproject, mcpt_probe_first_hits, mcpt_probe_reproject_motion
(csrc/reproject.hip) and their public surfaces.

CPU tests pin the C ABI surface and the numpy restatement of the kernel (tests/reproject_motion_ref.py) on worlds with known answers; GPU tests
check the two kernels against the trace probes and that restatement, and the call's sequencing, state and refusals on a dynamic S-cornell.
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import kit
from tests.kit import CAM_A, CAM_B, OPTS, SEED_F, SIZES, Cam, bits, compare_with_ref, synthetic_film
from tests.reproject_ref import camera_constants, reproject_ref
from tests.reproject_motion_ref import emissive_faces, reproject_motion_ref, shading_normals, view_features

NEW_SYMBOLS = ["mcpt_update_vertices_reproject", "mcpt_probe_first_hits", "mcpt_probe_reproject_motion"]
INVALID, UNSUPPORTED = 1, 6
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------ CPU: the ABI
def test_library_exports_the_motion_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, ("update_vertices_reproject", "probe_first_hits", "probe_reproject_motion"))


def test_null_context_is_an_invalid_argument_for_the_motion_calls(pkg):
    lib = pkg.load_library()
    cam = pkg.CameraC(); n = C.c_uint64(0)
    o = pkg.ReprojectOpts(); o.struct_size = C.sizeof(pkg.ReprojectOpts)       # the calls take §13's options struct as it is
    buf = np.zeros(8, np.float32); p = buf.ctypes.data_as(C.c_void_p)
    v = np.zeros((4, 3)); vp = v.ctypes.data_as(C.c_void_p)
    assert lib.mcpt_update_vertices_reproject(None, vp, 4, None, 0, None, None) == INVALID
    assert lib.mcpt_update_vertices_reproject(None, vp, 4, vp, 4, C.byref(cam), C.byref(o)) == INVALID
    assert lib.mcpt_probe_first_hits(None, p, p) == INVALID
    assert lib.mcpt_probe_reproject_motion(None, C.byref(cam), C.byref(cam), None, None, p, p, p, p, p, C.byref(o), p, C.byref(n)) == INVALID


# ------------------------------------------------------------------------------------------------------------------------ synthetic worlds
QUAD_C = np.array([0.05, -0.03, 1.0])                                        # centre of the quad that moves


def _world(pkg, w, h, cam):
    """A wall z = 0 (its left edge inside the view: the pixels beyond it miss), a quad one unit in front of it and one emissive triangle."""
    S = pkg.scenes
    m = S._Mesh()
    m.add_quad((-1.7, -3, 0), (40, -3, 0), (40, 3, 0), (-1.7, 3, 0), (0, 0, 1), 0)
    c = QUAD_C
    m.add_quad(c + (-0.5, -0.4, 0), c + (0.5, -0.4, 0), c + (0.5, 0.4, 0), c + (-0.5, 0.4, 0), (0, 0, 1), 1)
    i = [m.add_vertex(p, (0, 0, 1), (0, 0)) for p in ((0.8, 0.5, 1.5), (1.3, 0.5, 1.5), (0.8, 1.0, 1.5))]
    m.add_tri(i[0], i[1], i[2], 2)
    mats = [S.Material("wall", kd=(0.7, 0.7, 0.7)), S.Material("quad", kd=(0.2, 0.5, 0.3)), S.Material("lamp", kd=(0.5, 0.5, 0.5), radiance=(9.0, 9.0, 9.0))]
    return m.finish("motion-world", mats, S.Camera(cam.eye, cam.lookat, cam.up, cam.fovy, w, h))


QUAD_V = slice(4, 8)                                                         # the quad's vertices (and normals) in _world's arrays


def _moved(scene, kind):
    """(vertex, normal) of `scene` with its quad moved."""
    v, n = scene.vertex.copy(), scene.normal.copy()
    if kind.startswith("drift+"):                                             # the wall drifts by a fraction of a pixel: with a fixed camera a wall at
        v[:4] += (0.013, -0.021, 0.0); kind = kind[6:]                        # rest lands on whole pixels, which the restatement calls marginal
    if kind in ("lateral", "lateral+camera"):
        v[QUAD_V] += (0.237, 0.051, 0.0)                                     # 2.5 / 0.5 pixels at 23 rows: not a whole-pixel shift
    elif kind == "rotate":
        a = math.radians(30.0)
        R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        v[QUAD_V] = (v[QUAD_V] - QUAD_C) @ R.T + QUAD_C; n[QUAD_V] = n[QUAD_V] @ R.T
    elif kind == "translate-all":
        v += (0.31, -0.17, 0.23)
    else:
        assert kind == "identity"
    return v, n


PROBE_CASES = [(s, "drift+lateral", "default") for s in SIZES] + [((37, 23), "drift+rotate", "default"), ((130, 9), "drift+rotate", "other"),
                                                                  ((37, 23), "lateral+camera", "default"), ((130, 9), "lateral+camera", "other")]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _probe_case(size, kind, opts):
    """Inputs of one probe test.  The scene is the world BEFORE the move; the hits and the new features are those of the moved world.  The new
    features are alive everywhere (also where the centre ray misses or meets the lamp: those pixels must come back empty by the hit alone), a few
    pixels mostly background or mostly surface."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    w, h = size
    k = Case()
    k.old_cam = Cam(width=w, height=h, **CAM_A)
    k.new_cam = Cam(width=w, height=h, **(CAM_B if kind.endswith("camera") else CAM_A))
    k.scene = _world(pkg, w, h, k.old_cam)
    k.face, k.emissive = k.scene.face, emissive_faces(k.scene)
    k.old_v, k.old_n = k.scene.vertex, k.scene.normal
    k.new_v, k.new_n = _moved(k.scene, kind)
    seed = 1000 * w + h
    k.film = synthetic_film(h, w, seed, nan=0 if w * h < 10 else 3)
    if w * h == 1:
        k.film[0, 0] = (3.5, 7.0, 1.75, 7.0)
    k.old_feat, _, _, _ = view_features(k.old_cam, k.old_v, k.old_n, k.face, k.emissive)
    k.new_feat, k.hit_face, k.hit_uv, t = view_features(k.new_cam, k.new_v, k.new_n, k.face, k.emissive)
    dead = k.new_feat[..., 3] < 0.5
    k.new_feat[dead, :4] = (0.5, 0.5, 0.5, 1.0); k.new_feat[dead, 4:7] = (0.0, 0.0, 1.0); k.new_feat[dead, 7] = np.where(t[dead] > 0, t[dead], 4.0)
    u = np.random.default_rng(seed + 2).uniform(size=(h, w))
    if w * h > 1:
        k.new_feat[u < 0.05, 3] = 0.25; k.new_feat[(u >= 0.05) & (u < 0.1), 3] = 0.75
    k.opts = OPTS[opts]
    return k


def _ref(k, centre=(0.0, 0.0, 0.0), **over):
    kw = dict(k.opts); kw.update(over)
    return reproject_motion_ref(k.old_cam, k.new_cam, k.film, k.old_feat, k.new_feat, k.hit_face, k.hit_uv, k.face, k.emissive, k.old_v, k.old_n,
                                centre=centre, **kw)


def _erode(mask, by=2):
    out = mask.copy()
    for k in range(1, by + 1):
        out[:, k:] &= mask[:, :-k]; out[:, :-k] &= mask[:, k:]; out[k:] &= mask[:-k]; out[:-k] &= mask[k:]
        out[:, :k] = False; out[:, -k:] = False; out[:k] = False; out[-k:] = False
    return out


# ------------------------------------------------------------------------------------------------------------------------ CPU: the reference alone
def _plain_world(pkg, w, h, kind, cam_b=None, film_seed=11, linear=False):
    """A world without the probe cases' spoiled pixels: full-coverage features of both views, the film everywhere."""
    k = Case()
    k.old_cam = Cam(width=w, height=h, **CAM_A); k.new_cam = cam_b or k.old_cam
    k.scene = _world(pkg, w, h, k.old_cam)
    k.face, k.emissive = k.scene.face, emissive_faces(k.scene)
    k.old_v, k.old_n = k.scene.vertex, k.scene.normal
    k.new_v, k.new_n = _moved(k.scene, kind)
    k.film = synthetic_film(h, w, film_seed, zero_share=0.0)
    if linear:                                                               # a mean that is linear in the pixel coordinates: bilinear taps restore it exactly
        ys, xs = np.mgrid[0:h, 0:w]
        k.film[..., 3] = 12; k.film[..., :3] = (12 * (0.2 + 0.01 * xs + 0.02 * ys))[..., None]
    k.old_feat, k.old_hit, _, _ = view_features(k.old_cam, k.old_v, k.old_n, k.face, k.emissive)
    k.new_feat, k.hit_face, k.hit_uv, _ = view_features(k.new_cam, k.new_v, k.new_n, k.face, k.emissive)
    k.opts = {}
    return k


def test_ref_identity_returns_the_means_with_capped_counts(pkg):
    k = _plain_world(pkg, 37, 23, "identity")
    surface = k.new_feat[..., 3] >= 0.5
    assert (k.hit_face < 0).any() and k.emissive[np.maximum(k.hit_face, 0)].any() and 0.5 < surface.mean() < 1.0
    for cap in (64.0, 8.0):
        out, _ = _ref(k, max_history=cap)                                    # (every pixel lands on an integer: all of them are marginal)
        want = np.where(surface, np.minimum(k.film[..., 3], cap), 0)
        assert np.array_equal(out[..., 3], want)
        # float32 barycentrics place the point within 2^-23 x the triangle's extent in pixels (the 41.7-unit wall: 330) of the pixel centre, so a
        # stray tap weighs under 4e-5 and adds at most that times the largest mean of the film
        means = k.film[..., :3] / np.maximum(k.film[..., 3:], 1)
        np.testing.assert_allclose(out[surface, :3] / out[surface, 3:], means[surface], rtol=1e-6, atol=4e-5 * float(np.nanmax(means)))
        assert np.all(out[~surface] == 0)


def test_ref_scene_and_camera_translated_together_is_the_identity(pkg):
    T = np.array([0.31, -0.17, 0.23])
    cam_b = Cam(np.array(CAM_A["eye"]) + T, np.array(CAM_A["lookat"]) + T, CAM_A["up"], CAM_A["fovy"], 37, 23)
    k = _plain_world(pkg, 37, 23, "translate-all", cam_b)
    ident = _plain_world(pkg, 37, 23, "identity")
    out, _ = _ref(k, max_history=64.0)
    want, _ = _ref(ident, max_history=64.0)
    assert np.array_equal(out[..., 3], want[..., 3]) and (want[..., 3] > 0).mean() > 0.5
    np.testing.assert_allclose(out[..., :3], want[..., :3], rtol=1e-6, atol=2 * 4e-5 * 64 * 2.0)     # (two stray taps of the identity test's size, sums of <= 64 samples)
    # reprojection by the camera alone takes the scene for static: it looks the surface points up where they never were
    cam_only, _ = reproject_ref(k.old_cam, k.new_cam, k.film, k.old_feat, k.new_feat, max_history=64.0)
    assert (cam_only[..., 3] != want[..., 3]).mean() > 0.5


def test_ref_a_quad_moving_in_front_of_a_static_wall(pkg):
    w, h = 70, 44
    k = _plain_world(pkg, w, h, "lateral", linear=True)
    out, _ = _ref(k, max_history=64.0)
    quad = np.isin(np.arange(k.face.shape[0]), (2, 3))
    was_quad, is_quad = quad[np.maximum(k.old_hit, 0)] & (k.old_hit >= 0), quad[np.maximum(k.hit_face, 0)] & (k.hit_face >= 0)
    wall = np.isin(k.hit_face, (0, 1))
    # the strip the quad uncovered is wall the old view never saw: empty (pixels next to a border prove nothing either way)
    strip = _erode(wall & was_quad, 1)
    assert strip.sum() >= 20 and np.all(out[strip] == 0)
    # the quad carries its film from where it was: a shift by (0.237, 0.051) world units, seen from 3 + units away by an orthonormal camera
    c = camera_constants(k.old_cam)
    px = h / (c["h"] * ((QUAD_C - c["eye"]) @ c["front"]))                   # pixels per world unit at the quad's distance along the view axis
    ys, xs = np.mgrid[0:h, 0:w]
    inner = _erode(is_quad, 4) & _erode(was_quad | ~is_quad, 0)
    inner &= np.roll(_erode(was_quad, 2), (1, 3), (0, 1))                    # the source is inside the old quad as well
    assert inner.sum() >= 50 and np.all(out[inner, 3] == 12)
    right, up = c["right"], np.cross(c["right"], c["front"])
    dx, dy = (np.array([0.237, 0.051, 0.0]) @ right) * px, (np.array([0.237, 0.051, 0.0]) @ up) * px
    assert abs(dx - round(dx)) > 0.1 and 2 < dx < 6
    want = 0.2 + 0.01 * (xs - dx) + 0.02 * (ys - dy)
    # (the camera looks slightly off-axis, so the quad is not exactly parallel to its image plane: the shift varies by a few 1e-3 pixel over it)
    np.testing.assert_allclose(out[inner, 0] / 12, want[inner], atol=2e-3)
    # wall that was wall before and after keeps its film
    same = _erode(wall & ~was_quad & np.isin(k.old_hit, (0, 1)), 1)
    assert same.sum() >= 0.4 * w * h and np.all(out[same, 3] == 12)
    np.testing.assert_allclose(out[same, :3], k.film[same, :3], rtol=1e-5)


def test_ref_a_rotating_quad_keeps_its_history(pkg):
    k = _plain_world(pkg, 74, 46, "rotate")
    is_quad = np.isin(k.hit_face, (2, 3))
    out, _ = _ref(k, max_history=64.0)
    inner = _erode(is_quad, 3)
    assert inner.sum() >= 50 and np.all(out[inner, 3] > 0)
    # ... which a comparison with the NEW normal would lose: cos 30 deg = 0.866 is below the default threshold 0.9
    lost, _ = reproject_motion_ref(k.old_cam, k.new_cam, k.film, k.old_feat, k.new_feat, k.hit_face, k.hit_uv, k.face, k.emissive, k.old_v, k.new_n,
                                   max_history=64.0)
    assert np.all(lost[is_quad, 3] == 0)
    assert np.array_equal(lost[~is_quad], out[~is_quad])


@pytest.mark.parametrize("case", PROBE_CASES, ids=lambda c: "%dx%d-%s-%s" % (c[0][0], c[0][1], c[1], c[2]))
def test_marginal_share_of_the_synthetic_inputs(case):
    k = _probe_case(*case)
    out, marg = _ref(k)
    reused = out[..., 3] > 0
    print("[synthetic] %s: %d of %d pixels reused, %d marginal" % (case, int(reused.sum()), reused.size, int(marg.sum())))
    assert marg.mean() <= 0.02
    lamp = k.emissive[np.maximum(k.hit_face, 0)] & (k.hit_face >= 0)
    if reused.size > 1:
        assert 0.2 < reused.mean() < 0.98                                    # both outcomes are exercised
        assert lamp.any() and (k.hit_face < 0).any()                         # a hit on the emitter and a miss, with live features
        assert np.all(k.new_feat[lamp | (k.hit_face < 0), 3] >= 0.25)
        assert np.all(out[lamp | (k.hit_face < 0)] == 0)
    else:
        assert reused.all()


# ------------------------------------------------------------------------------------------------------------------------ GPU helpers
W = H = kit.CORNELL_SIZE


def _centre_rays(r):
    ys, xs = np.mgrid[0:r.height, 0:r.width]
    xy = np.stack([xs.ravel(), ys.ravel()], -1).astype(np.int32)
    return r.probe_cast_ray(xy, np.full((xy.shape[0], 2), 0.5, np.float32)).astype(np.float64)


def _trace4(r, rays):
    t, f, u, v = r.probe_trace4(rays[:, :3], rays[:, 3:])
    return np.concatenate([bits(t), f.view(np.uint32), bits(u), bits(v)])


def _own_tap_passes(r, scene, feat, depth_tolerance=0.05, normal_threshold=0.9):
    """For an update that leaves every surface point on its own pixel the gather has one tap of weight ~1: the pixel itself.  The kernel keeps a
    pixel exactly when (1) its features are alive, (2) its centre ray hits a non-emitter, and that tap passes (3) the depth test, feature depth
    against the hit distance, and (4) the normal test, feature normal against the hit's camera-facing shading normal.  Silhouette pixels, whose
    features average the object and what lies behind it, fail (3) or (4) and come back empty.  Returns (kept, undecided): undecided pixels are
    within 1e-3 of a threshold (the restatement's margin, widened for load_hit_shade's fp32 normal)."""
    face, uvt = r.probe_first_hits()
    rays = _centre_rays(r).reshape(r.height, r.width, 6)
    nn = (feat[..., 4:7] ** 2).sum(-1)
    alive = (feat[..., 3] >= 0.5) & (feat[..., 7] > 0) & (nn > 0)
    hit = (face >= 0) & ~emissive_faces(scene)[np.maximum(face, 0)]
    ns = shading_normals(scene.normal, scene.face, face, uvt[..., :2], rays[..., 3:])
    t = uvt[..., 2].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dz = np.abs(feat[..., 7] - t) / t
        cos = (feat[..., 4:7] * ns).sum(-1) / np.sqrt(nn)
    kept = alive & hit & (dz <= depth_tolerance) & (cos >= normal_threshold)
    undecided = alive & hit & ((np.abs(dz - depth_tolerance) <= 1e-3 * depth_tolerance) | (np.abs(cos - normal_threshold) <= 1e-3))
    return kept, undecided


def _assert_carried_over_in_place(out, film, kept, undecided, count):
    """Counts `count` on every kept pixel, zero elsewhere; each mean within 1e-3 x the largest old mean of its 3x3 neighbourhood (fp32
    barycentrics place the point within 2^-23 x the triangle's extent in pixels (<= 64) of the pixel centre, so a stray tap weighs under 1e-5;
    1e-3 is a hundredfold margin over that)."""
    sure = ~undecided
    assert 0.5 < kept.mean() < 1.0 and undecided.mean() <= 0.02
    assert np.all(out[kept & sure, 3] == count) and np.all(out[~kept & sure] == 0)
    means = film[..., :3] / np.maximum(film[..., 3:], 1)
    big = np.zeros(means.shape[:2])
    pad = np.pad(means.max(-1), 1)
    for dy in range(3):
        for dx in range(3):
            big = np.maximum(big, pad[dy:dy + means.shape[0], dx:dx + means.shape[1]])
    m = kept & sure
    err = np.abs(out[m, :3] / count - means[m]).max(-1)
    print("[in place] kept %d, undecided %d, largest mean error / bound %.3g" % (int(m.sum()), int(undecided.sum()), float((err / (1e-3 * big[m])).max())))
    assert np.all(err <= 1e-3 * big[m])


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_probe_first_hits_against_the_trace_probe(pkg):
    scene, r = kit.cornell(pkg, dynamic=False)
    rays = _centre_rays(r)
    face, uvt = r.probe_first_hits()
    t, f, u, v = r.probe_trace(rays[:, :3], rays[:, 3:])
    r.close()
    face, uvt = face.ravel(), uvt.reshape(-1, 3)
    assert 0.5 < (f >= 0).mean() and np.array_equal(face, f)
    hit = f >= 0
    # tests/test_gpu_parity.py _same_numbers: what it allows between its two trace probes
    assert np.allclose(uvt[hit, 2], t[hit], rtol=4e-6, atol=1e-7), np.abs(uvt[hit, 2] - t[hit]).max()
    assert np.allclose(uvt[hit, 0], u[hit], rtol=0, atol=4e-6) and np.allclose(uvt[hit, 1], v[hit], rtol=0, atol=4e-6)
    assert np.all(uvt[~hit] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PROBE_CASES, ids=lambda c: "%dx%d-%s-%s" % (c[0][0], c[0][1], c[1], c[2]))
def test_probe_matches_the_reference(pkg, case):
    k = _probe_case(*case)
    r = pkg.Renderer(k.scene, max_depth=2, flags=pkg.FLAG_DYNAMIC)
    centre = tuple(r.info().centre)
    got, reused = r.probe_reproject_motion(k.old_cam, k.new_cam, k.film, k.old_feat, k.new_feat, k.hit_face, k.hit_uv, old_vertex=k.old_v,
                                           old_normal=k.old_n, **k.opts)
    own, own_reused = r.probe_reproject_motion(k.old_cam, k.new_cam, k.film, k.old_feat, k.new_feat, k.hit_face, k.hit_uv, **k.opts)   # NULL = the context's
    bad = k.hit_face.copy(); bad.flat[0] = k.face.shape[0]
    with pytest.raises(pkg.McptError) as e:
        r.probe_reproject_motion(k.old_cam, k.new_cam, k.film, k.old_feat, k.new_feat, bad, k.hit_uv)
    assert "status 1" in str(e.value)
    nan = k.hit_uv.copy(); nan.flat[1] = np.nan
    with pytest.raises(pkg.McptError) as e:
        r.probe_reproject_motion(k.old_cam, k.new_cam, k.film, k.old_feat, k.new_feat, k.hit_face, nan)
    assert "status 1" in str(e.value)
    r.close()
    want, marg = _ref(k, centre=centre)
    assert reused == int((got[..., 3] > 0).sum())
    compare_with_ref(got, reused, want, marg)
    assert np.array_equal(bits(own), bits(got)) and own_reused == reused    # the context was created from the old arrays
    out_of_scene = (k.hit_face < 0) | k.emissive[np.maximum(k.hit_face, 0)]
    assert np.all(got[out_of_scene] == 0)


@pytest.mark.gpu
def test_identity_update_keeps_the_surface_pixels(pkg):
    scene, r = kit.cornell(pkg, dynamic=True)
    r.render(16, seed=3)
    film = r.read_accum()
    for cap, count in ((64.0, 16.0), (8.0, 8.0)):
        r.write_accum(film)
        r.update_vertices_reproject(scene.vertex, scene.normal, feature_spp=4, feature_seed=SEED_F, max_history=cap)
        out = r.read_accum(); feat = r.features()
        kept, undecided = _own_tap_passes(r, scene, feat)
        _assert_carried_over_in_place(out, film, kept, undecided, count)
        info = r.reproject_info()
        assert abs(int(info.pixels_reused) - int(kept.sum())) <= int(undecided.sum()) and info.last_ms > 0
        assert info.pixels_reused == int((out[..., 3] > 0).sum())
    assert r.reproject_info().reprojections == 2 and r.update_info().updates == 2
    r.close()


@pytest.mark.gpu
def test_scene_and_camera_translated_together(pkg):
    scene, r = kit.cornell(pkg, dynamic=True)
    T = np.array([0.0625, -0.03125, 0.125])
    cam = scene.camera
    cam_b = pkg.scenes.Camera(tuple(np.array(cam.eye) + T), tuple(np.array(cam.lookat) + T), cam.up, cam.fovy, W, H)
    moved = kit.with_arrays(pkg, scene, scene.vertex + T, camera=cam_b)
    r.render(16, seed=3)
    film = r.read_accum()
    for cap, count in ((64.0, 16.0), (8.0, 8.0)):
        r.update_vertices(scene.vertex); r.set_camera(cam)
        r.write_accum(film)
        r.update_vertices_reproject(moved.vertex, None, camera=cam_b, feature_spp=4, feature_seed=SEED_F, max_history=cap)
        out = r.read_accum(); feat = r.features()
        kept, undecided = _own_tap_passes(r, moved, feat)
        _assert_carried_over_in_place(out, film, kept, undecided, count)
    r.close()


@pytest.mark.gpu
def test_a_moved_sphere_matches_the_reference(pkg):
    scene, r = kit.cornell(pkg, dynamic=True)
    moved = kit.moved_sphere(pkg, scene)
    centre = tuple(r.info().centre)
    r.render(16, seed=3); r.render_features(4, seed=SEED_F)
    film, feat_a = r.read_accum(), r.features()
    hit_a, _ = r.probe_first_hits()
    r.update_vertices_reproject(moved.vertex, moved.normal, feature_spp=4, feature_seed=SEED_F, max_history=64.0)
    got, feat_b = r.read_accum(), r.features()
    hit_b, uvt_b = r.probe_first_hits()
    info = r.reproject_info()
    r.close()
    want, marg = reproject_motion_ref(scene.camera, scene.camera, film, feat_a, feat_b, hit_b, uvt_b[..., :2], scene.face, emissive_faces(scene),
                                      scene.vertex, scene.normal, max_history=64.0, centre=centre, whole_pixel_margin=1e-11)
    # (the camera is fixed and the room at rest: every wall point lands on its own pixel centre, see whole_pixel_margin)
    print("[moved sphere] %d of %d pixels reused, %d marginal" % (int((want[..., 3] > 0).sum()), W * H, int(marg.sum())))
    assert (want[..., 3] > 0).mean() >= 0.5 and marg.mean() <= 0.02
    compare_with_ref(got, info.pixels_reused, want, marg)
    # wall before and after, never under the sphere (nor next to a pixel that was): the count stays
    sphere = scene.face[:, 0, 3] == 4
    under = (sphere[np.maximum(hit_a, 0)] & (hit_a >= 0)) | (sphere[np.maximum(hit_b, 0)] & (hit_b >= 0))
    light = emissive_faces(scene)
    room = (hit_a >= 0) & (hit_b >= 0) & ~light[np.maximum(hit_a, 0)] & ~light[np.maximum(hit_b, 0)]
    clear = _erode(~under & room & (feat_a[..., 3] == 1) & (feat_b[..., 3] == 1), 1)
    # ... and inside one wall: where two walls meet the features average both normals, and the tap fails the test against the hit's own normal
    wall = hit_b // 2                                                        # two triangles per wall
    inside = np.ones_like(clear)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inside &= np.roll(wall, (dy, dx), (0, 1)) == wall
    clear &= inside
    assert clear.mean() > 0.3 and np.all(got[clear, 3] == 16)
    # the sphere took its film along
    on = _erode(sphere[np.maximum(hit_b, 0)] & (hit_b >= 0), 2)
    assert on.sum() >= 50 and (got[on, 3] > 0).mean() > 0.8


@pytest.mark.gpu
def test_state_after_the_call(pkg):
    scene, r = kit.cornell(pkg, dynamic=True)
    moved = kit.moved_sphere(pkg, scene)
    _, plain = kit.cornell(pkg, dynamic=True)
    _, fresh = kit.cornell(pkg, dynamic=False, scene=moved)
    n = W * H; nvn = scene.vertex.shape[0] + scene.normal.shape[0]
    r.render(4, seed=3)
    b0 = r.info().device_bytes
    r.update_vertices_reproject(moved.vertex, moved.normal, feature_spp=3, feature_seed=SEED_F)
    b1 = r.info().device_bytes
    assert b1 - b0 == (48 + 32 + 16) * n + 24 * nvn                          # the context never had features
    assert r.update_info().updates == 1 and r.reproject_info().reprojections == 1
    fresh.render_features(3, seed=SEED_F)
    assert np.array_equal(bits(r.features()), bits(fresh.features()))
    den = r.denoise()                                                        # at once, without a render_features call
    assert den.shape == (H, W, 4) and np.isfinite(den).all()
    r.validate_trees()
    plain.update_vertices(moved.vertex, moved.normal)
    rays = _centre_rays(plain)
    assert np.array_equal(_trace4(r, rays), _trace4(plain, rays))
    r.clear(); r.render(4, seed=9); plain.render(4, seed=9)
    assert np.array_equal(bits(r.read_accum()), bits(plain.read_accum()))
    paths = r.counters().paths; b2 = r.info().device_bytes
    r.update_vertices_reproject(scene.vertex, scene.normal)
    assert r.info().device_bytes == b2 and r.counters().paths == paths      # the second call allocates nothing
    assert r.update_info().updates == 2 and r.reproject_info().reprojections == 2
    with pytest.raises(pkg.McptError):
        r.denoised_device_ptr()                                              # describes the old scene
    clone = r.clone(0)
    assert clone.reproject_info().reprojections == 0
    cb0 = clone.info().device_bytes
    clone.render_features(4, seed=SEED_F)
    clone.update_vertices_reproject(moved.vertex, moved.normal)              # a clone starts without the buffers -- and with the current vertices
    assert clone.info().device_bytes - cb0 == (32 + 48 + 16) * n + 24 * nvn
    clone.close(); fresh.close(); plain.close(); r.close()
    # a context that had features: 48 + 16 B per pixel and the old arrays
    _, r2 = kit.cornell(pkg, dynamic=True)
    r2.render(4, seed=3); r2.render_features(4, seed=SEED_F)
    b0 = r2.info().device_bytes
    r2.update_vertices_reproject(moved.vertex, moved.normal)
    assert r2.info().device_bytes - b0 == (48 + 16) * n + 24 * nvn
    r2.close()


@pytest.mark.gpu
def test_ordering_without_synchronisation_and_a_bound_film(pkg):
    import torch
    scene, a = kit.cornell(pkg, dynamic=True)
    _, b = kit.cornell(pkg, dynamic=True)
    moved = kit.moved_sphere(pkg, scene)
    t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    a.bind_accum(t.data_ptr())
    a.render(4, seed=3)
    a.update_vertices_reproject(moved.vertex, moved.normal, feature_seed=SEED_F, max_history=16.0)
    a.render(4, seed=3, first_sample=4)
    b.render(4, seed=3); b.sync()
    b.update_vertices_reproject(moved.vertex, moved.normal, feature_seed=SEED_F, max_history=16.0); b.sync()
    b.render(4, seed=3, first_sample=4); b.sync()
    a.sync()
    fa, fb = t.cpu().numpy(), b.read_accum()
    a.bind_accum(0)
    own = a.read_accum()
    a.close(); b.close()
    assert (fa[..., 3] > 4).mean() > 0.5
    assert np.array_equal(bits(fa), bits(fb))
    assert np.all(own == 0)                                                  # the context's own film was never written


@pytest.mark.gpu
def test_refusals_change_nothing(pkg):
    scene, r = kit.cornell(pkg, dynamic=True)
    _, static = kit.cornell(pkg, dynamic=False)
    moved = kit.moved_sphere(pkg, scene)
    cam = scene.camera
    good = Cam((0.55, 0.5, 2.2), cam.lookat, cam.up, cam.fovy, W, H)
    nan = float("nan")

    def snapshot(x):
        rays = _centre_rays(x)
        return [bits(rays), bits(x.read_accum()), bits(x.features()), _trace4(x, rays)]

    def unchanged(x, before):
        for p, q in zip(snapshot(x), before):
            assert np.array_equal(p, q)

    for x in (r, static):
        x.render(4, seed=3); x.render_features(4, seed=SEED_F)
    before, before_static = snapshot(r), snapshot(static)
    with pytest.raises(pkg.McptError) as e:
        static.update_vertices_reproject(moved.vertex, moved.normal)
    assert "status %d" % UNSUPPORTED in str(e.value)
    unchanged(static, before_static)
    static.close()
    v_nan = moved.vertex.copy(); v_nan[int(scene.face[0, 0, 0]), 1] = nan
    bad_calls = [dict(vertex=v_nan, normal=moved.normal), dict(vertex=moved.vertex[:-1], normal=moved.normal),
                 dict(vertex=moved.vertex, normal=moved.normal[:-1]),
                 dict(vertex=moved.vertex, normal=moved.normal, camera=Cam(good.eye, good.lookat, good.up, good.fovy, W + 1, H)),
                 dict(vertex=moved.vertex, normal=moved.normal, camera=Cam(good.eye, good.eye, good.up, good.fovy, W, H)),
                 dict(vertex=moved.vertex, normal=moved.normal, camera=Cam((nan, 0.5, 2.3), good.lookat, good.up, good.fovy, W, H))]
    bad_calls += [dict(vertex=moved.vertex, normal=moved.normal, camera=good, **kw) for kw in (
        dict(feature_spp=65), dict(max_history=nan), dict(max_history=0.5), dict(depth_tolerance=1.5), dict(normal_threshold=-0.5))]
    for kw in bad_calls:
        with pytest.raises(pkg.McptError) as e:
            r.update_vertices_reproject(**kw)
        assert "status %d" % INVALID in str(e.value), kw
        unchanged(r, before)
    v = np.ascontiguousarray(moved.vertex); vp = v.ctypes.data_as(C.c_void_p)
    o = pkg.ReprojectOpts(); o.struct_size = C.sizeof(pkg.ReprojectOpts) - 4
    assert r.lib.mcpt_update_vertices_reproject(r.ctx, vp, v.shape[0], None, 0, None, C.byref(o)) == INVALID
    assert r.lib.mcpt_update_vertices_reproject(r.ctx, None, v.shape[0], None, 0, None, None) == INVALID
    unchanged(r, before)
    assert r.reproject_info().reprojections == 0 and r.update_info().updates == 0
    assert r.lib.mcpt_update_vertices_reproject(r.ctx, vp, v.shape[0], None, 0, None, None) == 0       # NULL normals, camera, opts: keep / defaults
    assert r.reproject_info().reprojections == 1 and r.update_info().updates == 1
    assert not np.array_equal(_trace4(r, _centre_rays(r)), before[3])
    r.close()


@pytest.mark.gpu
def test_facade_update_reproject(pkg, tmp_path):
    exe = kit.build_facade("facade_update_reproject.cpp", tmp_path)
    w, h, k, cap = 44, 30, 6, 4
    a = pkg.scenes.cornell_box_small(w, h)
    cam = a.camera
    b = kit.with_arrays(pkg, kit.moved_sphere(pkg, a), camera=pkg.scenes.Camera((0.56, 0.5, 2.25), cam.lookat, cam.up, cam.fovy, w, h))
    obj_a = a.write(str(tmp_path / "a")); obj_b = b.write(str(tmp_path / "b"))
    outs = [str(tmp_path / n) for n in ("before.bin", "same.bin", "moved.bin", "final.bin")]
    line = kit.run_facade(exe, [obj_a, obj_b, str(k), str(cap)] + outs)
    assert [int(x) for x in line[:3]] == [w, h, k]
    before, same, moved, final = [np.fromfile(p, np.float32).reshape(h, w, 4) for p in outs]
    assert np.all(before[..., 3] == k)
    kept = same[..., 3] > 0
    assert 0.5 < kept.mean() < 1.0 and int(line[3]) == int(kept.sum())     # (the uploaded film and the device film reuse the same pixels)
    assert np.all(same[kept, 3] == cap) and np.all(same[~kept] == 0)
    # the identity update lands every point within 2^-23 x 44 pixels of its own pixel centre (fp32 barycentrics): see _assert_carried_over_in_place
    means = before[..., :3] / k
    assert np.all(np.abs(same[kept, :3] / cap - means[kept]) <= 1e-3 * float(means.max()))
    assert (moved[..., 3] > 0).mean() > 0.5 and moved[..., 3].max() == cap
    assert np.array_equal(final[..., 3], moved[..., 3] + k)                # the next frames add to the history


@pytest.mark.gpu
def test_cli_wobble_reproject(pkg, tmp_path):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    base = [obj, "--turntable", "3", "--spp", "4", "--depth", "5", "--deterministic"]
    still, plain, carried = str(tmp_path / "still"), str(tmp_path / "plain"), str(tmp_path / "carried")
    for extra in (["--out", still], ["--out", plain, "--wobble", "0.01"], ["--out", carried, "--wobble", "0.01", "--reproject", "32"]):
        p = kit.run_cli(base + extra)
        assert p.returncode == 0, p.stderr[-2000:]

    s, p, c = kit.turntable_frames(still), kit.turntable_frames(plain), kit.turntable_frames(carried)
    assert s[0] == p[0] == c[0]                                              # frame 0 is the run without the flags
    assert p[1] != s[1] and c[1] != p[1] and c[2] != p[2]                    # the vertices moved; the film was carried over
    p = kit.run_cli([obj, "--spp", "4", "--wobble", "0.01", "--out", str(tmp_path / "no")])
    assert p.returncode == 2
