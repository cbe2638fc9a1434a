"""Live scenes: mcpt_set_camera, mcpt_update_vertices (csrc/refit.hip: the triangle streams and light records rewritten, both
trees refitted on the device), mcpt_get_update_info, mcpt_probe_validate_trees and their public surfaces.

Closest hit and any hit do not depend on the tree, so the oracle of a moved context is this library's own fresh mcpt_create of the moved scene:
bit for bit where both round about the same centre, within the device-builder test's tolerances where the bounding box moves too.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

from tests import kit, ploc_ref
from tests.kit import bits, render_film

NEW_SYMBOLS = ["mcpt_set_camera", "mcpt_update_vertices", "mcpt_get_update_info", "mcpt_probe_validate_trees"]
INVALID, UNSUPPORTED = 1, 6


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_update_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS)
    assert pkg.FLAG_DYNAMIC == 0x20


def test_null_context_is_an_invalid_argument_for_the_update_calls(pkg):
    lib = pkg.load_library()
    cam = pkg.CameraC(); info = pkg.UpdateInfo()
    v = np.zeros((4, 3)); vp = v.ctypes.data_as(C.c_void_p)
    assert lib.mcpt_set_camera(None, C.byref(cam)) == INVALID
    assert lib.mcpt_update_vertices(None, vp, 4, None, 0) == INVALID
    assert lib.mcpt_get_update_info(None, C.byref(info)) == INVALID
    assert lib.mcpt_probe_validate_trees(None) == INVALID


# ------------------------------------------------------------------------------------------------------------------------ GPU helpers
def _rays(pkg, r, scene, n_box=3000, seed=3):
    """The scene's own camera rays and random rays through its bounding box."""
    cam = scene.camera
    _, _, od = kit.camera_rays(r, cam.width, cam.height, 1)
    o, d = kit.box_rays(*kit.used_bounds(scene), n_box, seed)
    return np.concatenate([od[:, :3], o]), np.concatenate([od[:, 3:], d])


def _same_render(a, b):
    """The criteria of tests/test_gpu_bvh_build.py::test_device_and_host_trees_render_the_same_samples between two trees of one scene."""
    assert np.array_equal(a[..., 3], b[..., 3])
    differ = np.any(a[..., :3] != b[..., :3], axis=-1)
    assert differ.mean() <= 0.01, differ.mean()
    assert abs(a[..., :3].mean() - b[..., :3].mean()) <= 2e-3 * a[..., :3].mean()


def _tri_t64(scene, face, o, d):
    """fp64 distance along ray (o, d) to the plane point of `face` (Moeller-Trumbore), one ray."""
    p = scene.vertex[scene.face[face, :, 0]]
    e1, e2 = p[1] - p[0], p[2] - p[0]
    pv = np.cross(d, e2); det = e1 @ pv
    tv = o - p[0]; qv = np.cross(tv, e1)
    return float(e2 @ qv / det)


def _compare_traces(pkg, R, F, moved, probe="probe_trace4", exact=True, rays=None):
    o, d = rays or _rays(pkg, F, moved)
    tr, fr, _, _ = getattr(R, probe)(o, d); tf, ff, _, _ = getattr(F, probe)(o, d)
    assert (ff >= 0).mean() > 0.3
    hit = ff >= 0
    if exact:
        assert np.array_equal(fr >= 0, ff >= 0)
        assert np.array_equal(bits(tr[hit]), bits(tf[hit]))
        # another face only between exact ties (the two trees' leaf orders differ, and with them the tie ranks): wherever the faces differ the
        # ray meets both at the same distance, up to what fp32 can tell apart
        for i in np.flatnonzero(hit & (fr != ff)):
            a, b = _tri_t64(moved, fr[i], o[i], d[i]), _tri_t64(moved, ff[i], o[i], d[i])
            assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (i, fr[i], ff[i], a, b)
    else:
        # the two contexts round their fp32 records about different centres: a ray that grazes a silhouette may hit in one and miss in the other,
        # so "hit/miss equal and t within the device-builder test's tolerance" is asked of at least 99.9 % of the rays, as that test asks it
        ok = (fr >= 0) == hit
        ok[hit] &= np.isclose(tr[hit], tf[hit], rtol=2e-5, atol=2e-6)
        print("[moved box] %s: %d of %d rays agree (hit/miss and t)" % (probe, int(ok.sum()), ok.size))
        assert ok.mean() >= 0.999, ok.mean()
    t2 = np.where(hit, tf * 0.999, 1e30).astype(np.float64)             # shadow rays that stop just short of the closest hit, and open ones
    t2[::2] = 1e30
    if probe == "probe_trace4":
        ar = R.probe_trace4(o, d, t2=t2, any_hit=True)[1]; af = F.probe_trace4(o, d, t2=t2, any_hit=True)[1]
    else:
        ar = R.probe_trace(o, d, t2=t2, any_hit=True)[1]; af = F.probe_trace(o, d, t2=t2, any_hit=True)[1]
    if exact:
        assert np.array_equal(ar, af)
    else:
        assert (ar == af).mean() >= 0.999


# ------------------------------------------------------------------------------------------------------------------------ GPU
W, H = 68, 52


@pytest.mark.gpu
def test_set_camera_equals_a_context_created_with_that_camera(pkg):
    sa = pkg.scenes.cornell_box_small(W, H)
    cam_b = pkg.scenes.Camera((0.9, 0.7, 1.9), (0.4, 0.35, 0.1), (0.0, 1.0, 0.0), 52.0, W, H)
    sb = kit.with_arrays(pkg, sa, camera=cam_b)
    fl = pkg.FLAG_DETERMINISTIC                                            # (no FLAG_DYNAMIC: the camera moves on every context)
    r = pkg.Renderer(sa, max_depth=8, flags=fl); fresh = pkg.Renderer(sb, max_depth=8, flags=fl)
    film_a = render_film(r, 8, 5)
    r.render_features(4, seed=5); r.features()
    # refusals change nothing
    for bad in (pkg.scenes.Camera(cam_b.eye, cam_b.lookat, cam_b.up, 52.0, W + 1, H), pkg.scenes.Camera(cam_b.eye, cam_b.lookat, cam_b.up, 52.0, W, H - 1),
                pkg.scenes.Camera(cam_b.eye, cam_b.eye, cam_b.up, 52.0, W, H), pkg.scenes.Camera((float("nan"), 0.7, 1.9), cam_b.lookat, cam_b.up, 52.0, W, H),
                pkg.scenes.Camera(cam_b.eye, cam_b.lookat, cam_b.up, float("inf"), W, H)):
        with pytest.raises(pkg.McptError) as e:
            r.set_camera(bad)
        assert "status 1" in str(e.value)
    assert r.lib.mcpt_set_camera(r.ctx, None) == INVALID
    assert np.array_equal(bits(render_film(r, 8, 5)), bits(film_a))
    r.features()                                                           # still there after the refused calls
    r.set_camera(cam_b)
    with pytest.raises(pkg.McptError):
        r.features()                                                       # gone, as on a clone
    with pytest.raises(pkg.McptError):
        r.denoise()
    xy, xi, rays = kit.camera_rays(r, W, H, 1)
    assert np.array_equal(bits(rays.astype(np.float32)), bits(fresh.probe_cast_ray(xy, xi)))
    film_b = render_film(fresh, 8, 5)
    assert not np.array_equal(film_a, film_b)
    assert np.array_equal(bits(render_film(r, 8, 5)), bits(film_b))
    assert r.update_info().updates == 0 and r.update_info().wide_area_ratio == 1.0
    r.close(); fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_tree", [False, True])
def test_update_with_the_creation_vertices_is_the_identity(pkg, gpu_tree):
    scene = pkg.scenes.cornell_box_small(W, H)
    fl = pkg.FLAG_DETERMINISTIC | pkg.FLAG_DYNAMIC | pkg.FLAG_COUNT_TRAVERSAL | (pkg.FLAG_GPU_BVH_BUILD if gpu_tree else 0)
    r = pkg.Renderer(scene, max_depth=8, flags=fl)
    r.validate_trees()
    o, d = _rays(pkg, r, scene)
    t2 = np.full(o.shape[0], 0.8)
    before = r.probe_trace4(o, d); before_any = r.probe_trace4(o, d, t2=t2, any_hit=True)[1]
    r.reset_counters()
    film = render_film(r, 8, 5)
    c0 = r.counters(); work0 = c0.box_tests + c0.tri_tests
    assert work0 > 0
    lp, lxi = kit.light_points(*kit.used_bounds(scene), 500, 2)
    lights = r.probe_sample_light(lp, lxi)
    for normal in (None, scene.normal):
        r.update_vertices(scene.vertex, normal)
        r.validate_trees()
        after = r.probe_trace4(o, d)
        for a, b in zip(before, after):
            assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
        assert np.array_equal(before_any, r.probe_trace4(o, d, t2=t2, any_hit=True)[1])
        assert np.array_equal(bits(lights), bits(r.probe_sample_light(lp, lxi)))
        r.reset_counters()
        assert np.array_equal(bits(render_film(r, 8, 5)), bits(film))
        c1 = r.counters(); work1 = c1.box_tests + c1.tri_tests
        info = r.update_info()
        print("[identity] gpu_tree=%s normals=%s  traversal work after / before = %.6f  wide_area_ratio = %.8f  update %.3f ms" % (
            gpu_tree, normal is not None, work1 / work0, info.wide_area_ratio, info.last_update_ms))
        # not a measurement: a refitted box exceeds the built one only by padding a padded box again (~1e-6 relative per level)
        assert work1 <= 1.01 * work0
        assert abs(info.wide_area_ratio - 1.0) <= 1e-3
    assert r.update_info().updates == 2
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["host", "device", "recursive"])
def test_moved_geometry_same_bounding_box(pkg, which):
    scene = pkg.scenes.cornell_box(W, H, sphere_lon=24, sphere_lat=12)
    moved = kit.moved_sphere(pkg, scene)
    kw = dict(max_depth=8)
    fl = pkg.FLAG_DETERMINISTIC | (pkg.FLAG_GPU_BVH_BUILD if which == "device" else 0)
    if which == "recursive":
        kw["integrator"] = pkg.INTEGRATOR_RECURSIVE_NEE
    R = pkg.Renderer(scene, flags=fl | pkg.FLAG_DYNAMIC, **kw); F = pkg.Renderer(moved, flags=fl, **kw)
    assert list(R.info().centre) == list(F.info().centre)
    R.update_vertices(moved.vertex, moved.normal)
    R.validate_trees()
    if which != "recursive":
        _compare_traces(pkg, R, F, moved, "probe_trace4")
    _compare_traces(pkg, R, F, moved, "probe_trace")                       # the binary tree
    lp, lxi = kit.light_points(*kit.used_bounds(moved), 2000, 4)
    assert np.array_equal(bits(R.probe_sample_light(lp, lxi)), bits(F.probe_sample_light(lp, lxi)))
    _same_render(render_film(R, 16, 21), render_film(F, 16, 21))
    info = R.update_info()
    print("[moved] %s  wide_area_ratio = %.4f  update %.3f ms" % (which, info.wide_area_ratio, info.last_update_ms))
    assert info.updates == 1 and info.last_update_ms > 0
    R.close(); F.close()


@pytest.mark.gpu
def test_there_and_back(pkg):
    scene = pkg.scenes.cornell_box(W, H, sphere_lon=24, sphere_lat=12)
    moved = kit.moved_sphere(pkg, scene)
    r = pkg.Renderer(scene, max_depth=8, flags=pkg.FLAG_DETERMINISTIC | pkg.FLAG_DYNAMIC | pkg.FLAG_COUNT_TRAVERSAL)
    r.reset_counters()
    film = render_film(r, 8, 5)
    c0 = r.counters(); work0 = c0.box_tests + c0.tri_tests
    r.update_vertices(moved.vertex, moved.normal)
    r.validate_trees()
    assert not np.array_equal(render_film(r, 8, 5), film)
    r.update_vertices(scene.vertex, scene.normal)
    r.validate_trees()
    r.reset_counters()
    assert np.array_equal(bits(render_film(r, 8, 5)), bits(film))
    c1 = r.counters(); work1 = c1.box_tests + c1.tri_tests
    info = r.update_info()
    print("[there and back] traversal work after / before = %.6f  wide_area_ratio = %.8f" % (work1 / work0, info.wide_area_ratio))
    assert work1 <= 1.01 * work0                                           # the boxes shrink again
    assert abs(info.wide_area_ratio - 1.0) <= 1e-3 and info.updates == 2
    r.close()


@pytest.mark.gpu
def test_moved_geometry_moved_bounding_box(pkg):
    scene = pkg.scenes.veach_mis(64, 36, light_lon=12, light_lat=6, plate_cells=4)
    v = scene.vertex
    ext = (v.max(0) - v.min(0)).max()
    amp = 0.03 * ext                                                        # a few percent of the scene's extent, the lights included
    field = np.stack([np.sin(0.37 * v[:, 1] + 0.21 * v[:, 2]), np.cos(0.29 * v[:, 0] - 0.17 * v[:, 2]), np.sin(0.23 * v[:, 0] + 0.31 * v[:, 1])], -1)
    moved = kit.with_arrays(pkg, scene, v + amp * field + np.array([0.4, -0.25, 0.3]))
    fl = pkg.FLAG_DETERMINISTIC
    R = pkg.Renderer(scene, max_depth=8, flags=fl | pkg.FLAG_DYNAMIC); F = pkg.Renderer(moved, max_depth=8, flags=fl)
    assert list(R.info().centre) != list(F.info().centre)
    centre = list(R.info().centre)
    R.update_vertices(moved.vertex)
    assert list(R.info().centre) == centre                                 # device coordinates stay relative to the creation-time centre
    R.validate_trees()
    _compare_traces(pkg, R, F, moved, "probe_trace4", exact=False)
    lp, lxi = kit.light_points(*kit.used_bounds(moved), 2000, 6)
    a, b = R.probe_sample_light(lp, lxi), F.probe_sample_light(lp, lxi)
    assert np.array_equal(a[:, 8], b[:, 8])                                # the same light triangle
    both = (a[:, 6] > 0) & (b[:, 6] > 0)
    assert both.mean() > 0.2 and ((a[:, 6] > 0) == (b[:, 6] > 0)).mean() >= 0.999
    np.testing.assert_allclose(a[both, 6], b[both, 6], rtol=1e-5)
    fa, fb = render_film(R, 64, 9), render_film(F, 64, 9)
    assert np.array_equal(fa[..., 3], fb[..., 3])
    assert abs(fa[..., :3].mean() - fb[..., :3].mean()) <= 2e-3 * fb[..., :3].mean()
    R.close(); F.close()


@pytest.mark.gpu
def test_update_refusals(pkg):
    scene = pkg.scenes.cornell_box_small(W, H)
    fl = pkg.FLAG_DETERMINISTIC
    plain = pkg.Renderer(scene, max_depth=6, flags=fl); dyn = pkg.Renderer(scene, max_depth=6, flags=fl | pkg.FLAG_DYNAMIC)
    with pytest.raises(pkg.McptError) as e:
        plain.update_vertices(scene.vertex)
    assert "status %d" % UNSUPPORTED in str(e.value)
    film = render_film(dyn, 4, 5)
    nv, nn = scene.vertex.shape[0], scene.normal.shape[0]
    used = int(scene.face[0, 0, 0])
    nan = scene.vertex.copy(); nan[used, 1] = float("nan")
    inf = scene.vertex.copy(); inf[used, 0] = float("inf")
    far = scene.vertex.copy(); far[used, 2] = 1e19
    for v, n in ((scene.vertex[:-1], None), (np.concatenate([scene.vertex, scene.vertex[:1]]), None), (scene.vertex, scene.normal[:-1]), (nan, None), (inf, None),
                 (far, scene.normal)):
        with pytest.raises(pkg.McptError) as e:
            dyn.update_vertices(v, n)
        assert "status %d" % INVALID in str(e.value)
    assert dyn.lib.mcpt_update_vertices(dyn.ctx, None, nv, None, 0) == INVALID
    assert dyn.update_info().updates == 0
    assert np.array_equal(bits(render_film(dyn, 4, 5)), bits(film))
    dyn.validate_trees()
    # what the flag costs: at least the 24 B of indices per triangle, and nothing without it
    ip, idn = plain.info(), dyn.info()
    assert idn.device_bytes - ip.device_bytes >= 24 * ip.n_tris
    again = pkg.Renderer(scene, max_depth=6, flags=fl)
    assert again.info().device_bytes == ip.device_bytes
    assert (idn.n_tris, idn.n_nodes, idn.wide_nodes, idn.wide_tree_hash, idn.traversal_bytes) == (ip.n_tris, ip.n_nodes, ip.wide_nodes, ip.wide_tree_hash, ip.traversal_bytes)
    plain.close(); dyn.close(); again.close()


@pytest.mark.gpu
def test_clone_ordering_and_bookkeeping(pkg):
    scene = pkg.scenes.cornell_box(W, H, sphere_lon=24, sphere_lat=12)
    moved = kit.moved_sphere(pkg, scene); moved2 = kit.moved_sphere(pkg, scene, shift=(-0.1, 0.2, 0.12), squash=0.8)
    fl = pkg.FLAG_DETERMINISTIC | pkg.FLAG_DYNAMIC
    R = pkg.Renderer(scene, max_depth=8, flags=fl)
    R.update_vertices(moved.vertex, moved.normal)
    clone = R.clone()
    film = render_film(R, 8, 5)
    assert np.array_equal(bits(render_film(clone, 8, 5)), bits(film))
    clone.update_vertices(moved2.vertex, moved2.normal)                    # a clone of a dynamic context is dynamic
    clone.validate_trees()
    F2 = pkg.Renderer(moved2, max_depth=8, flags=pkg.FLAG_DETERMINISTIC)
    _same_render(render_film(clone, 16, 21), render_film(F2, 16, 21))
    assert np.array_equal(bits(render_film(R, 8, 5)), bits(film))                 # the source did not move with its clone
    assert clone.update_info().updates == 1 and R.update_info().updates == 1
    clone.close(); F2.close(); R.close()
    # render; clear; update; render with nothing in between, on the default pipeline with one-sample (known-length) jobs: no kernel of the
    # first render may read a half-written stream, none of the second the old one
    A = pkg.Renderer(scene, max_depth=8, flags=pkg.FLAG_DYNAMIC); F = pkg.Renderer(moved, max_depth=8)
    for s in range(6):
        A.render(1, seed=21, first_sample=s)
    A.clear()
    A.update_vertices(moved.vertex, moved.normal)
    for s in range(16):
        A.render(1, seed=21, first_sample=s)
    for s in range(16):
        F.render(1, seed=21, first_sample=s)
    _same_render(A.read_accum(), F.read_accum())
    A.update_vertices(scene.vertex, scene.normal)
    info = A.update_info()
    assert info.updates == 2 and info.last_update_ms > 0
    A.close(); F.close()


@pytest.mark.gpu
def test_facade_set_camera_and_update(pkg, tmp_path):
    exe = kit.build_facade("facade_update.cpp", tmp_path)
    a = pkg.scenes.cornell_box(44, 30, sphere_lon=24, sphere_lat=12)
    b = kit.moved_sphere(pkg, a)
    b = kit.with_arrays(pkg, b, camera=pkg.scenes.Camera((0.8, 0.6, 2.0), (0.45, 0.4, 0.0), (0.0, 1.0, 0.0), 48.0, 44, 30))
    obj_a = a.write(str(tmp_path / "a")); obj_b = b.write(str(tmp_path / "b"))
    outs = [str(tmp_path / n) for n in ("cam_moved.bin", "cam_fresh.bin", "upd_moved.bin", "upd_fresh.bin")]
    k = 5
    line = kit.run_facade(exe, [obj_a, obj_b, str(k)] + outs)
    w, h = int(line[0]), int(line[1])
    assert (w, h, int(line[2])) == (44, 30, k)
    cm, cf, um, uf = [np.fromfile(p, np.float32).reshape(h, w, 4) for p in outs]
    assert np.all(cm[..., 3] == k) and np.all(um[..., 3] == k)              # the sample counts restarted and end at k
    assert np.array_equal(bits(cm), bits(cf))                           # same tree, another camera: the same film
    assert not np.array_equal(cm, um)
    _same_render(um, uf)                                                   # refitted against freshly built: up to exact ties


@pytest.mark.gpu
def test_cli_turntable(pkg, tmp_path):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    out = str(tmp_path / "img")
    p = kit.run_cli([obj, "--turntable", "3", "--spp", "4", "--depth", "5", "--out", out])
    assert p.returncode == 0, p.stderr[-2000:]
    imgs = kit.turntable_frames(out)
    assert imgs[0] != imgs[1] and imgs[1] != imgs[2]


@pytest.mark.gpu
def test_refit_is_faster_than_the_rebuild_it_replaces(pkg):
    """S-bath detail 160 (0.59 M triangles, bench configuration c4), a smooth displacement of its fixtures: device time of mcpt_update_vertices,
    median of 20 after 3 warm-ups, against bvh_build_ms + upload_ms of a fresh MCPT_FLAG_GPU_BVH_BUILD context of the moved scene in the same
    process -- the faster builder, and only part of what mcpt_create costs.  Strictly less is the condition for the feature to exist; the
    measured figures are in DESIGN.md §12 and profiles/refit_probe.json."""
    scene = pkg.scenes.bathroom_stress(64, 36, detail=160, tex_size=16)
    fixtures = np.isin(scene.face[:, 0, 3], (5, 6))                          # ceramic and chrome: the tessellated spheres
    vi = np.unique(scene.face[fixtures][:, :, 0])
    v = scene.vertex.copy()
    p = v[vi]
    v[vi] = p + 0.02 * np.stack([np.sin(9.0 * p[:, 1]), np.sin(7.0 * p[:, 2]), np.sin(8.0 * p[:, 0])], -1)
    moved = kit.with_arrays(pkg, scene, v)
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    ms = []
    for i in range(23):
        R.update_vertices(moved.vertex if i % 2 == 0 else scene.vertex)
        ms.append(R.update_info().last_update_ms)
    R.update_vertices(moved.vertex)
    R.validate_trees()
    ratio = R.update_info().wide_area_ratio
    F = pkg.Renderer(moved, max_depth=6, flags=pkg.FLAG_GPU_BVH_BUILD)
    fi = F.info()
    R.render(4, seed=3); F.render(4, seed=3)
    a, b = R.read_accum(), F.read_accum()
    R.close(); F.close()
    refit = float(np.median(ms[3:])); rebuild = fi.bvh_build_ms + fi.upload_ms
    print("\n[refit] %d triangles: update %.3f ms (median of 20; min %.3f max %.3f) | fresh device build %.1f + upload %.1f = %.1f ms | ratio %.5f | wide_area_ratio %.4f" % (
        fi.n_tris, refit, min(ms[3:]), max(ms[3:]), fi.bvh_build_ms, fi.upload_ms, rebuild, refit / rebuild, ratio))
    assert np.isfinite(a).all() and abs(a[..., :3].mean() - b[..., :3].mean()) <= 0.05 * b[..., :3].mean()
    assert refit > 0 and refit < rebuild


@pytest.mark.gpu
@pytest.mark.parametrize("maker,args", [("lattice_soup", (3,)), ("lattice_soup", (9,)), ("lattice_soup", (257,)), ("coincident", (300,)), ("shells", (150, 1.2))])
def test_refit_of_small_tied_and_deep_device_built_trees(pkg, maker, args):
    """The refit on device-BUILT trees at the sizes no other scene has (tests/ploc_ref.py makes them): one-node levels and a single wide record
    (3 and 9 triangles), a block edge (257), a run of exact ties (300 copies) and a chain 148 deep, kept by this wavefront context.  An update
    with the creation vertices changes no traced bit; after every vertex is scaled by 1.25 about the centre the context equals a fresh one of the
    scaled scene by _compare_traces' criteria for contexts that round on their own."""
    scene = getattr(ploc_ref, maker)(pkg, *args)
    fl = pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD
    os.environ["MCPT_VALIDATE_BVH"] = "1"
    try:
        R = pkg.Renderer(scene, flags=fl)
    finally:
        os.environ.pop("MCPT_VALIDATE_BVH", None)
    assert R.info().bvh_builder == 1
    o, d = ploc_ref.interior_rays(scene, 1500, seed=9)[:2]
    before = R.probe_trace4(o, d)
    R.update_vertices(scene.vertex); R.validate_trees()
    after = R.probe_trace4(o, d)
    assert (before[1] >= 0).mean() > 0.3
    for a, b in zip(before, after):
        assert np.array_equal(bits(a), bits(b))
    lo, hi = kit.used_bounds(scene); c = 0.5 * lo + 0.5 * hi
    moved = kit.with_arrays(pkg, scene, vertex=(scene.vertex - c) * 1.25 + c)
    R.update_vertices(moved.vertex); R.validate_trees()
    os.environ["MCPT_VALIDATE_BVH"] = "1"
    try:
        F = pkg.Renderer(moved, flags=fl)
    finally:
        os.environ.pop("MCPT_VALIDATE_BVH", None)
    assert F.info().bvh_builder == 1
    _compare_traces(pkg, R, F, moved, "probe_trace4", exact=False, rays=ploc_ref.interior_rays(moved, 1500, seed=10)[:2])
    R.close(); F.close()
