"""Tree rebuild of a live context: mcpt_rebuild_trees (csrc/rebuild.hip: the builders' input formed on the device, every leaf-order
stream moved to the new leaf order, the lights renumbered; csrc/rebuild_plan.h: the permutation; scene_build.cpp: build_trees, the one tree path of
mcpt_create and the rebuild), mcpt_get_rebuild_info and their public surfaces.

The yardstick is this library's own fresh mcpt_create of the same geometry, as in tests/test_scene_update.py: where the centre stays, a rebuilt
context IS that fresh context, bit for bit.  The rebuilt context is compared with itself only where "nothing changed" is the claim.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import subprocess
import time

import numpy as np
import pytest

from tests import deform_kit, kit, ploc_ref, transform_ref as T
from tests.kit import ROOT, bits, render_film
from tests.test_scene_update import _compare_traces, _rays, _same_render

NEW_SYMBOLS = ["mcpt_rebuild_trees", "mcpt_get_rebuild_info"]
INVALID, UNSUPPORTED = 1, 6
W, H = 68, 52
SPHERE = 4                                                                   # material of S-cornell's glossy sphere


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_rebuild_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, ["rebuild", "rebuild_info"])
    assert (pkg.REBUILD_SAME, pkg.REBUILD_HOST, pkg.REBUILD_DEVICE) == (0, 1, 2)
    assert set(pkg.RebuildInfo().as_dict()) == {"struct_size", "rebuilds", "last_ms", "last_build_ms", "last_device_ms", "area_ratio_before"}


def test_null_context_is_an_invalid_argument_for_the_rebuild_calls(pkg):
    lib = pkg.load_library()
    o = pkg.RebuildOpts(); o.struct_size = C.sizeof(pkg.RebuildOpts)
    info = pkg.RebuildInfo()
    assert lib.mcpt_rebuild_trees(None, None) == INVALID
    assert lib.mcpt_rebuild_trees(None, C.byref(o)) == INVALID
    assert lib.mcpt_get_rebuild_info(None, C.byref(info)) == INVALID


def test_rebuild_structs_have_the_headers_layout(pkg, tmp_path):
    """sizeof and every offsetof of mcpt_rebuild_opts / mcpt_rebuild_info as a C compiler sees include/mcpt.h, against the ctypes classes."""
    for cls, name in ((pkg.RebuildOpts, "mcpt_rebuild_opts"), (pkg.RebuildInfo, "mcpt_rebuild_info")):
        c, py, consts = deform_kit.c_layout(cls, name, tmp_path, macros=("MCPT_REBUILD_SAME", "MCPT_REBUILD_HOST", "MCPT_REBUILD_DEVICE"))
        assert c == py, name
        assert consts == [pkg.REBUILD_SAME, pkg.REBUILD_HOST, pkg.REBUILD_DEVICE]


def test_rebuild_plans_are_inverse_permutations_and_refuse_anything_else(tmp_path):
    """csrc/rebuild_plan.h is pure host code: tests/rebuild_plan_check.cpp, a stand-alone program built with the host compiler and its address
    and undefined-behaviour sanitizers, plans random pairs of leaf orders at n = 1, 2, 3, 64, 65, 256, 257 and 100 003 -- src_of_dst and dst_of_src
    are inverse, the old order gathered by src_of_dst is the new one -- and is refused, with a message, a duplicate, a gap and an index out of
    range on either side."""
    exe = str(tmp_path / "rebuild_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "rebuild_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) >= 200


# (n_tris, n_nodes, wide_nodes, wide_depth, wide_tree_hash) of mcpt_check_scene on the commit before build_host_scene's tree block became
# build_trees: the host path must go on producing these bits.
PARENT_TREES = {
    "cornell": (540, 293, 62, 5, 0x0fcbe8ca8b5fa158),
    "veach": (576, 335, 73, 5, 0x86ac8f7eb72bfbb5),
    "bath16": (5636, 3010, 600, 8, 0x932e35c546799c10),
    "soup3": (3, 1, 1, 1, 0x61de8a9942a1bc7f),
    "soup9": (9, 4, 1, 1, 0x2677ea16c8556979),
    "soup257": (257, 147, 41, 4, 0x6d8f4fd6cfc6476d),
    "coincident300": (300, 171, 33, 5, 0x7eff572a69efc995),
    "shells150": (150, 87, 16, 15, 0xd630ef9daf847218),
    "strip1": (2, 1, 1, 1, 0x0071523ba403e630),
}


def _pinned_scene(pkg, name):
    S = pkg.scenes
    return {"cornell": lambda: S.cornell_box(W, H, sphere_lon=24, sphere_lat=12),
            "veach": lambda: S.veach_mis(64, 36, light_lon=12, light_lat=6, plate_cells=4),
            "bath16": lambda: S.bathroom_stress(64, 36, detail=16, tex_size=16),
            "soup3": lambda: ploc_ref.lattice_soup(pkg, 3), "soup9": lambda: ploc_ref.lattice_soup(pkg, 9), "soup257": lambda: ploc_ref.lattice_soup(pkg, 257),
            "coincident300": lambda: ploc_ref.coincident(pkg, 300), "shells150": lambda: ploc_ref.shells(pkg, 150, 1.2),
            "strip1": lambda: ploc_ref.strip(pkg, 1)}[name]()


@pytest.mark.parametrize("name", sorted(PARENT_TREES))
def test_check_scene_builds_the_trees_it_built_before_the_refactor(pkg, name):
    st, info, msg = pkg.check_scene(_pinned_scene(pkg, name))
    assert st == 0, msg
    assert (info.n_tris, info.n_nodes, info.wide_nodes, info.wide_depth, info.wide_tree_hash) == PARENT_TREES[name]


# ------------------------------------------------------------------------------------------------------------------------ GPU helpers
def _cornell(pkg):
    return pkg.scenes.cornell_box(W, H, sphere_lon=24, sphere_lat=12)


def _scrambled(pkg, scene, seed=7):
    """The sphere's vertex positions permuted among themselves: the same points, so the same bounding box and centre, under faces that now span
    the sphere -- hostile to the topology a refit keeps."""
    vi = np.unique(scene.face[scene.face[:, 0, 3] == SPHERE][:, :, 0])
    v = scene.vertex.copy()
    v[vi] = v[vi][np.random.default_rng(seed).permutation(vi.size)]
    return kit.with_arrays(pkg, scene, v)


def _tree_info(r):
    i = r.info()
    return (i.wide_tree_hash, i.n_nodes, i.wide_nodes, i.wide_depth, i.bvh_depth, i.max_leaf, i.bvh_builder)


def _probes(pkg, r, scene, binary=True):
    """Everything the probes say about a context, as bit patterns: both traversals (closest and any hit), light sampling, the light list, the
    lobe classes."""
    o, d = _rays(pkg, r, scene, n_box=1500)
    t2 = np.full(o.shape[0], 0.8)
    lp, lxi = kit.light_points(*kit.used_bounds(scene), 500, 2)
    out = {}
    for k, a in enumerate(r.probe_trace4(o, d)):
        out["trace4_%d" % k] = bits(a)
    out["trace4_any"] = r.probe_trace4(o, d, t2=t2, any_hit=True)[1]
    if binary:
        for k, a in enumerate(r.probe_trace(o, d)):
            out["trace_%d" % k] = bits(a)
        out["trace_any"] = r.probe_trace(o, d, t2=t2, any_hit=True)[1]
    out["sample_light"] = bits(r.probe_sample_light(lp, lxi))
    for k, a in enumerate(r.probe_lights()):
        out["lights_%d" % k] = bits(a)
    out["classes"] = r.probe_face_classes()
    return out


def _work(r):
    c = r.counters()
    return c.box_tests + c.tri_tests


def _with_validation(make):
    os.environ["MCPT_VALIDATE_BVH"] = "1"
    try:
        return make()
    finally:
        os.environ.pop("MCPT_VALIDATE_BVH", None)


def _read_denoised(r):
    out = np.zeros((r.height, r.width, 4), np.float32)
    r._check(r.lib.mcpt_read_denoised(r.ctx, out.ctypes.data_as(C.c_void_p)))
    return out


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "device"])
def test_a_rebuilt_context_is_the_fresh_context(pkg, builder):
    scene = _cornell(pkg); moved = _scrambled(pkg, scene)
    fl = pkg.FLAG_DETERMINISTIC | pkg.FLAG_DYNAMIC | pkg.FLAG_COUNT_TRAVERSAL | (pkg.FLAG_GPU_BVH_BUILD if builder == "device" else 0)
    R = pkg.Renderer(scene, max_depth=8, flags=fl); F = pkg.Renderer(moved, max_depth=8, flags=fl)
    assert list(R.info().centre) == list(F.info().centre)
    film0 = render_film(R, 8, 5)
    R.update_vertices(moved.vertex)
    ratio = R.update_info().wide_area_ratio
    print("[rebuild] %s: wide_area_ratio after the scramble = %.4f" % (builder, ratio))
    assert ratio > 1.2                                                     # a condition on the input: the refitted tree is a bad one
    refit = R.clone()                                                      # keeps the refitted trees
    refit_hash = R.info().wide_tree_hash
    R.rebuild()
    R.validate_trees()
    # ---- the same trees, the same streams
    assert _tree_info(R) == _tree_info(F)
    assert R.info().traversal_bytes == F.info().traversal_bytes and list(R.info().centre) == list(F.info().centre)
    assert refit.info().wide_tree_hash == refit_hash != R.info().wide_tree_hash
    deform_kit.assert_same(_probes(pkg, R, moved), _probes(pkg, F, moved))
    # ---- the film was kept and goes on
    assert np.array_equal(bits(R.read_accum()), bits(film0))
    R.render(8, seed=5, first_sample=8)
    assert np.all(R.read_accum()[..., 3] == 16)
    F.render(8, seed=5); F.render(8, seed=5, first_sample=8)
    assert np.all(F.read_accum()[..., 3] == 16)
    # ---- the same second call from an empty film, and what it costs to traverse
    films, work = {}, {}
    for name, r in (("rebuilt", R), ("fresh", F), ("refit", refit)):
        r.reset_counters(); r.clear(); r.render(8, seed=5, first_sample=8)
        films[name] = r.read_accum(); work[name] = _work(r)
    assert np.array_equal(bits(films["rebuilt"]), bits(films["fresh"]))
    _same_render(films["refit"], films["fresh"])
    print("[rebuild] %s: traversal work rebuilt / fresh = %.6f, refit / fresh = %.4f" % (builder, work["rebuilt"] / work["fresh"], work["refit"] / work["fresh"]))
    assert work["fresh"] > 0 and abs(work["rebuilt"] - work["fresh"]) <= 0.01 * work["fresh"]
    assert work["rebuilt"] < work["refit"]
    # ---- bookkeeping
    ui, ri = R.update_info(), R.rebuild_info()
    assert ui.wide_area_ratio == 1.0 and ui.updates == 1
    assert ri.rebuilds == 1 and ri.area_ratio_before == ratio
    assert ri.last_ms > 0 and 0 < ri.last_build_ms < ri.last_ms and 0 < ri.last_device_ms < ri.last_ms
    R.close(); F.close(); refit.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "device"])
def test_rebuild_right_after_creation_is_the_identity(pkg, builder):
    scene = _cornell(pkg)
    fl = pkg.FLAG_DETERMINISTIC | pkg.FLAG_DYNAMIC | (pkg.FLAG_GPU_BVH_BUILD if builder == "device" else 0)
    R = pkg.Renderer(scene, max_depth=8, flags=fl)
    film = render_film(R, 8, 5)
    before = _probes(pkg, R, scene)
    info = R.info(); tree = _tree_info(R)                                  # (after the probes: they allocate their pool)
    R.rebuild()
    R.validate_trees()
    assert _tree_info(R) == tree and R.info().device_bytes == info.device_bytes and R.info().traversal_bytes == info.traversal_bytes
    assert (R.info().bvh_build_ms, R.info().upload_ms) == (info.bvh_build_ms, info.upload_ms)
    deform_kit.assert_same(_probes(pkg, R, scene), before)
    assert np.array_equal(bits(R.read_accum()), bits(film))
    assert np.array_equal(bits(render_film(R, 8, 5)), bits(film))
    ri = R.rebuild_info()
    assert ri.rebuilds == 1 and ri.area_ratio_before == 1.0 and R.update_info().wide_area_ratio == 1.0 and R.update_info().updates == 0
    R.close()


M_A = T.about(T.rotation((1, 2, 3), 30.0) @ np.diag([0.8, 0.6, 0.9]), (0.5, 0.3, 0.5), (0.1, 0.2, -0.05))
M_B = T.about(T.rotation((0, 1, 0), -75.0) @ np.diag([0.7, 1.1, 0.7]), (0.5, 0.3, 0.5), (-0.08, 0.1, 0.1))


def _edit(mats, **by_index):
    out = list(mats)
    for k, fields in by_index.items():
        out[int(k[1:])] = dataclasses.replace(out[int(k[1:])], **fields)
    return out


@pytest.mark.gpu
def test_what_a_rebuild_keeps(pkg):
    scene = _cornell(pkg)
    S = pkg.scenes
    fl = pkg.FLAG_DETERMINISTIC | pkg.FLAG_DYNAMIC | pkg.FLAG_COUNT_TRAVERSAL
    R = pkg.Renderer(scene, max_depth=8, flags=fl)
    vg, ng = pkg.groups_from_faces(scene, (scene.face[:, 0, 3] == SPHERE).astype(int))
    light = int(np.flatnonzero([max(m.radiance) > 0 for m in scene.materials])[0])
    mats1 = _edit(scene.materials, **{"m%d" % light: dict(radiance=(9.0, 7.0, 3.0)), "m%d" % SPHERE: dict(ks=(0.3, 0.2, 0.1))})
    # the scene edits first: each of them drops the features and the tile error, which the calls after them bring back
    R.set_vertex_groups(vg, ng, 2); R.update_transforms(np.stack([T.identity(1)[0], M_A])); R.update_materials(mats1)
    R.render_features(4, seed=5)
    R.render(8, seed=3)
    R.denoise()
    R.render_adaptive(seed=3, first_sample=8, min_spp=2, max_spp=8, threshold=0.05)
    kept = dict(features=R.features(), film=R.read_accum(), denoised=_read_denoised(R), tile_error=R.tile_error(), counters=bytes(R.counters()))
    infos = (R.transform_info().as_dict(), R.material_info().as_dict(), R.update_info().updates)
    assert infos[0]["n_groups"] == 2 and kept["film"][..., 3].min() >= 8
    R.rebuild()
    R.validate_trees()
    after = dict(features=R.features(), film=R.read_accum(), denoised=_read_denoised(R), tile_error=R.tile_error(), counters=bytes(R.counters()))
    for k in kept:
        assert (kept[k] == after[k]) if isinstance(kept[k], bytes) else np.array_equal(bits(kept[k]), bits(after[k])), k
    assert (R.transform_info().as_dict(), R.material_info().as_dict(), R.update_info().updates) == infos
    # ---- the groups, the rest pose and the materials still work on the rebuilt context
    m2 = np.stack([T.identity(1)[0], M_B])
    mats2 = _edit(mats1, **{"m%d" % light: dict(radiance=(5.0, 6.0, 7.0)), "m%d" % SPHERE: dict(ks=(0.0, 0.0, 0.0))})
    R.update_transforms(m2); R.update_materials(mats2)
    R.validate_trees()
    edited = S.SceneData(scene.name, T.transform_vertices(scene.vertex, vg, m2), T.transform_normals(scene.normal, ng, m2), scene.texcoord, scene.face,
                         mats2, scene.camera, dict(scene.meta))
    F = pkg.Renderer(edited, max_depth=8, flags=pkg.FLAG_DETERMINISTIC)
    assert list(R.info().centre) == list(F.info().centre)
    _compare_traces(pkg, R, F, edited, "probe_trace4", exact=True)
    _compare_traces(pkg, R, F, edited, "probe_trace", exact=True)
    for a, b in zip(R.probe_lights(), F.probe_lights()):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(R.probe_face_classes(), F.probe_face_classes())
    R.close(); F.close()


@pytest.mark.gpu
def test_motion_reprojection_after_a_rebuild(pkg):
    """mcpt_update_vertices_reproject works on the rebuilt streams as on the created ones: a context rebuilt right after creation (the same trees
    in new buffers) and one never rebuilt carry the same film over the same update, bit for bit, and count the same reused pixels."""
    scene = _cornell(pkg); moved = kit.moved_sphere(pkg, scene)
    out = []
    for rebuild in (False, True):
        r = pkg.Renderer(scene, max_depth=8, flags=pkg.FLAG_DETERMINISTIC | pkg.FLAG_DYNAMIC)
        r.render(16, seed=3); r.render_features(4, seed=5)
        if rebuild:
            r.rebuild()
        r.update_vertices_reproject(moved.vertex, moved.normal, feature_spp=4, feature_seed=5, max_history=64.0)
        out.append((r.read_accum(), int(r.reproject_info().pixels_reused)))
        r.close()
    assert out[0][1] == out[1][1] and out[0][1] > 0.3 * W * H
    assert np.array_equal(bits(out[0][0]), bits(out[1][0]))


@pytest.mark.gpu
def test_update_after_a_rebuild(pkg):
    """The refit runs on the rebuilt trees (new level tables, new box scratch): back to the original vertices on trees built for the scramble."""
    scene = _cornell(pkg); moved = _scrambled(pkg, scene)
    R = pkg.Renderer(scene, max_depth=8, flags=pkg.FLAG_DETERMINISTIC | pkg.FLAG_DYNAMIC); F = pkg.Renderer(scene, max_depth=8, flags=pkg.FLAG_DETERMINISTIC)
    R.update_vertices(moved.vertex); R.rebuild()
    R.update_vertices(scene.vertex)
    R.validate_trees()
    _compare_traces(pkg, R, F, scene, "probe_trace4", exact=True)
    _compare_traces(pkg, R, F, scene, "probe_trace", exact=True)
    _same_render(render_film(R, 16, 21), render_film(F, 16, 21))
    assert R.update_info().updates == 2 and R.rebuild_info().rebuilds == 1
    R.close(); F.close()


@pytest.mark.gpu
@pytest.mark.parametrize("maker,args", [("lattice_soup", (3,)), ("lattice_soup", (9,)), ("lattice_soup", (257,)), ("coincident", (300,)), ("shells", (150, 1.2)),
                                        ("strip", (1,))])
def test_rebuild_of_small_tied_and_deep_device_built_trees(pkg, maker, args):
    """The sizes of tests/test_scene_update.py::test_refit_of_small_tied_and_deep_device_built_trees, device builder: one wide record (3 and 9
    triangles), the edge of a 256-thread block for a lane per triangle and for a lane per 16 bytes (257), exact ties whose ranks follow the new
    order (300 copies), a chain about 148 deep, and two triangles, where mcpt_create and the rebuild never call the device builder.  Every vertex
    scaled by 1.25 about the centre, updated, rebuilt: equal to a fresh context by _compare_traces' criteria for contexts that round on their own."""
    scene = getattr(ploc_ref, maker)(pkg, *args)
    fl = pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD
    R = _with_validation(lambda: pkg.Renderer(scene, flags=fl))
    built = 0 if maker == "strip" else 1
    assert R.info().bvh_builder == built
    lo, hi = kit.used_bounds(scene); c = 0.5 * lo + 0.5 * hi
    moved = kit.with_arrays(pkg, scene, vertex=(scene.vertex - c) * 1.25 + c)
    R.update_vertices(moved.vertex)
    _with_validation(lambda: R.rebuild())
    R.validate_trees()
    F = _with_validation(lambda: pkg.Renderer(moved, flags=fl))
    assert R.info().bvh_builder == F.info().bvh_builder == built
    _compare_traces(pkg, R, F, moved, "probe_trace4", exact=False, rays=ploc_ref.interior_rays(moved, 1500, seed=10)[:2])
    assert R.update_info().wide_area_ratio == 1.0 and R.rebuild_info().rebuilds == 1
    R.close(); F.close()


@pytest.mark.gpu
def test_reference_tie_ranks_are_carried_through_a_rebuild(pkg):
    """300 copies of one triangle under MCPT_FLAG_REFERENCE_TIE_ORDER: which copy a ray names is decided by the ranks alone.  The host builder
    gives the device-built context another leaf order; the ranks travel with their triangles, so every ray names the face it named."""
    scene = ploc_ref.coincident(pkg, 300)
    R = pkg.Renderer(scene, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD | pkg.FLAG_REFERENCE_TIE_ORDER)
    o, d = ploc_ref.interior_rays(scene, 1500, seed=9)[:2]
    before = R.probe_trace4(o, d)
    h0 = R.info().wide_tree_hash
    R.rebuild(pkg.REBUILD_HOST)
    R.validate_trees()
    assert R.info().wide_tree_hash != h0 and R.info().bvh_builder == 0
    after = R.probe_trace4(o, d)
    assert (before[1] >= 0).mean() > 0.3
    for a, b in zip(before, after):
        assert np.array_equal(bits(a), bits(b))
    R.close()


@pytest.mark.gpu
def test_the_overflow_area_follows_a_deeper_wide_tree(pkg):
    """A chain of 150 nested shells: the host builder's tree is shallow, the device builder's about 148 deep.  Rebuilding the shallow context with
    the device builder must give the trace kernel the larger stack-overflow area before the first render walks the deep tree; the other way round
    the context ends as the host-built one."""
    scene = ploc_ref.shells(pkg, 150, 1.2)
    fl = pkg.FLAG_DYNAMIC | pkg.FLAG_DETERMINISTIC
    host = pkg.Renderer(scene, flags=fl); dev = pkg.Renderer(scene, flags=fl | pkg.FLAG_GPU_BVH_BUILD)
    hi, di = host.info(), dev.info()
    print("[deeper] wide_depth host %d, device %d" % (hi.wide_depth, di.wide_depth))
    assert (hi.bvh_builder, di.bvh_builder) == (0, 1) and di.wide_depth > hi.wide_depth
    film_host, film_dev = render_film(host, 4, 3), render_film(dev, 4, 3)
    host.rebuild(pkg.REBUILD_DEVICE)
    host.validate_trees()
    assert _tree_info(host) == _tree_info(dev) and host.info().wide_depth > hi.wide_depth
    a = render_film(host, 4, 3)
    assert np.isfinite(a).all()
    _same_render(a, film_dev)
    dev.rebuild(pkg.REBUILD_HOST)
    dev.validate_trees()
    assert _tree_info(dev) == (hi.wide_tree_hash, hi.n_nodes, hi.wide_nodes, hi.wide_depth, hi.bvh_depth, hi.max_leaf, 0)
    b = render_film(dev, 4, 3)
    assert np.isfinite(b).all()
    _same_render(b, film_host)
    host.close(); dev.close()


@pytest.mark.gpu
def test_rebuild_refusals_change_nothing(pkg):
    scene = _cornell(pkg)
    fl = pkg.FLAG_DETERMINISTIC
    plain = pkg.Renderer(scene, max_depth=6, flags=fl); dyn = pkg.Renderer(scene, max_depth=6, flags=fl | pkg.FLAG_DYNAMIC)

    def state(r):
        return (bytes(r.info()), bits(r.read_accum()).tobytes(), r.rebuild_info().as_dict(), r.update_info().updates)

    for r in (plain, dyn):
        r.render(4, seed=5)
    s_plain, s_dyn = state(plain), state(dyn)
    with pytest.raises(pkg.McptError) as e:
        plain.rebuild()
    assert "status %d" % UNSUPPORTED in str(e.value)
    with pytest.raises(pkg.McptError) as e:
        dyn.rebuild(3)
    assert "status %d" % INVALID in str(e.value)
    o = pkg.RebuildOpts(); o.struct_size = C.sizeof(pkg.RebuildOpts) - 4
    assert dyn.lib.mcpt_rebuild_trees(dyn.ctx, C.byref(o)) == INVALID
    o.struct_size = 0
    assert dyn.lib.mcpt_rebuild_trees(dyn.ctx, C.byref(o)) == INVALID
    assert dyn.lib.mcpt_get_rebuild_info(dyn.ctx, None) == INVALID
    assert state(plain) == s_plain and state(dyn) == s_dyn
    dyn.validate_trees()
    assert np.array_equal(bits(render_film(dyn, 4, 5)), bits(render_film(plain, 4, 5)))
    assert dyn.lib.mcpt_rebuild_trees(dyn.ctx, None) == 0                  # NULL options: the defaults
    assert dyn.rebuild_info().rebuilds == 1
    plain.close(); dyn.close()


@pytest.mark.gpu
def test_clones_before_and_after_a_rebuild(pkg):
    scene = _cornell(pkg); moved = _scrambled(pkg, scene); moved2 = _scrambled(pkg, scene, seed=8)
    fl = pkg.FLAG_DETERMINISTIC | pkg.FLAG_DYNAMIC
    R = pkg.Renderer(scene, max_depth=8, flags=fl)
    R.update_vertices(moved.vertex)
    early = R.clone()
    h_refit = R.info().wide_tree_hash
    R.rebuild()
    late = R.clone()
    assert early.info().wide_tree_hash == h_refit != R.info().wide_tree_hash == late.info().wide_tree_hash
    assert late.rebuild_info().rebuilds == 0 and late.update_info().wide_area_ratio == 1.0
    film = render_film(R, 8, 5)
    assert np.array_equal(bits(render_film(late, 8, 5)), bits(film))
    _same_render(render_film(early, 8, 5), film)
    # a clone of a rebuilt context can itself update and rebuild, and the source does not follow it
    late.update_vertices(moved2.vertex); late.validate_trees()
    late.rebuild(); late.validate_trees()
    F2 = pkg.Renderer(moved2, max_depth=8, flags=pkg.FLAG_DETERMINISTIC)
    assert _tree_info(late) == _tree_info(F2)
    assert np.array_equal(bits(render_film(late, 8, 5)), bits(render_film(F2, 8, 5)))
    assert np.array_equal(bits(render_film(R, 8, 5)), bits(film))
    early.validate_trees()
    for r in (R, early, late, F2):
        r.close()


@pytest.mark.gpu
def test_facade_rebuild(pkg, tmp_path):
    exe = kit.build_facade("facade_rebuild.cpp", tmp_path)
    a = pkg.scenes.cornell_box(44, 30, sphere_lon=24, sphere_lat=12)
    b = _scrambled(pkg, a)
    obj_a = a.write(str(tmp_path / "a")); obj_b = b.write(str(tmp_path / "b"))
    outs = [str(tmp_path / n) for n in ("rebuilt.bin", "fresh.bin")]
    j, k = 2, 6
    line = kit.run_facade(exe, [obj_a, obj_b, str(j), str(k)] + outs)
    w, h = int(line[0]), int(line[1])
    assert (w, h, int(line[2])) == (44, 30, k)
    assert float(line[3]) > 1.2 and int(line[4]) == 1
    assert int(line[5]) == int(line[6])                                    # the rebuilt context has the fresh context's trees
    rebuilt, fresh = [np.fromfile(p, np.float32).reshape(h, w, 4) for p in outs]
    assert np.all(rebuilt[..., 3] == k)                                    # the picture went on across the rebuild: j + (k - j) samples
    _same_render(rebuilt, fresh)                                           # j of them through the refitted trees: up to exact ties


@pytest.mark.gpu
def test_cli_rebuild_above(pkg, tmp_path):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    out = str(tmp_path / "img")
    base = [obj, "--turntable", "3", "--spp", "4", "--depth", "5", "--out", out]
    def rebuild_lines(stdout):
        lines = [l.split() for l in stdout.splitlines() if l.startswith("rebuild: frame ")]
        for words in lines:                                                # rebuild: frame F    wide_area_ratio before: X    cost: Y ms
            assert 0 <= int(words[2]) < 3 and float(words[5]) > 0.0 and float(words[7]) > 0.0 and words[8] == "ms"
        return lines

    p = kit.run_cli(base + ["--spin", "glossy", "--rebuild-above", "1.0"])
    assert p.returncode == 0, p.stderr[-2000:]
    imgs = kit.turntable_frames(out)
    assert imgs[0] != imgs[1] and imgs[1] != imgs[2]
    lines = rebuild_lines(p.stdout)
    print("[cli] --rebuild-above 1.0: %d rebuilds" % len(lines))
    assert len(lines) <= 3 and all(float(w[5]) > 1.0 for w in lines)
    p = kit.run_cli(base + ["--spin", "glossy", "--rebuild-above", "0"])       # every ratio exceeds 0: one rebuild per frame
    assert p.returncode == 0, p.stderr[-2000:]
    assert [int(w[2]) for w in rebuild_lines(p.stdout)] == [0, 1, 2]
    kit.turntable_frames(out)
    q = kit.run_cli(base + ["--spin", "glossy", "--rebuild-above", "1e9"])   # never reached: no rebuild, the same frames
    assert q.returncode == 0 and not [l for l in q.stdout.splitlines() if l.startswith("rebuild: ")]
    q = kit.run_cli(base + ["--rebuild-above", "1.1"])
    assert q.returncode == 2 and "--rebuild-above" in q.stderr
    q = kit.run_cli([obj, "--wobble", "0.01", "--rebuild-above", "1.1"])
    assert q.returncode == 2


@pytest.mark.gpu
def test_rebuild_is_cheaper_than_the_create_it_replaces(pkg):
    """S-bath detail 64 (0.12 M triangles) with the fixture displacement of test_refit_is_faster_than_the_rebuild_it_replaces:
    mcpt_rebuild_info::last_ms, median of 5, against the wall time of constructing a fresh Renderer of the moved scene with the same flags in the
    same process, median of 5.  The call does a subset of mcpt_create's work plus small read-backs: strictly less is the condition for it to be
    worth calling.  The measured figures are in DESIGN.md §17."""
    scene = pkg.scenes.bathroom_stress(64, 36, detail=64, tex_size=16)
    fixtures = np.isin(scene.face[:, 0, 3], (5, 6))
    vi = np.unique(scene.face[fixtures][:, :, 0])
    v = scene.vertex.copy()
    p = v[vi]
    v[vi] = p + 0.02 * np.stack([np.sin(9.0 * p[:, 1]), np.sin(7.0 * p[:, 2]), np.sin(8.0 * p[:, 0])], -1)
    moved = kit.with_arrays(pkg, scene, v)
    fl = pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD
    R = pkg.Renderer(scene, max_depth=6, flags=fl)
    n_tris = R.info().n_tris
    rebuild_ms, create_ms = [], []
    for i in range(5):
        R.update_vertices(moved.vertex if i % 2 == 0 else scene.vertex)
        R.rebuild()
        rebuild_ms.append(R.rebuild_info().last_ms)
    R.validate_trees()
    for i in range(5):
        t0 = time.perf_counter()
        F = pkg.Renderer(moved, max_depth=6, flags=fl)
        create_ms.append(1e3 * (time.perf_counter() - t0))
        if i < 4:
            F.close()
    R.close(); F.close()
    rb, cr = float(np.median(rebuild_ms)), float(np.median(create_ms))
    print("\n[rebuild cost] %d triangles: rebuild %.2f ms (median of 5; min %.2f max %.2f) | fresh Renderer %.2f ms (median of 5; min %.2f max %.2f) | ratio %.3f" % (
        n_tris, rb, min(rebuild_ms), max(rebuild_ms), cr, min(create_ms), max(create_ms), rb / cr))
    assert 0 < rb < cr
