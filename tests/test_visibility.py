"""Faces of a live scene shown and hidden on the device: mcpt_set_face_visibility and its _reproject form (csrc/visibility.hip: the
hide pass after rf_triangles_kernel; csrc/materials.hip: the light list rebuilt with "visible" as a second membership test),
mcpt_get_visibility_info, mcpt_probe_triangles and their public surfaces.

Two oracles.  The records and boxes are held to tests/visibility_ref.py, the numpy restatement of the rules, bit for bit.  Everything a ray can
see is held to this library's own fresh context of the SUB-SCENE: the same SceneData with the hidden rows of `face` deleted (vertex arrays kept;
the hidden parts lie inside the room, so the bounding box and with it the centre are the same).  The two contexts have different trees, so
among triangles hit at exactly the same distance they may name different ones: `_assert_same_rays` states what is compared how.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests import deform_kit as K, kit, visibility_ref as V
from tests.deform_kit import _any_hits, _assert_same_rays, _full_state
from tests.kit import bits, render_film

NEW_SYMBOLS = ["mcpt_set_face_visibility", "mcpt_set_face_visibility_reproject", "mcpt_get_visibility_info", "mcpt_probe_triangles"]
METHODS = ["set_face_visibility", "set_face_visibility_reproject", "visibility_info", "probe_triangles"]
INVALID, NO_LIGHTS, UNSUPPORTED = 1, 4, 6
SEED_F = 5


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_visibility_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, METHODS)
    assert callable(pkg.visibility_from_materials)


def test_null_context_is_an_invalid_argument_for_the_visibility_calls(pkg):
    lib = pkg.load_library()
    buf = np.zeros(64, np.float32); p = buf.ctypes.data_as(C.c_void_p); info = pkg.VisibilityInfo()
    assert lib.mcpt_set_face_visibility(None, p, 4) == INVALID
    assert lib.mcpt_set_face_visibility_reproject(None, p, 4, None, None) == INVALID
    assert lib.mcpt_get_visibility_info(None, C.byref(info)) == INVALID
    assert lib.mcpt_probe_triangles(None, p, p) == INVALID


def test_visibility_info_has_the_headers_layout(pkg, tmp_path):
    """sizeof and every offsetof of mcpt_visibility_info as a C compiler sees include/mcpt.h, against the ctypes class."""
    c, py, _ = K.c_layout(pkg.VisibilityInfo, "mcpt_visibility_info", tmp_path)
    assert c == py and c[0] == 56
    assert [f[0] for f in pkg.VisibilityInfo._fields_] == ["struct_size", "set", "n_hidden", "n_hidden_emitters", "updates", "reserved0", "last_ms", "device_bytes",
                                                           "reserved"]


def test_visibility_from_materials(pkg):
    s = K.scene(pkg, small=True)
    mtl = s.face[:, 0, 3]
    m = pkg.visibility_from_materials(s, [K.SPHERE])
    assert m.dtype == np.uint8 and m.shape == (s.face.shape[0],) and np.array_equal(m == 0, mtl == K.SPHERE) and set(np.unique(m)) == {0, 1}
    assert np.array_equal(pkg.visibility_from_materials(s, [K.SPHERE, K.LAMP, K.LAMP]) == 0, (mtl == K.SPHERE) | (mtl == K.LAMP))
    assert pkg.visibility_from_materials(s, []).all()
    for bad in ([-1], [len(s.materials)]):
        with pytest.raises(ValueError):
            pkg.visibility_from_materials(s, bad)


def _plan_cases(pkg):
    """(mask or None, face_material, material_emits): S-cornell-small under masks of every kind, and shapes at the edges."""
    s = K.scene(pkg, small=True); fm = s.face[:, 0, 3].astype(np.uint32); em = V.emits(s.materials).astype(np.uint8)
    rng = np.random.default_rng(7); nf = fm.shape[0]
    cases = [(None, fm, em), (np.ones(nf, np.uint8), fm, em), (np.zeros(nf, np.uint8), fm, em), (pkg.visibility_from_materials(s, [K.SPHERE]), fm, em),
             (pkg.visibility_from_materials(s, [K.LAMP]), fm, em), ((rng.uniform(size=nf) < 0.5).astype(np.uint8) * 200, fm, em),
             ((rng.uniform(size=nf) < 0.5).astype(np.uint8), fm, np.ones_like(em)), ((rng.uniform(size=nf) < 0.9).astype(np.uint8), fm, np.zeros_like(em)),
             (np.zeros(0, np.uint8), np.zeros(0, np.uint32), em), (None, np.zeros(0, np.uint32), np.zeros(0, np.uint8)),
             (np.array([1, 0, 1, 0], np.uint8), np.array([0, 1, 7, 9], np.uint32), np.array([1, 1], np.uint8)),    # materials out of range: never emitters
             (np.array([0], np.uint8), np.array([0], np.uint32), np.array([1], np.uint8))]
    assert em.sum() == 1 and em[K.LAMP]
    return cases


@K.needs_hipcc
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_plan_is_the_restatement(pkg, tmp_path, sanitized):
    """vs_plan of csrc/visibility_plan.h -- what both validation paths count visible emitters with -- built into the stand-alone program
    tests/visibility_plan_check.cpp (its own main; no device is touched, nothing is loaded into Python) against visibility_ref.plan.
    `sanitized`: the same program under the host's address and undefined-behaviour sanitizers, which must stay silent."""
    exe = K.build_host_check("visibility_plan_check", [], tmp_path, sanitized)
    cases = _plan_cases(pkg)
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(np.array([len(cases)], np.uint32).tobytes())
        for mask, fm, em in cases:
            f.write(np.array([fm.size, em.size, 0 if mask is None else 1], np.uint32).tobytes())
            f.write(b"" if mask is None else mask.tobytes()); f.write(fm.tobytes()); f.write(em.tobytes())
    K.run_host_check(exe, tmp_path, sanitized)
    raw = np.fromfile(str(tmp_path / "out.bin"), np.uint32)
    at = 0
    for i, (mask, fm, em) in enumerate(cases):
        want = V.plan(mask, fm, em)
        got = raw[at:at + 3 + em.size]; at += 3 + em.size
        assert got[:3].tolist() == [want["n_hidden"], want["n_hidden_emitters"], want["n_lights"]], i
        assert np.array_equal(got[3:], want["visible_faces"]), i
    assert at == raw.size
    assert V.plan(cases[3][0], cases[3][1], cases[3][2])["n_lights"] == 2 and V.plan(cases[4][0], cases[4][1], cases[4][2])["n_lights"] == 0


# ------------------------------------------------------------------------------------------------------------------------ GPU helpers
def _ctx(pkg, scene, dynamic=True):
    return pkg.Renderer(scene, max_depth=6, flags=K.FLAGS(pkg) if dynamic else pkg.FLAG_DETERMINISTIC)


def _hidden_sphere(pkg, small=False):
    s = K.scene(pkg, small)
    return s, pkg.visibility_from_materials(s, [K.SPHERE])


def _assert_records(pkg, r, scene, mask, vertex=None):
    """probe_triangles() against the restatement, bit for bit."""
    rec, box = r.probe_triangles()
    want_rec, want_box = V.hide(*V.visible_records(scene.vertex if vertex is None else vertex, scene.face, tuple(r.info().centre)), mask)
    bad = np.flatnonzero((bits(rec) != bits(want_rec)).any(axis=1) | (bits(box) != bits(want_box)).any(axis=1))
    assert bad.size == 0, "face %d of %d differing: device %r %r, restatement %r %r" % (bad[0], bad.size, rec[bad[0]].tolist(), box[bad[0]].tolist(),
                                                                                      want_rec[bad[0]].tolist(), want_box[bad[0]].tolist())
    return rec, box


def _infos(r):
    i = r.info()
    out = {"scene": [getattr(i, k) if k != "centre" else tuple(i.centre) for k, _ in i._fields_ if k != "upload_ms"]}
    out.update(update=r.update_info().as_dict(), visibility=r.visibility_info().as_dict(), material=r.material_info().as_dict(),
               reproject=r.reproject_info().as_dict())
    return out


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_records_of_hidden_and_visible_faces(pkg, small):
    scene, mask = _hidden_sphere(pkg, small)
    hidden = mask == 0
    r = _ctx(pkg, scene)
    with pytest.raises(pkg.McptError) as e:
        r.probe_triangles()                                                  # the boxes are scratch of the scene update: none has run
    assert "status 1" in str(e.value)
    r.update_vertices(scene.vertex)
    rec0, box0 = _assert_records(pkg, r, scene, None)
    ratio0 = r.update_info().wide_area_ratio
    bytes0 = r.info().device_bytes; nt = scene.face.shape[0]
    assert r.visibility_info().as_dict() == dict(struct_size=56, set=0, n_hidden=0, n_hidden_emitters=0, updates=0, last_ms=0.0, device_bytes=0)
    r.set_face_visibility(mask)
    rec, box = _assert_records(pkg, r, scene, mask)
    assert np.array_equal(bits(rec[~hidden]), bits(rec0[~hidden])) and np.array_equal(bits(box[~hidden]), bits(box0[~hidden]))
    assert np.array_equal(bits(rec[hidden, :3]), bits(rec0[hidden, :3]))      # v0 kept
    assert np.all(bits(rec[hidden, 3:]) == 0)                                  # both edges +0
    assert np.array_equal(bits(box[hidden, :3]), bits(rec[hidden, :3])) and np.array_equal(bits(box[hidden, 3:]), bits(rec[hidden, :3]))
    r.validate_trees()
    ui, vi = r.update_info(), r.visibility_info()
    assert ui.updates == 2 and ui.wide_area_ratio < ratio0
    assert (vi.set, vi.n_hidden, vi.n_hidden_emitters, vi.updates, vi.device_bytes) == (1, int(hidden.sum()), 0, 1, nt) and vi.last_ms > 0
    assert r.info().device_bytes - bytes0 == nt + 4 * nt + 4 * ((nt + 255) // 256)   # the mask; the light rebuild's scan scratch (§15's, allocated once)
    assert r.info().n_lights == 2 == r.material_info().n_lights
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_nothing_hits_a_hidden_face_and_the_rest_is_the_sub_scene(pkg, small):
    scene, mask = _hidden_sphere(pkg, small)
    sub, new_of_old = V.sub_scene(pkg, scene, mask)
    r, s = _ctx(pkg, scene), _ctx(pkg, sub)
    assert tuple(r.info().centre) == tuple(s.info().centre)
    r.set_face_visibility(mask)
    a, b = _full_state(pkg, r), _full_state(pkg, s)
    _assert_same_rays(a, b, new_of_old, mask == 0)
    # the first-hit and the feature kernel walk the binary tree with the same triangle test: no pixel sees the sphere either
    face, _ = r.probe_first_hits()
    assert not (mask == 0)[face[face >= 0]].any()
    sface, _ = s.probe_first_hits()
    assert np.array_equal(face >= 0, sface >= 0)
    r.render_features(4, seed=SEED_F); s.render_features(4, seed=SEED_F)
    fr, fs = r.features(), s.features()
    assert float(np.mean(np.any(bits(fr) != bits(fs), axis=-1))) <= 0.01
    r.close(); s.close()


@pytest.mark.gpu
def test_hide_then_show_is_a_refit_without_a_move(pkg):
    scene, mask = _hidden_sphere(pkg)
    r, o = K.pair(pkg)
    nt = scene.face.shape[0]
    b0 = r.info().device_bytes
    assert b0 == o.info().device_bytes
    r.set_face_visibility(mask)
    assert r.info().device_bytes == b0 + nt + 4 * nt + 4 * ((nt + 255) // 256)
    r.set_face_visibility(None)
    o.update_vertices(scene.vertex)
    vi = r.visibility_info()
    assert (vi.set, vi.n_hidden, vi.n_hidden_emitters, vi.updates, vi.device_bytes) == (0, 0, 0, 2, 0)
    # the mask is freed; the scan scratch of the light rebuild stays, as after mcpt_update_materials (include/mcpt.h)
    assert r.info().device_bytes == b0 + 4 * nt + 4 * ((nt + 255) // 256) == o.info().device_bytes + 4 * nt + 4 * ((nt + 255) // 256)
    K.assert_same(_full_state(pkg, r), _full_state(pkg, o))                   # the same topology and the same boxes: film included
    assert np.array_equal(bits(r.probe_triangles()[0]), bits(o.probe_triangles()[0])) and np.array_equal(bits(r.probe_triangles()[1]), bits(o.probe_triangles()[1]))
    assert r.update_info().updates == 2 and o.update_info().updates == 1
    assert r.update_info().wide_area_ratio == o.update_info().wide_area_ratio
    r.close(); o.close()


@pytest.mark.gpu
def test_hiding_an_emitter_takes_it_off_the_light_list(pkg):
    scene = K.scene(pkg)
    lamp = np.flatnonzero(scene.face[:, 0, 3] == K.LAMP)
    assert lamp.size == 2
    mask = np.ones(scene.face.shape[0], np.uint8); mask[lamp[0]] = 0
    sub, new_of_old = V.sub_scene(pkg, scene, mask)
    r, s = _ctx(pkg, scene), _ctx(pkg, sub)
    assert r.info().n_lights == 2
    r.set_face_visibility(mask)
    assert r.info().n_lights == r.material_info().n_lights == s.info().n_lights == 1
    vi = r.visibility_info()
    assert (vi.set, vi.n_hidden, vi.n_hidden_emitters) == (1, 1, 1)
    lr, ls = r.probe_lights(), s.probe_lights()
    assert np.array_equal(new_of_old[lr[0]], ls[0]) and lr[0].tolist() == [lamp[1]]
    assert np.array_equal(bits(lr[1]), bits(ls[1])) and np.array_equal(bits(lr[2]), bits(ls[2]))
    lp, lxi = kit.light_points(0.0, 1.0, 4096, 11)
    sr, ss = r.probe_sample_light(lp, lxi), s.probe_sample_light(lp, lxi)
    assert np.array_equal(new_of_old[sr[:, 8].astype(np.int64)], ss[:, 8].astype(np.int64))
    keep = [0, 1, 2, 3, 4, 5, 6, 7, 9]
    assert np.array_equal(bits(sr[:, keep]), bits(ss[:, keep]))
    _assert_same_rays(_full_state(pkg, r), _full_state(pkg, s), new_of_old, mask == 0)
    # every lamp face hidden: no light would be left -- refused, by either form, and nothing changes
    before, infos = _full_state(pkg, r), _infos(r)
    rec = r.probe_triangles()
    dark = mask.copy(); dark[lamp] = 0
    for call in (lambda: r.set_face_visibility(dark), lambda: r.set_face_visibility_reproject(dark), lambda: r.set_face_visibility(np.zeros_like(mask))):
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % NO_LIGHTS in str(e.value)
    assert _infos(r) == infos
    K.assert_same(before, _full_state(pkg, r))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(rec, r.probe_triangles()))
    r.close(); s.close()


@pytest.mark.gpu
def test_material_edits_under_a_mask(pkg):
    scene, mask = _hidden_sphere(pkg)
    n_sphere = int((mask == 0).sum())
    glow = list(scene.materials); glow[K.SPHERE] = dataclasses.replace(glow[K.SPHERE], radiance=(0.8, 0.5, 0.3))
    only_sphere = list(glow); only_sphere[K.LAMP] = dataclasses.replace(only_sphere[K.LAMP], radiance=(0.0, 0.0, 0.0))
    glowing = pkg.scenes.SceneData(scene.name, scene.vertex, scene.normal, scene.texcoord, scene.face, glow, scene.camera, dict(scene.meta))
    r = _ctx(pkg, scene)
    r.set_face_visibility(mask)
    r.update_materials(glow)                                                 # the hidden sphere emits: it stays out of the list
    assert r.info().n_lights == r.material_info().n_lights == 2 and r.probe_lights()[0].size == 2
    assert r.visibility_info().n_hidden_emitters == n_sphere
    sub, new_of_old = V.sub_scene(pkg, glowing, mask)
    s = _ctx(pkg, sub)
    _assert_same_rays(_full_state(pkg, r), _full_state(pkg, s), new_of_old, mask == 0)
    s.close()
    before, infos = _full_state(pkg, r), _infos(r)
    with pytest.raises(pkg.McptError) as e:
        r.update_materials(only_sphere)                                      # the only emitter left would be the hidden one
    assert "status %d" % NO_LIGHTS in str(e.value)
    assert _infos(r) == infos
    K.assert_same(before, _full_state(pkg, r))
    r.set_face_visibility(None)                                              # shown: the sphere's faces join the list, in face order
    assert r.info().n_lights == r.material_info().n_lights == n_sphere + 2
    f = _ctx(pkg, glowing)
    f.update_vertices(scene.vertex)                                          # (the refit r's trees have been through)
    assert f.info().n_lights == n_sphere + 2
    lp, lxi = kit.light_points(0.0, 1.0, 4096, 11)
    faces = r.probe_lights()[0]
    assert faces.size == n_sphere + 2 and np.all(np.diff(faces) > 0)
    assert np.array_equal(r.probe_face_classes(), f.probe_face_classes())
    assert np.array_equal(bits(r.probe_sample_light(lp, lxi)), bits(f.probe_sample_light(lp, lxi)))
    K.assert_same(_full_state(pkg, r), _full_state(pkg, f))
    r.close(); f.close()


@pytest.mark.gpu
def test_the_mask_is_sticky_through_every_route(pkg):
    scene, mask = _hidden_sphere(pkg)
    sub, new_of_old = V.sub_scene(pkg, scene, mask)
    r, s = _ctx(pkg, scene), _ctx(pkg, sub)
    lamp_faces = lambda sc: (sc.face[:, 0, 3] == K.LAMP).astype(int)
    r.set_vertex_groups(*pkg.groups_from_faces(scene, lamp_faces(scene)), 2); s.set_vertex_groups(*pkg.groups_from_faces(sub, lamp_faces(sub)), 2)
    r.set_face_visibility(mask)
    moved = kit.moved_sphere(pkg, scene)
    m = np.stack([K.T.identity(1)[0], K.M_LAMP])

    def both(call):
        call(r); call(s)
        _assert_same_rays(_full_state(pkg, r), _full_state(pkg, s), new_of_old, mask == 0)

    both(lambda c: c.update_vertices(moved.vertex, moved.normal))
    _assert_records(pkg, r, scene, mask, moved.vertex)
    both(lambda c: c.update_transforms(m))                                    # the groups' rest pose is the creation scene: the sphere is back, the lamp moves
    assert np.abs(r.vertices()[0] - scene.vertex).max() > 0.1                 # (the lamp has moved; what the matrices write is tests/test_transforms.py's business)
    _assert_records(pkg, r, scene, mask, r.vertices()[0])
    r.set_auto_normals(); s.set_auto_normals()
    both(lambda c: c.update_normals())
    _assert_records(pkg, r, scene, mask, r.vertices()[0])
    vi = r.visibility_info()
    assert (vi.set, vi.n_hidden, vi.updates) == (1, int((mask == 0).sum()), 1) and vi.last_ms > 0
    assert r.update_info().updates == 4 and r.info().n_lights == 2
    r.close(); s.close()


@pytest.mark.gpu
def test_refusals_change_nothing(pkg):
    scene, mask = _hidden_sphere(pkg, small=True)
    lib = pkg.load_library()
    fixed = _ctx(pkg, scene, dynamic=False)
    before, infos = _full_state(pkg, fixed), _infos(fixed)
    for call in (lambda: fixed.set_face_visibility(mask), lambda: fixed.set_face_visibility(None), lambda: fixed.set_face_visibility_reproject(mask),
                 lambda: fixed.probe_triangles(), lambda: fixed.set_face_visibility(mask[:-1])):   # (UNSUPPORTED comes before the count is looked at)
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % UNSUPPORTED in str(e.value)
    assert _infos(fixed) == infos
    K.assert_same(before, _full_state(pkg, fixed))
    fixed.close()
    r = _ctx(pkg, scene)
    r.set_face_visibility(mask)
    before, infos = _full_state(pkg, r), _infos(r)
    rec = r.probe_triangles()
    nf = mask.shape[0]
    longer = np.ones(nf + 1, np.uint8)
    assert lib.mcpt_set_face_visibility(r.ctx, longer.ctypes.data_as(C.c_void_p), nf + 1) == INVALID
    assert lib.mcpt_set_face_visibility(r.ctx, longer.ctypes.data_as(C.c_void_p), nf - 1) == INVALID
    assert lib.mcpt_set_face_visibility(r.ctx, None, 0) == INVALID           # the count is checked with a NULL mask too
    assert lib.mcpt_set_face_visibility_reproject(r.ctx, longer.ctypes.data_as(C.c_void_p), nf + 1, None, None) == INVALID
    bad_opts = pkg.ReprojectOpts(); bad_opts.struct_size = 4
    assert lib.mcpt_set_face_visibility_reproject(r.ctx, None, nf, None, C.byref(bad_opts)) == INVALID   # the options come after the mask: still nothing changed
    assert lib.mcpt_get_visibility_info(r.ctx, None) == INVALID
    assert _infos(r) == infos
    K.assert_same(before, _full_state(pkg, r))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(rec, r.probe_triangles()))
    r.close()


@pytest.mark.gpu
def test_clone_and_rebuild_keep_the_mask(pkg):
    scene, mask = _hidden_sphere(pkg)
    hidden = mask == 0
    identity = np.arange(scene.face.shape[0], dtype=np.int32)
    r = _ctx(pkg, scene)
    r.set_face_visibility(mask)
    before = _full_state(pkg, r)
    c = r.clone(0)
    assert c.visibility_info().as_dict() == r.visibility_info().as_dict()
    assert c.info().n_lights == 2
    K.assert_same(before, _full_state(pkg, c))
    assert np.array_equal(bits(c.probe_triangles(boxes=False)), bits(r.probe_triangles(boxes=False)))
    c.update_vertices(scene.vertex)                                          # the clone's own updates hide the same faces
    K.assert_same(before, _full_state(pkg, c))
    c.close()
    r.rebuild(pkg.REBUILD_DEVICE)                                            # other trees over the same records
    r.validate_trees()
    assert r.visibility_info().as_dict() == dict(r.visibility_info().as_dict(), set=1, n_hidden=int(hidden.sum()))
    rec = r.probe_triangles(boxes=False)
    assert np.all(bits(rec[hidden, 3:]) == 0) and np.array_equal(bits(rec), bits(V.hide(*V.visible_records(scene.vertex, scene.face, tuple(r.info().centre)), mask)[0]))
    with pytest.raises(pkg.McptError):
        r.probe_triangles()                                                  # the boxes are in the old leaf order until the next update
    _assert_same_rays(before, _full_state(pkg, r), identity, hidden)          # hidden stays hidden: the per-ray answers are kept
    ratio = r.update_info().wide_area_ratio
    r.update_vertices(scene.vertex)                                          # ... and the next update tightens the boxes again
    assert r.update_info().wide_area_ratio < ratio
    _assert_records(pkg, r, scene, mask)
    _assert_same_rays(before, _full_state(pkg, r), identity, hidden)
    r.set_face_visibility(None)
    o = _ctx(pkg, scene)
    o.update_vertices(scene.vertex)
    _assert_same_rays(_full_state(pkg, r), _full_state(pkg, o), identity)     # hide-then-show's state, up to the new trees
    assert r.visibility_info().set == 0
    r.close(); o.close()


@pytest.mark.gpu
def test_reprojection_carries_the_film_across_the_change(pkg):
    scene, mask = _hidden_sphere(pkg)
    opts = dict(feature_spp=4, feature_seed=SEED_F, max_history=64.0)
    r = _ctx(pkg, scene)
    r.render(16, seed=3); r.render_features(4, seed=SEED_F)
    film, feat_a = r.read_accum(), r.features()
    paths = r.counters().paths
    r.set_face_visibility_reproject(mask, **opts)
    got, feat_b = r.read_accum(), r.features()
    hit_b, uvt_b = r.probe_first_hits()
    assert not (mask == 0)[hit_b[hit_b >= 0]].any()
    want, reused = r.probe_reproject_motion(scene.camera, scene.camera, film, feat_a, feat_b, hit_b, uvt_b[..., :2], max_history=64.0)
    assert np.array_equal(bits(got), bits(want))
    ri = r.reproject_info()
    assert ri.reprojections == 1 and ri.pixels_reused == reused and 0.5 * got.shape[0] * got.shape[1] < reused < got.shape[0] * got.shape[1]
    assert r.update_info().updates == 1 and r.visibility_info().updates == 1 and r.counters().paths == paths
    _assert_records(pkg, r, scene, mask)
    r.close()
    # an all-visible mask changes nothing: the call is update_vertices_reproject with the vertices as they are
    a, b = _ctx(pkg, scene), _ctx(pkg, scene)
    for c in (a, b):
        c.render(16, seed=3)
    a.set_face_visibility_reproject(np.ones_like(mask), **opts)
    b.update_vertices_reproject(scene.vertex, **opts)
    assert np.array_equal(bits(a.read_accum()), bits(b.read_accum())) and np.array_equal(bits(a.features()), bits(b.features()))
    assert a.reproject_info().pixels_reused == b.reproject_info().pixels_reused
    assert (a.visibility_info().set, a.visibility_info().n_hidden) == (1, 0)
    K.assert_same(_full_state(pkg, a), _full_state(pkg, b))
    a.close(); b.close()


@pytest.mark.gpu
def test_facade_set_visible(pkg, tmp_path):
    exe = kit.build_facade("facade_visibility.cpp", tmp_path)
    a = pkg.scenes.cornell_box(44, 30, sphere_lon=24, sphere_lat=12)
    obj = a.write(str(tmp_path / "a"))
    outs = [str(tmp_path / n) for n in ("hidden.bin", "shown.bin", "rp.bin")]
    k = 4
    line = kit.run_facade(exe, [obj, "glossy", str(k)] + outs)
    w, h = int(line[0]), int(line[1])
    assert (w, h, int(line[2])) == (44, 30, k)
    hidden, shown, rp = [np.fromfile(p, np.float32).reshape(h, w, 4) for p in outs]
    r = _ctx(pkg, a)

    def film():                                                              # Render::render k times: one sample each, numbered from 0, of the program's seed
        r.clear()
        for i in range(k):
            r.render(1, seed=17, first_sample=i)
        return r.read_accum()

    r.set_face_visibility(pkg.visibility_from_materials(a, [K.SPHERE]))
    assert np.array_equal(bits(hidden), bits(film()))
    r.set_face_visibility(None)
    assert np.array_equal(bits(shown), bits(film())) and not np.array_equal(hidden, shown)
    assert np.all(rp[..., 3] >= 1) and np.all(rp[..., 3] <= 5) and (rp[..., 3] > 1).mean() > 0.5   # history capped at 4, plus the new frame
    r.close()


@pytest.mark.gpu
def test_cli_hide_and_blink(pkg, tmp_path):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    frames = {}
    for name, extra in (("plain", []), ("blink", ["--blink", "glossy", "2"]), ("hide", ["--hide", "glossy"])):
        out = str(tmp_path / name)
        p = kit.run_cli([obj, "--turntable", "4", "--spp", "4", "--depth", "5", "--deterministic", "--out", out] + extra)
        assert p.returncode == 0, p.stderr[-2000:]
        frames[name] = kit.turntable_frames(out, 4)
    assert frames["blink"][:2] == frames["plain"][:2]                        # visible on frames 0 and 1 ...
    assert frames["blink"][2] != frames["plain"][2] and frames["blink"][3] != frames["plain"][3]
    assert frames["blink"][2:] == frames["hide"][2:]                         # ... hidden on 2 and 3, as --hide hides it
    assert frames["hide"][0] != frames["plain"][0]
    out = str(tmp_path / "rp")
    p = kit.run_cli([obj, "--turntable", "4", "--spp", "4", "--depth", "5", "--reproject", "8", "--blink", "glossy", "1", "--out", out])
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(set(kit.turntable_frames(out, 4))) == 4
    for bad, word in ((["--hide", "nobody"], "no material named"), (["--blink", "glossy", "0"], "K >= 1"), (["--hide", "glossy", "--wobble", "0.01"], "--hide")):
        p = kit.run_cli([obj, "--turntable", "2", "--spp", "1", "--out", out] + bad)
        assert p.returncode in (1, 2) and word in p.stderr, p.stderr[-500:]
