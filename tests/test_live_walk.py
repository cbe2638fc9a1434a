"""Random walks over the live-scene API against a history-free context: one context gets groups, a skin, morph targets,
keyframes, an image texture and a constant colour set at the start and is then driven through a seeded list of ops of every kind -- all deformer
routes in both forms, owners and parts updates, auto normals, material, light and texture edits, the mask, rebuilds with every builder, camera
moves, clones, renders, feature and denoise calls, refused calls.  tests/live_model.py keeps the books.  After every step but a render the cheap read-backs are
held to the model; at every 8th step and at the end the context is held, bit for bit, to a context that reaches the same scene by the shortest
history the model describes (live_model.history), and at the end of a walk that leaves a mask set also to the SUB-SCENE context of
tests/test_visibility.py, which uses none of the visibility code.

What is by design, with the source that makes it so (csrc/mcpt_api.cpp); the model follows each, and nothing is compared more loosely for it:
  * rf_forget_derived is called by apply_camera, rf_enqueue_update, mcpt_update_materials and mcpt_update_texture only.  mcpt_rebuild_trees keeps
    the features, the denoised output and the tile error (include/mcpt.h: "film, counters, features ... stay"), and so do the set calls that move
    nothing -- mcpt_set_vertex_owners (set and clear), mcpt_set_auto_normals, mcpt_set_skin_mode: after these ops the derived buffers are NOT
    expected refused.  After every op that moves or recolours the scene, or moves the camera, they are.
  * a reprojecting form renders the new scene's features itself (rp_frame: dn_render_features after rf_enqueue_update): after it the features
    are held, the denoised output and the tile error are not.
  * a clone starts every counter at 0 but the mask's: Visibility::clone_from copies `updates` with the mask ("the source's counter and
    duration"), while rf_clone copies no other deformer's count.
The cheap checks are skipped after a render op, so that the next op is enqueued behind it without a sync; what a render changes, the film's sample
count, is checked at the next checkpoint.

A failure prints the seed, the step and the op list up to it as a Python literal that `_run` accepts.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import deform_kit as K, kit, live_model as L, visibility_ref as V
from tests.deform_kit import _assert_same_rays, _full_state
from tests.kit import bits
from tests.test_update_routes import INCREMENTS

INVALID, NO_LIGHTS = 1, 4
STEPS, EVERY = 48, 8
# (seed, the context is created with FLAG_GPU_BVH_BUILD, auto normals are on from the start)
WALKS = [(973, False, False), (58, False, False), (493, True, False), (891, False, True)]
RP = dict(feature_spp=4, feature_seed=5)


def _ops(walk):
    seed, device, auto = walk
    return L.generate(seed, STEPS, device, auto)


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_the_generator_is_deterministic_per_seed():
    for walk in WALKS:
        assert repr(_ops(walk)) == repr(_ops(walk))
    assert repr(_ops(WALKS[0])) != repr(_ops(WALKS[1]))
    assert eval(repr(_ops(WALKS[0]))) == _ops(WALKS[0])                      # the printed list is the list


def test_every_pose_stays_in_the_room_and_no_op_leaves_the_scene_dark(pkg):
    for walk in WALKS:
        m = L.LiveModel(pkg, auto=walk[2])
        assert L.in_room(m) and m.lights().size == 2
        for step, op in enumerate(_ops(walk)):
            if op[0] == "refuse":
                if op[1]["what"] == "mask":
                    assert m.plan(_dark_mask(m))["n_lights"] == 0
                if op[1]["what"] == "materials":                             # refused because of the mask: without it the sphere would light the scene
                    assert m.plan(materials=L.edited(m.materials, L.ONLY_SPHERE))["n_lights"] == 0
                    assert m.plan(None, L.edited(m.materials, L.ONLY_SPHERE))["n_lights"] > 2000
                continue
            m.apply(op)
            assert L.in_room(m), (walk, step, op)
            assert m.lights().size > 0 and m.lights().size == m.plan()["n_lights"], (walk, step, op)


def _followed(ops, event, then):
    """Is there an op satisfying `event` with an op satisfying `then` later in the list?"""
    first = next((i for i, op in enumerate(ops) if event(op)), None)
    return first is not None and any(then(op) for op in ops[first + 1:])


def _mask_drops(ops):
    """The indices of the ops that drop a mask that is in force."""
    out = []; set_ = False
    for i, (kind, a) in enumerate(ops):
        if kind == "visibility":
            if a["what"] == "none" and set_:
                out.append(i)
            set_ = a["what"] != "none"
    return out


def test_the_committed_seeds_cover_every_op_and_every_order_that_matters(pkg):
    walks = [_ops(w) for w in WALKS]
    every = [op for ops in walks for op in ops]
    kinds = [L.KIND[k] for k, _ in every] + [16 for _, a in every if a.get("reproject")]
    for k in range(1, 18):
        assert kinds.count(k) >= 2, k
    names = {k for k, _ in every}
    assert names == set(L.KIND)
    has = lambda kind, **kw: any(k == kind and all(a.get(x) == y for x, y in kw.items()) for k, a in every)
    for normals in (False, True):
        assert has("vertices", normals=normals)
    assert has("morph", bones=None) and any(k == "morph" and a["bones"] is not None for k, a in every)
    assert has("skin", mode=0) and has("skin", mode=1)
    assert has("owners", layout=None) and has("owners", layout=0) and has("owners", layout=1)
    assert any(k == "parts" and sum(a[x] is not None for x in ("groups", "bones", "weights", "time")) >= 2 for k, a in every)
    assert has("parts", morph_then_skin=True)
    for which in ("sphere", "all", "off"):
        assert has("auto_normals", mask=which)
    for edit in ("glow", "unglow", "dim", "mirror"):
        assert has("materials", edit=edit)
    assert has("texture", index=L.TILES) and has("texture", index=L.RED)
    for what in ("subset", "sphere", "none"):
        assert has("visibility", what=what)
    for builder in (0, L.HOST, L.DEVICE):
        assert has("rebuild", builder=builder)
    for what in ("n_materials", "bone", "mask", "materials"):
        assert has("refuse", what=what)
    for kind in L.ROUTES + ("visibility",):                                    # op 16: the _reproject form of 1 - 6 and 10
        assert has(kind, reproject=True) and has(kind, reproject=False)
    # the sphere turned into an emitter and later back
    assert any(_followed(ops, lambda o: o == ("materials", {"edit": "glow"}), lambda o: o == ("materials", {"edit": "unglow"})) for ops in walks)
    events = {"mask set": lambda o: o[0] == "visibility" and o[1]["what"] != "none", "list grows": lambda o: o == ("materials", {"edit": "glow"}),
              "rebuild": lambda o: o[0] == "rebuild", "clone": lambda o: o[0] == "clone"}
    for name, event in events.items():
        for later in L.ROUTES + ("texture",):
            assert any(_followed(ops, event, lambda o: o[0] == later) for ops in walks), (name, later)
    # a mask dropped: a None op while a mask is in force (the generator draws no other, and this test does not rely on that)
    for ops in walks:
        assert all(i in _mask_drops(ops) for i, o in enumerate(ops) if o[0] == "visibility" and o[1]["what"] == "none")
    for later in L.ROUTES + ("texture",):
        assert any(any(o[0] == later for o in ops[drops[0] + 1:]) for ops in walks for drops in [_mask_drops(ops)] if drops), ("mask dropped", later)
    # the light list reallocates through both of its growing callers: the materials edit and a mask change (mt_ensure_list from vs_set)
    grown = []
    for walk, ops in zip(WALKS, walks):
        m = L.LiveModel(pkg, auto=walk[2])
        for op in ops:
            if op[0] != "refuse":
                m.apply(op)
        grown += m.grown_by
    assert "materials" in grown and "visibility" in grown


def test_the_model_without_ops_has_the_empty_history(pkg):
    assert L.history(L.LiveModel(pkg)) == []
    m = L.LiveModel(pkg); m.apply(("render", {"n": 2})); m.apply(("texture", {"index": L.RED, "seed": 1})); m.apply(("materials", {"edit": "glow"}))
    assert L.history(m) == []                                                # materials and textures are the oracle's creation scene
    m.apply(("rebuild", {"builder": 0}))
    assert [c[0] for c in L.history(m)] == ["update_vertices", "rebuild"]
    m.apply(("vertices", {"sphere": [10.0, 0.0, 0.1, 0.0], "lamp": [0.0, 0.0, 0.1, 0.0], "normals": False, "reproject": False}))
    h = L.history(m)
    assert [c[0] for c in h] == ["update_vertices", "rebuild", "update_vertices"] and np.array_equal(h[2][1], m.vertex) and np.array_equal(h[2][2], m.normal)


def test_the_models_counters_are_the_increments_of_the_update_routes(pkg):
    pose = {"sphere": [10.0, 0.0, 0.1, 0.0], "lamp": [0.0, 0.0, 0.1, 0.0]}
    bones = [pose["sphere"]] * 3 + [pose["lamp"]]
    ops = {"arrays": ("vertices", dict(pose, normals=True)), "groups": ("transforms", dict(pose)), "skin": ("skin", {"mode": 0, "bones": bones}),
           "morph": ("morph", {"weights": [-0.1, 0.5], "bones": None}), "morph+bones": ("morph", {"weights": [-0.1, 0.5], "bones": bones}), "normals": ("normals", {})}
    assert set(ops) == set(INCREMENTS)
    for auto in (False, True):
        for reproject in (False, True):
            for route, (kind, a) in ops.items():
                if kind == "normals" and (reproject or not auto):
                    continue
                m = L.LiveModel(pkg, auto=auto)
                m.apply((kind, dict(a, reproject=reproject)))
                got = tuple(m.count[k] for k in ("update", "transform", "skin", "morph", "normals", "reproject"))
                assert got == INCREMENTS[route] + (1 if kind == "normals" else int(auto), int(reproject)), (route, auto, reproject)


# ------------------------------------------------------------------------------------------------------------------------ GPU: the walk
def _scene(pkg, m):
    s = m.fx.scene
    return pkg.scenes.SceneData(s.name, s.vertex, s.normal, s.texcoord, s.face, list(m.materials), s.camera, dict(s.meta))


def _dark_mask(m):
    """Every emitter hidden, the lamp included."""
    mask = np.ones(m.fx.face_material.shape[0], np.uint8) if m.mask is None else m.mask.copy()
    mask[V.emits(m.materials)[m.fx.face_material]] = 0
    return mask


def _counters(r):
    return {"update": r.update_info().updates, "transform": r.transform_info().updates, "skin": r.skin_info().updates, "morph": r.morph_info().updates,
            "keyframe": r.keyframe_info().updates, "parts": r.parts_info().updates, "normals": r.normals_info().updates,
            "visibility": r.visibility_info().updates, "material": r.material_info().updates, "rebuild": r.rebuild_info().rebuilds,
            "reproject": r.reproject_info().reprojections}


def _snapshot(r):
    """What a refused call must leave as it was: the infos, the arrays, the light list's bits."""
    i = r.info()
    scene = [getattr(i, k) if k != "centre" else tuple(i.centre) for k, _ in i._fields_ if k != "upload_ms"]
    vi = r.visibility_info()
    return {"scene": scene, "counters": _counters(r), "visibility": (vi.set, vi.n_hidden, vi.n_hidden_emitters), "n_lights": r.material_info().n_lights,
            "mode": r.skin_mode(), "arrays": [bits(x).copy() for x in r.vertices()], "lights": [bits(x).copy() for x in r.probe_lights()]}


def _same_snapshot(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k in ("arrays", "lights"):
            assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
        else:
            assert a[k] == b[k], k


def _refused(pkg, call, status):
    with pytest.raises(pkg.McptError) as e:
        call()
    assert "status %d" % status in str(e.value)


def _do(pkg, r, m, op):
    """The op on the context; `m` is the model BEFORE it.  Returns the context the walk goes on with."""
    kind, a = op
    fx = m.fx
    form = "_reproject" if a.get("reproject") else ""
    opts = RP if form else {}
    if kind == "vertices":
        v, n = L.pose_arrays(fx, a["sphere"], a["lamp"])
        getattr(r, "update_vertices" + form)(v, n if a["normals"] else None, **opts)
    elif kind == "transforms":
        getattr(r, "update_transforms" + form)(L.group_matrices(a), **opts)
    elif kind == "skin":
        r.set_skin_mode(pkg.SKIN_DUAL_QUATERNION if a["mode"] else pkg.SKIN_LINEAR)
        getattr(r, "update_skin" + form)(L.bone_matrices(a["bones"]), **opts)
    elif kind == "morph":
        getattr(r, "update_morph" + form)(a["weights"], None if a["bones"] is None else L.bone_matrices(a["bones"]), **opts)
    elif kind == "keyframes":
        getattr(r, "update_keyframes" + form)(a["time"], **opts)
    elif kind == "owners":
        if a["layout"] is None: r.clear_vertex_owners()
        else: r.set_vertex_owners(fx.owners[a["layout"]], fx.owners[a["layout"]])
    elif kind == "parts":
        getattr(r, "update_parts" + form)(groups=None if a["groups"] is None else L.group_matrices(a["groups"]),
                                          bones=None if a["bones"] is None else L.bone_matrices(a["bones"]), weights=a["weights"], time=a["time"],
                                          morph_then_skin=a["morph_then_skin"], **opts)
    elif kind == "auto_normals":
        if a["mask"] == "off": r.set_auto_normals(mode=pkg.NORMALS_OFF)
        else: r.set_auto_normals(None if a["mask"] == "all" else fx.sphere.astype(np.uint8))
    elif kind == "normals":
        r.update_normals()
    elif kind == "materials":
        r.update_materials(L.edited(m.materials, L.EDITS[a["edit"]]))
    elif kind == "texture":
        r.update_texture(a["index"], L.texels(fx, a["index"], a["seed"]))
    elif kind == "visibility":
        getattr(r, "set_face_visibility" + form)(L.subset_mask(fx, a["what"], a["seed"]), **opts)
    elif kind == "rebuild":
        r.rebuild(a["builder"])
    elif kind == "camera":
        r.set_camera(L.camera(pkg, fx, a["eye"]))
    elif kind == "clone":
        c = r.clone(0); r.close()
        return c
    elif kind == "render":
        r.render(a["n"], seed=5, first_sample=m.samples)
    elif kind == "features":
        r.render_features(4, seed=5)
        if a["denoise"]: r.denoise()
        if a["adaptive"]: r.render_adaptive(seed=5, first_sample=m.samples, min_spp=2, max_spp=2)
    else:
        assert kind == "refuse"
        before = _snapshot(r)
        if a["what"] == "n_materials":
            _refused(pkg, lambda: r.update_materials(m.materials[:-1]), INVALID)
        elif a["what"] == "bone":
            bad = L.bone_matrices([[0.0, 0.0, 0.1, 0.0]] * 4); bad[2, 1, 3] = np.nan
            _refused(pkg, lambda: r.update_skin(bad), INVALID)
        elif a["what"] == "mask":
            _refused(pkg, lambda: r.set_face_visibility(_dark_mask(m)), NO_LIGHTS)
        else:
            _refused(pkg, lambda: r.update_materials(L.edited(m.materials, L.ONLY_SPHERE)), NO_LIGHTS)
        _same_snapshot(before, _snapshot(r))
    if form:
        r.clear()                                                            # the carried film's counts are the reprojection suites' business
    return r


def _cheap(pkg, r, m):
    """After every step: the arrays, the light counts, the counters, the light list's faces, and which derived buffers can be read."""
    K.assert_arrays(r, m.vertex, m.normal)
    plan = m.plan()
    vi = r.visibility_info()
    assert r.info().n_lights == r.material_info().n_lights == plan["n_lights"]
    assert (vi.set, vi.n_hidden, vi.n_hidden_emitters) == (int(m.mask is not None), plan["n_hidden"], plan["n_hidden_emitters"])
    assert _counters(r) == m.count
    assert r.skin_mode() == int(m.dq)
    faces = r.probe_lights()[0]
    assert np.all(np.diff(faces) > 0) and np.array_equal(faces, m.lights())
    if m.refit_ever:                                                         # the triangle records a refit wrote, hidden faces shrunk to a point (visibility_ref)
        rec, box = V.hide(*V.visible_records(m.vertex, m.fx.scene.face, tuple(r.info().centre)), m.mask)
        assert np.array_equal(bits(r.probe_triangles(boxes=False)), bits(rec))
        if m.box_valid:                                                      # (not after a rebuild or a clone: the boxes are scratch of the update)
            assert np.array_equal(bits(r.probe_triangles()[1]), bits(box))
        else:
            _refused(pkg, r.probe_triangles, INVALID)
    out = np.zeros((r.height, r.width, 4), np.float32)
    for name, held, read in (("features", m.features, r.features), ("denoised", m.denoised, lambda: r._check(r.lib.mcpt_read_denoised(r.ctx, pkg._ptr(out)))),
                             ("tile error", m.tile_error, r.tile_error)):
        if held:
            read()
        else:
            with pytest.raises(pkg.McptError) as e:
                read()
            assert "status %d" % INVALID in str(e.value), name


def _look(pkg, r, both_boxes):
    lp, lxi = kit.light_points(0.0, 1.0, 4096, 11)
    s = _full_state(pkg, r)                                                   # (validate_trees, both traversals, shade records, light list, the 4-spp film)
    s["classes"] = r.probe_face_classes(); s["sample_light"] = r.probe_sample_light(lp, lxi)
    if both_boxes:
        s["records"], s["boxes"] = r.probe_triangles()
    else:
        s["records"] = r.probe_triangles(boxes=False)
    return s


def _checkpoint(pkg, r, m, flags, end):
    assert np.all(r.read_accum()[..., 3] == m.samples)                       # every render since the last clear, and nothing else
    calls = L.history(m)
    o = pkg.Renderer(_scene(pkg, m), max_depth=6, flags=flags)
    for call in calls:
        getattr(o, call[0])(*call[1:])
    boxes = m.box_valid and m.refit_since_rebuild                            # rf_tri_box is current on both: an update since creation, clone or rebuild
    a = _look(pkg, r, boxes); m.samples = 4
    K.assert_same(a, _look(pkg, o, boxes))
    o.close()
    if end and m.mask is not None:                                           # the second oracle: the hidden rows of `face` deleted
        sub, new_of_old = V.sub_scene(pkg, _scene(pkg, m), m.mask)
        s = pkg.Renderer(sub, max_depth=6, flags=flags)
        s.update_vertices(m.vertex, m.normal); s.set_camera(m.camera)
        _assert_same_rays(a, _full_state(pkg, s), new_of_old, m.hidden())
        s.close()


def _run(ops, device=False, auto=False, seed=None):
    """Walk `ops` on a fresh context: the cheap checks after every step (after a render none: the next op is enqueued behind it, without a sync),
    the oracle at every 8th step and at the end."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    flags = K.FLAGS(pkg) | (pkg.FLAG_GPU_BVH_BUILD if device else 0)
    m = L.LiveModel(pkg); fx = m.fx
    r = pkg.Renderer(fx.scene, max_depth=6, flags=flags)
    fx.setup(pkg, r)
    if auto:
        first = ("auto_normals", {"mask": "sphere"})
        r = _do(pkg, r, m, first); m.apply(first)
    step = -1
    try:
        _cheap(pkg, r, m)
        for step, op in enumerate(ops):
            r = _do(pkg, r, m, op)
            if op[0] != "refuse":
                m.apply(op)
            if op[0] != "render":
                _cheap(pkg, r, m)
            if (step + 1) % EVERY == 0 or step + 1 == len(ops):
                _checkpoint(pkg, r, m, flags, step + 1 == len(ops))
    except BaseException:
        print("\nlive walk failed: seed %r, device builder %r, auto normals %r, at step %d\n_run(%r, device=%r, auto=%r)" %
              (seed, device, auto, step, ops[:step + 1], device, auto))
        raise
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("walk", WALKS, ids=lambda w: "seed%d%s%s" % (w[0], "-device" if w[1] else "", "-auto" if w[2] else ""))
def test_walk(walk):
    seed, device, auto = walk
    _run(_ops(walk), device, auto, seed)
