"""A host model of a live context and the seeded generator of the op lists tests/test_live_walk.py walks: what a context
holds after ANY history of the live-scene calls -- the vertex and normal arrays, materials and textures, the mask, the camera, the skinning mode,
the auto-normal lists, the owners, every counter, what the trees were last built from, the samples in the film and which derived buffers are
current -- and the SHORTEST history that describes the same scene (`history`).

Nothing of a kernel is restated here.  Poses come from the deformers' restatements (transform_ref, skin_ref, skin_dq_ref, morph_ref, keyframes_ref,
parts_ref, normals_ref) and the light counts from visibility_ref; the model only keeps the books the C ABI layer keeps (csrc/mcpt_api.cpp).

An op is a pair (kind, arguments) of Python literals: a list of them printed is a list `_run` of the walk accepts.  Everything large -- a mask, a
pose, texels -- is derived from the few numbers the op carries (`Fixture` and the functions below), the same way on every replay.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from tests import deform_kit as K, keyframes_ref as F, morph_ref as M, normals_ref as N, parts_ref as P, skin_dq_ref as DQ, skin_ref as S
from tests import transform_ref as T, visibility_ref as V

WHITE, RED, GREEN, LAMP, SPHERE, TILES = range(6)                            # materials: S-cornell's five and the floor's image texture
N_GROUPS, N_BONES, N_TARGETS, N_FRAMES = 3, K.N_BONES, 2, 3
LAMP_PIVOT = (0.5, 0.999, 0.5)
DIM = 0.005 / np.sqrt(3.0)                                                   # |radiance| = 0.005: emissive, but below the list's 0.01
GLOW = (0.8, 0.5, 0.3)
HOST, DEVICE = 1, 2                                                          # REBUILD_HOST, REBUILD_DEVICE (0: the builder of creation)
COUNTERS = ("update", "transform", "skin", "morph", "keyframe", "parts", "normals", "visibility", "material", "rebuild", "reproject")
# the issue's op kinds by number, for the coverage test; 16 is any op with reproject = True
KIND = {"vertices": 1, "transforms": 2, "skin": 3, "morph": 4, "keyframes": 5, "owners": 6, "parts": 6, "auto_normals": 7, "normals": 7, "materials": 8,
        "texture": 9, "visibility": 10, "rebuild": 11, "camera": 12, "clone": 13, "render": 14, "features": 15, "refuse": 17}
ROUTES = ("vertices", "transforms", "skin", "morph", "keyframes", "parts")   # the deformer routes 1 - 6
EDITS = {"glow": {SPHERE: dict(radiance=GLOW)}, "unglow": {SPHERE: dict(radiance=(0.0, 0.0, 0.0))}, "dim": {SPHERE: dict(radiance=(DIM, DIM, DIM))},
         "mirror": {SPHERE: dict(ks=(0.5, 0.5, 0.5), ns=10000.0)}, "gloss": {SPHERE: dict(ks=(0.5, 0.5, 0.5), ns=50.0)},
         "matt": {SPHERE: dict(ks=(0.0, 0.0, 0.0))}, "shiny walls": {WHITE: dict(ks=(0.2, 0.2, 0.2), ns=50.0)}, "plain walls": {WHITE: dict(ks=(0.0, 0.0, 0.0))},
         "lamp colour": {LAMP: dict(radiance=(4.0, 9.0, 14.0))}, "lamp": {LAMP: dict(radiance=(17.0, 12.0, 4.0))}}
# (for the refusal alone: the lamp dark and the sphere the only emitter)
ONLY_SPHERE = {SPHERE: dict(radiance=GLOW), LAMP: dict(radiance=(0.0, 0.0, 0.0))}


# ------------------------------------------------------------------------------------------------------------------------ the fixture
class Fixture:
    """deform_kit.scene with a sixth material -- an 8 x 8 image texture on the floor; the red wall's 1 x 1 texture is the constant colour -- and
    everything the set calls of the walk's context take."""

    def __init__(self, pkg):
        base = K.scene(pkg)
        face = base.face.copy(); face[0:2, :, 3] = TILES                     # the floor's two triangles
        tiles = dataclasses.replace(base.materials[WHITE], name="tiles", texture=pkg.scenes.value_noise_texture(8, 9, (0.2, 0.6, 0.3), 0.3))
        self.scene = pkg.scenes.SceneData(base.name, base.vertex, base.normal, base.texcoord, face, list(base.materials) + [tiles], base.camera, dict(base.meta))
        s = self.scene
        self.face_material = face[:, 0, 3].copy()
        assert (base.face[0:2, 0, 3] == WHITE).all() and np.abs(base.vertex[face[0:2, :, 0], 1]).max() == 0.0   # (the floor)
        self.sphere, self.lamp = K.parts(pkg)                                # boolean per vertex; normal k belongs to vertex k in these scenes
        assert np.array_equal(face[:, :, 0], face[:, :, 1]) and s.vertex.shape == s.normal.shape
        self.sphere_faces = np.flatnonzero(self.face_material == SPHERE); self.lamp_faces = np.flatnonzero(self.face_material == LAMP)
        group = np.where(self.sphere, 1, np.where(self.lamp, 2, 0)).astype(np.uint32)
        self.groups = (group, group)
        self.skin = K.bend(pkg)
        vi = np.flatnonzero(self.sphere); rng = np.random.default_rng(17)
        nudge = rng.uniform(-0.02, 0.02, (len(vi[::5]), 3)); nudge[:, 1] = np.abs(nudge[:, 1])     # (upwards: the sphere stands on the floor)
        self.vertex_targets = [(vi, s.vertex[vi] - K.CENTRE), (vi[::5], nudge)]
        self.normal_targets = [(vi, rng.uniform(-0.3, 0.3, (len(vi), 3))), (vi[::5], rng.uniform(-0.3, 0.3, (len(vi[::5]), 3)))]
        vf = np.repeat(s.vertex[None], N_FRAMES, 0); nf = np.repeat(s.normal[None], N_FRAMES, 0)
        vf[1], nf[1] = pose_arrays(self, (20.0, 0.12, 0.25, -0.1), (10.0, 0.05, 0.2, 0.0))
        vf[2], nf[2] = pose_arrays(self, (-35.0, -0.1, 0.1, 0.1), (-20.0, -0.1, 0.05, 0.1))
        self.frames = (vf, nf)
        y = s.vertex[:, 1]
        band = np.where(y < 0.2, P.KEYFRAMES, np.where(y < 0.4, P.SKIN, P.MORPH))
        self.owners = [np.where(self.sphere, band, np.where(self.lamp, P.GROUPS, P.NONE)).astype(np.uint8),
                       np.where(self.sphere, P.SKIN, np.where(self.lamp, P.KEYFRAMES, P.NONE)).astype(np.uint8)]

    def setup(self, pkg, r):
        """Everything set at the start: each call takes the scene as it is -- the creation arrays -- as its rest pose."""
        r.set_vertex_groups(self.groups[0], self.groups[1], N_GROUPS); r.set_vertex_skin(*self.skin, N_BONES)
        r.set_vertex_morph(self.vertex_targets, self.normal_targets); r.set_vertex_keyframes(self.frames[0], self.frames[1])


@functools.lru_cache(maxsize=None)
def fixture(pkg):
    return Fixture(pkg)


def rigid(pose):
    """(degrees about z, shift x, y, z): the sphere turned about its centre and moved."""
    return K.clean(T.about(T.rotation((0, 0, 1), pose[0]), K.CENTRE, pose[1:4]))


def lamp_matrix(pose):
    """(degrees about y, shift x, DOWN by y, z): the lamp turned about its middle and lowered."""
    return K.clean(T.about(T.rotation((0, 1, 0), pose[0]), LAMP_PIVOT, (pose[1], -pose[2], pose[3])))


def pose_arrays(fx, sphere, lamp):
    """The caller's arrays of update_vertices: the creation scene with the sphere and the lamp moved rigidly, normals turned with them."""
    s = fx.scene
    v = s.vertex.copy(); n = s.normal.copy()
    for part, m in ((fx.sphere, rigid(sphere)), (fx.lamp, lamp_matrix(lamp))):
        v[part] = v[part] @ m[:, :3].T + m[:, 3]; n[part] = n[part] @ m[:, :3].T
    return v, n


def group_matrices(a):
    return np.stack([T.identity(1)[0], rigid(a["sphere"]), lamp_matrix(a["lamp"])])


def bone_matrices(b):
    """[low, high, third, lamp]: bone 0 holds the walls and stays the identity; all rigid, as dual-quaternion mode asks."""
    return K.mats(low=rigid(b[0]), high=rigid(b[1]), third=rigid(b[2]), lamp=lamp_matrix(b[3]))


def subset_mask(fx, what, seed):
    """The mask of a visibility op: None, every sphere face hidden, or a random subset of them."""
    if what == "none":
        return None
    m = np.ones(fx.scene.face.shape[0], np.uint8)
    m[fx.sphere_faces] = 0 if what == "sphere" else np.random.default_rng(seed).uniform(size=fx.sphere_faces.size) < 0.5
    return m


def texels(fx, index, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.05, 0.9, (8, 8, 3) if index == TILES else (1, 1, 3)).astype(np.float32)


def camera(pkg, fx, eye):
    c = fx.scene.camera
    return pkg.scenes.Camera(tuple(eye), c.lookat, c.up, c.fovy, c.width, c.height)


def edited(materials, edit):
    out = list(materials)
    for i, fields in edit.items():
        out[i] = dataclasses.replace(out[i], **fields)
    return out


# ------------------------------------------------------------------------------------------------------------------------ the model
class LiveModel:
    def __init__(self, pkg, auto=False):
        self.pkg = pkg; self.fx = fx = fixture(pkg)
        s = fx.scene
        self.vertex = s.vertex.copy(); self.normal = s.normal.copy()
        self.materials = list(s.materials)
        self.mask = None; self.camera = s.camera
        self.dq = False; self.auto = None; self.owners = None                # auto: the (offset, entry) lists of the normals pass
        self.count = dict.fromkeys(COUNTERS, 0)
        self.refit_ever = False; self.refit_since_rebuild = False
        self.rebuilt = None                                                  # the state the trees were last built from
        self.box_valid = False
        self.samples = 0
        self.features = self.denoised = self.tile_error = False
        self.ops = 0
        self.capacity = 2                                                    # entries the light list has room for: it only grows (mt_ensure_list)
        self.grown_by = []                                                   # the kinds of the ops that made it reallocate
        if auto:
            self.apply(("auto_normals", {"mask": "sphere"}))

    # ---- what the infos report
    def plan(self, mask="current", materials=None):
        return V.plan(self.mask if isinstance(mask, str) else mask, self.fx.face_material, V.emits(self.materials if materials is None else materials))

    def lights(self):
        """The faces of the light list, ascending."""
        visible = np.ones(self.fx.face_material.shape[0], bool) if self.mask is None else self.mask != 0
        return np.flatnonzero(V.emits(self.materials)[self.fx.face_material] & visible)

    def hidden(self):
        return np.zeros(self.fx.face_material.shape[0], bool) if self.mask is None else self.mask == 0

    # ---- the one path of every scene update (rf_enqueue_update)
    def _refit(self, reproject=False):
        if self.auto is not None:
            self.normal = N.apply(self.auto[0], self.auto[1], self.vertex, self.normal); self.count["normals"] += 1
        self.count["update"] += 1
        self.refit_ever = self.refit_since_rebuild = True; self.box_valid = True
        self.features = self.denoised = self.tile_error = False
        if reproject:                                                        # rp_frame renders the new scene's features; the walk clears the carried film
            self.count["reproject"] += 1; self.features = True; self.samples = 0

    def _skin(self, v, n, bones):
        R = DQ if self.dq else S
        vb, vw, nb, nw = self.fx.skin
        return R.skin_vertices(v, vb, vw, bones), R.skin_normals(n, nb, nw, bones)

    def _morph(self, weights, bones):
        s = self.fx.scene
        v = M.morph_vertices(s.vertex, self.fx.vertex_targets, weights); n = M.morph_normals(s.normal, self.fx.normal_targets, weights)
        return (v, n) if bones is None else self._skin(v, n, bones)

    def _keyframes(self, time):
        return F.play_vertices(self.fx.frames[0], time), F.play_normals(self.fx.frames[1], time)

    def apply(self, op):
        """The exact effect of one op that is not refused."""
        self._apply(op)
        if self.lights().size > self.capacity:                               # (by the materials edit or by a mask change; a clone copies the list as long as it is)
            self.capacity = int(self.lights().size); self.grown_by.append(op[0])

    def _apply(self, op):
        kind, a = op
        fx = self.fx; s = fx.scene; c = self.count
        rp = bool(a.get("reproject"))
        self.ops += 1
        if kind == "vertices":
            v, n = pose_arrays(fx, a["sphere"], a["lamp"])
            self.vertex = v
            if a["normals"]: self.normal = n
            self._refit(rp)
        elif kind == "transforms":
            m = group_matrices(a)
            self.vertex = T.transform_vertices(s.vertex, fx.groups[0], m); self.normal = T.transform_normals(s.normal, fx.groups[1], m)
            c["transform"] += 1; self._refit(rp)
        elif kind == "skin":
            self.dq = bool(a["mode"])
            self.vertex, self.normal = self._skin(s.vertex, s.normal, bone_matrices(a["bones"]))
            c["skin"] += 1; self._refit(rp)
        elif kind == "morph":
            bones = None if a["bones"] is None else bone_matrices(a["bones"])
            self.vertex, self.normal = self._morph(a["weights"], bones)
            c["morph"] += 1; c["skin"] += bones is not None; self._refit(rp)
        elif kind == "keyframes":
            self.vertex, self.normal = self._keyframes(a["time"])
            c["keyframe"] += 1; self._refit(rp)
        elif kind == "owners":
            self.owners = None if a["layout"] is None else fx.owners[a["layout"]]
        elif kind == "parts":
            assert self.owners is not None
            out = {}
            bones = None if a["bones"] is None else bone_matrices(a["bones"])
            if a["groups"] is not None:
                m = group_matrices(a["groups"])
                out[P.GROUPS] = (T.transform_vertices(s.vertex, fx.groups[0], m), T.transform_normals(s.normal, fx.groups[1], m)); c["transform"] += 1
            if bones is not None:
                out[P.SKIN] = self._skin(s.vertex, s.normal, bones); c["skin"] += 1
            if a["weights"] is not None:
                then_skin = bool(a["morph_then_skin"])
                out[P.MORPH] = self._morph(a["weights"], bones if then_skin else None); c["morph"] += 1; c["skin"] += then_skin
            if a["time"] is not None:
                out[P.KEYFRAMES] = self._keyframes(a["time"]); c["keyframe"] += 1
            self.vertex = P.combine(self.vertex, self.owners, {k: x[0] for k, x in out.items()})
            self.normal = P.combine(self.normal, self.owners, {k: x[1] for k, x in out.items()})
            c["parts"] += 1; self._refit(rp)
        elif kind == "auto_normals":
            which = a["mask"]
            self.auto = None if which == "off" else N.per_record(s.face, s.normal.shape[0], self.vertex, self.normal, None if which == "all" else fx.sphere.astype(np.uint8))
        elif kind == "normals":
            assert self.auto is not None
            self._refit()
        elif kind == "materials":
            self.materials = edited(self.materials, EDITS[a["edit"]])
            c["material"] += 1; self.features = self.denoised = self.tile_error = False
        elif kind == "texture":
            t = texels(fx, a["index"], a["seed"]); m = self.materials[a["index"]]
            self.materials[a["index"]] = dataclasses.replace(m, texture=t) if a["index"] == TILES else dataclasses.replace(m, kd=tuple(float(x) for x in t[0, 0]))
            self.features = self.denoised = self.tile_error = False
        elif kind == "visibility":
            self.mask = subset_mask(fx, a["what"], a["seed"])
            c["visibility"] += 1; self._refit(rp)
        elif kind == "rebuild":
            # film, counters, features and denoised output stay (include/mcpt.h: the scene is the same); the boxes are in the old leaf order
            self.rebuilt = dict(vertex=self.vertex.copy(), normal=self.normal.copy(), mask=None if self.mask is None else self.mask.copy(), builder=a["builder"])
            self.refit_since_rebuild = False; self.box_valid = False; c["rebuild"] += 1
        elif kind == "camera":
            self.camera = camera(self.pkg, fx, a["eye"]); self.features = self.denoised = self.tile_error = False
        elif kind == "clone":
            # the scene, the trees, the set-up and the mask travel; the film, the derived buffers, the boxes and every counter but the mask's do not
            self.count = {k: (c[k] if k == "visibility" else 0) for k in COUNTERS}
            self.samples = 0; self.features = self.denoised = self.tile_error = False; self.box_valid = False
        elif kind == "render":
            self.samples += a["n"]
        elif kind == "features":
            self.features = True; self.denoised = bool(a["denoise"])
            if a["adaptive"]:
                self.samples += 2; self.tile_error = True
        else:
            raise ValueError(kind)


def in_room(model):
    """Every vertex of the sphere and the lamp inside the unit room."""
    part = model.fx.sphere | model.fx.lamp
    v = model.vertex[part]
    return bool(np.isfinite(v).all() and v.min() >= 0.0 and v.max() <= 1.0)


# ------------------------------------------------------------------------------------------------------------------------ the shortest history
def _canonical(state_mask, vertex, normal, had_mask):
    calls = []
    if state_mask is not None or had_mask:
        calls.append(("set_face_visibility", state_mask))
    calls.append(("update_vertices", vertex, normal))
    return calls


def history(model):
    """The calls that take a context created from the rest scene -- with the model's materials and textures -- to the model's scene: the state of
    the last rebuild and that rebuild, when there was one; the state now, when a refit has run since, or at all when there was no rebuild; the
    camera, when it moved.  A model without ops has the empty history."""
    calls = []; had_mask = False
    rb = model.rebuilt
    if rb is not None:
        calls += _canonical(rb["mask"], rb["vertex"], rb["normal"], False) + [("rebuild", rb["builder"])]; had_mask = rb["mask"] is not None
    if model.refit_since_rebuild:
        calls += _canonical(model.mask, model.vertex, model.normal, had_mask)
    if model.camera != model.fx.scene.camera:
        calls.append(("set_camera", model.camera))
    return calls


# ------------------------------------------------------------------------------------------------------------------------ the generator
def _r(rng, lo, hi):
    return round(float(rng.uniform(lo, hi)), 3)


def _sphere_pose(rng):
    return [_r(rng, -40, 40), _r(rng, -0.1, 0.1), _r(rng, 0.06, 0.28), _r(rng, -0.1, 0.1)]


def _lamp_pose(rng):
    return [_r(rng, -40, 40), _r(rng, -0.1, 0.1), _r(rng, 0.02, 0.25), _r(rng, -0.1, 0.1)]


def _bones(rng):
    return [_sphere_pose(rng), _sphere_pose(rng), _sphere_pose(rng), _lamp_pose(rng)]


def _weights(rng):
    return [_r(rng, -0.4, 0.0), _r(rng, 0.0, 1.0)]                           # the swell only shrinks: the sphere stands on the floor


def generate(seed, steps=48, device=False, auto=False):
    """The op list of one walk.  The generator keeps only what decides which ops are valid -- the mask's kind, the owners, auto normals, whether
    the sphere glows -- and draws everything else from the seeded stream."""
    rng = np.random.default_rng(seed)
    mask, owners, glows = "none", False, False
    kinds = ["vertices", "transforms", "skin", "morph", "keyframes", "owners", "parts", "auto_normals", "normals", "materials", "texture", "visibility",
             "rebuild", "camera", "clone", "render", "features", "refuse"]
    weight = np.array([2, 2, 2, 2, 2, 1.5, 2.5, 1.5, 1.5, 3, 2, 3, 2, 1, 1, 2, 1.5, 2.5]); weight = weight / weight.sum()
    ops = []
    while len(ops) < steps:
        kind = kinds[int(rng.choice(len(kinds), p=weight))]
        rp = bool(rng.uniform() < 0.25)
        if kind == "vertices":
            a = {"sphere": _sphere_pose(rng), "lamp": _lamp_pose(rng), "normals": bool(rng.uniform() < 0.5), "reproject": rp}
        elif kind == "transforms":
            a = {"sphere": _sphere_pose(rng), "lamp": _lamp_pose(rng), "reproject": rp}
        elif kind == "skin":
            a = {"mode": int(rng.integers(2)), "bones": _bones(rng), "reproject": rp}
        elif kind == "morph":
            a = {"weights": _weights(rng), "bones": _bones(rng) if rng.uniform() < 0.5 else None, "reproject": rp}
        elif kind == "keyframes":
            a = {"time": [0.0, 1.0, 2.0][int(rng.integers(3))] if rng.uniform() < 0.25 else _r(rng, -0.2, 2.2), "reproject": rp}
        elif kind == "owners":
            a = {"layout": None if owners and rng.uniform() < 0.3 else int(rng.integers(2))}; owners = a["layout"] is not None
        elif kind == "parts":
            if not owners:
                continue
            pick = rng.uniform(size=4) < 0.6
            if pick.sum() < 2:
                pick[:] = True
            a = {"groups": {"sphere": _sphere_pose(rng), "lamp": _lamp_pose(rng)} if pick[0] else None, "bones": _bones(rng) if pick[1] else None,
                 "weights": _weights(rng) if pick[2] else None, "time": _r(rng, 0.0, 2.0) if pick[3] else None, "reproject": rp}
            a["morph_then_skin"] = bool(pick[1] and pick[2] and rng.uniform() < 0.5)
        elif kind == "auto_normals":
            a = {"mask": ["sphere", "all", "off"][int(rng.integers(3))]}; auto = a["mask"] != "off"
        elif kind == "normals":
            if not auto:
                continue
            a = {}
        elif kind == "materials":
            names = [k for k in EDITS if (k != "glow" or not glows)]
            p = np.array([4.0 if k in ("glow", "unglow", "dim", "mirror") else 1.0 for k in names])
            a = {"edit": names[int(rng.choice(len(names), p=p / p.sum()))]}
            if a["edit"] in ("glow", "unglow", "dim"): glows = a["edit"] == "glow"
        elif kind == "texture":
            a = {"index": [TILES, RED][int(rng.integers(2))], "seed": int(rng.integers(1 << 16))}
        elif kind == "visibility":
            what = ["subset", "sphere", "none"][int(rng.integers(3))]
            if what == "none" and mask == "none":                            # a mask is dropped only while one is in force
                continue
            a = {"what": what, "seed": int(rng.integers(1 << 16)), "reproject": rp}; mask = what
        elif kind == "rebuild":
            a = {"builder": int(rng.integers(3)) if device else int(rng.integers(2))}      # (a walk without the device builder never asks for it)
        elif kind == "camera":
            a = {"eye": [_r(rng, 0.3, 0.7), _r(rng, 0.3, 0.7), _r(rng, 2.0, 2.6)]}
        elif kind == "clone":
            a = {}
        elif kind == "render":
            a = {"n": int(rng.integers(1, 4))}
        elif kind == "features":
            a = {"denoise": bool(rng.uniform() < 0.6), "adaptive": bool(rng.uniform() < 0.4)}
        else:
            what = ["n_materials", "bone", "mask", "materials"][int(rng.integers(4))]
            if what == "materials" and mask != "sphere":                     # the sphere as the only emitter is refused only while all of it is hidden
                continue
            a = {"what": what}
        ops.append((kind, a))
    return ops
