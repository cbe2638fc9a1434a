"""numpy restatement of the face-visibility rules (include/mcpt.h): what the intersection records and refit boxes of a context hold
after an update under a mask, what a mask means for the light list (csrc/visibility_plan.h), and the sub-scene -- the same scene with the hidden
faces deleted -- that a masked context must be indistinguishable from.  Everything is in Model::face order."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def _down(v):
    """fp64 -> the largest fp32 not above it (refit.hip: rf_down)."""
    f = v.astype(F32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, F32(-np.inf)), f).astype(F32)


def _up(v):
    f = v.astype(F32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, F32(np.inf)), f).astype(F32)


def visible_records(vertex, face, centre):
    """What rf_triangles_kernel writes per face: ((n, 9) fp32 {first corner less the centre, edge 1, edge 2 from the world coordinates},
    (n, 6) fp32 box {lo, hi}: the fp64 bound of the centred corners rounded outward)."""
    w = np.asarray(vertex, np.float64)[np.asarray(face)[:, :, 0]]                # (n, 3 corners, 3)
    v = w - np.asarray(centre, np.float64)
    rec = np.concatenate([v[:, 0].astype(F32), (w[:, 1] - w[:, 0]).astype(F32), (w[:, 2] - w[:, 0]).astype(F32)], axis=1)
    box = np.concatenate([_down(v.min(axis=1)), _up(v.max(axis=1))], axis=1)
    return rec, box


def hide(rec, box, mask):
    """The hide pass on records and boxes of visible faces: a hidden face keeps its first corner, both edges become +0 and its box the point of the
    first corner; a visible face keeps every bit."""
    rec = np.array(rec, F32, copy=True); box = np.array(box, F32, copy=True)
    if mask is None:
        return rec, box
    h = np.asarray(mask).reshape(-1) == 0
    rec[h, 3:] = F32(0.0)
    box[h, :3] = rec[h, :3]; box[h, 3:] = rec[h, :3]
    return rec, box


def plan(mask, face_material, material_emits):
    """csrc/visibility_plan.h: vs_plan.  mask None = every face visible."""
    fm = np.asarray(face_material, np.int64).reshape(-1); em = np.asarray(material_emits).reshape(-1) != 0
    vis = np.ones(fm.shape[0], bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    known = fm < em.shape[0]
    emits = np.zeros(fm.shape[0], bool); emits[known] = em[fm[known]]
    return {"n_hidden": int((~vis).sum()), "n_hidden_emitters": int((~vis & emits).sum()), "n_lights": int((vis & emits).sum()),
            "visible_faces": np.bincount(fm[vis & known], minlength=em.shape[0]).astype(np.uint32)}


def emits(materials):
    """Per material: does it pass the light list's test, the fp64 length of its radiance > 0.01 (scene_build.cpp: device_material)?"""
    return np.array([bool(np.sqrt(np.sum(np.asarray(m.radiance, np.float64) ** 2)) > 0.01) for m in materials])


def sub_scene(pkg, scene, mask):
    """(the scene without its hidden faces -- vertex arrays kept --, new_of_old: the monotone renumbering of the faces, -1 for a hidden one)."""
    vis = np.asarray(mask).reshape(-1) != 0
    new_of_old = np.where(vis, np.cumsum(vis) - 1, -1).astype(np.int32)
    s = pkg.scenes.SceneData(scene.name, scene.vertex, scene.normal, scene.texcoord, np.ascontiguousarray(scene.face[vis]), scene.materials, scene.camera,
                             dict(scene.meta))
    return s, new_of_old
