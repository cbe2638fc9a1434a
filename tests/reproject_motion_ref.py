"""numpy restatement of motion-vector reprojection (csrc/reproject.hip rp_reproject_motion_kernel): fp64 geometry and projection,
fp32 film arithmetic, plus the small fp64 ray caster the tests build their synthetic worlds with.

reproject_motion_ref returns the film the kernel writes and a per-pixel *marginal* mask with §13's criteria (tests/reproject_ref.py: a decision
within 1e-4 relative of flipping) and one more of the same kind: the sign of n . vec that turns the old shading normal towards the old eye.
"""
from __future__ import annotations

import numpy as np

from tests.reproject_ref import MARGIN, F32, basis_inverse, camera_constants, centre_rays, project, _near


def emissive_faces(scene):
    """Per face: its material is an emitter by the feature kernel's rule (MAT_EMIT_0: |radiance| > 1e-4)."""
    rad = np.array([np.linalg.norm(np.asarray(m.radiance, np.float64)) for m in scene.materials])
    return rad[scene.face[:, 0, 3]] > 1e-4


def ray_cast(vertex, face, origin, dirs):
    """Closest hit of the rays origin + t dirs ((h, w, 3) unit directions) with the triangles, fp64 Moeller-Trumbore, brute force:
    ((h, w) face or -1, (h, w, 2) float32 {u, v}, (h, w) float64 t)."""
    p = np.asarray(vertex, np.float64)[face[:, :, 0]]
    best_t = np.full(dirs.shape[:2], np.inf); best_f = np.full(dirs.shape[:2], -1, np.int32); best_uv = np.zeros(dirs.shape[:2] + (2,), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for f in range(face.shape[0]):
            e1, e2 = p[f, 1] - p[f, 0], p[f, 2] - p[f, 0]
            h = np.cross(dirs, e2); a = h @ e1
            s = origin - p[f, 0]
            u = (h @ s) / a
            q = np.cross(s, e1)
            v = (dirs @ q) / a
            t = (e2 @ q) / a
            ok = (np.abs(a) >= 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 1e-4) & (t < best_t)
            best_t = np.where(ok, t, best_t); best_f = np.where(ok, f, best_f)
            best_uv = np.where(ok[..., None], np.stack([np.broadcast_to(u, ok.shape), v], -1), best_uv)
    return best_f, best_uv.astype(F32), np.where(best_f >= 0, best_t, 0.0)


def shading_normals(normal, face, hit_face, hit_uv, toward):
    """(h, w, 3) fp64 unit shading normals of the hits (load_hit_shade's corner convention), turned against `toward` ((h, w, 3): from the eye to the
    point); zero for a miss."""
    n = np.asarray(normal, np.float64)[face[:, :, 1]][np.maximum(hit_face, 0)]              # (h, w, 3 corners, 3)
    u, v = hit_uv[..., 0].astype(np.float64), hit_uv[..., 1].astype(np.float64)
    s = (1.0 - u - v)[..., None] * n[..., 0, :] + u[..., None] * n[..., 1, :] + v[..., None] * n[..., 2, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = s / np.linalg.norm(s, axis=-1, keepdims=True)
    s = np.where((np.sum(s * toward, -1) > 0)[..., None], -s, s)
    return np.where((hit_face >= 0)[..., None], s, 0.0)


def view_features(cam, vertex, normal, face, emissive, centre=(0.0, 0.0, 0.0)):
    """What a one-sample-at-the-centre feature render of the view would hold, and the hits it came from: ((h, w, 8) float32 features, face, uv, t).
    Non-emissive hits: albedo 0.5, coverage 1, the camera-facing shading normal, depth t; everything else: zeros."""
    c = camera_constants(cam, centre)
    d = centre_rays(c)
    eye = c["eye"] + np.asarray(centre, np.float64)
    hf, uv, t = ray_cast(vertex, face, eye, d)
    surf = (hf >= 0) & ~emissive[np.maximum(hf, 0)]
    feat = np.zeros(d.shape[:2] + (8,), F32)
    feat[..., :3] = np.where(surf[..., None], 0.5, 0.0); feat[..., 3] = surf
    feat[..., 4:7] = np.where(surf[..., None], shading_normals(normal, face, hf, uv, d), 0.0); feat[..., 7] = np.where(surf, t, 0.0)
    return feat, hf, uv, t


def reproject_motion_ref(old_cam, new_cam, old_film, old_feat, new_feat, hit_face, hit_uv, face, emissive, old_vertex, old_normal, max_history=32.0,
                         depth_tolerance=0.05, normal_threshold=0.9, centre=(0.0, 0.0, 0.0), whole_pixel_margin=MARGIN):
    """(film (h, w, 4) float32, marginal (h, w) bool).  hit_face / hit_uv: per pixel of the NEW view the first hit's face (-1 = miss) and float32
    {u, v}; face: (n_face, 3, 4) Model::face; emissive: (n_face,) bool; old_vertex / old_normal: the scene before the update (world coordinates).
    whole_pixel_margin: how close to an integer sx or sy must come to make the pixel marginal -- §13's 1e-4 by default.  What that criterion
    guards is the floor: device and restatement form sx from the same fp32 u, v by about 30 fp64 operations on values up to the width, so at
    64 pixels they agree to 30 x 64 x 2^-53 = 2e-13 pixel; only a point within that of a whole pixel can take its taps from the neighbouring
    cell, and the cell it loses then weighs 2e-13.  A scene at rest under a fixed camera lands EVERY point next to a whole pixel (within
    2^-23 x the triangle's extent, and far closer on axis-aligned walls); a test of such a scene passes 1e-11 here, fifty times the agreement."""
    co, cn = camera_constants(old_cam, centre), camera_constants(new_cam, centre)
    w, h = cn["width"], cn["height"]
    old_film = np.asarray(old_film, F32).reshape(h, w, 4); old_feat = np.asarray(old_feat, F32).reshape(h, w, 8); new_feat = np.asarray(new_feat, F32).reshape(h, w, 8)
    hit_face = np.asarray(hit_face, np.int64).reshape(h, w); hit_uv = np.asarray(hit_uv, F32).reshape(h, w, 2)
    out = np.zeros((h, w, 4), F32); marginal = np.zeros((h, w), bool)
    inv = basis_inverse(co)
    if inv is None:
        return out, marginal
    max_history, depth_tolerance, normal_threshold = F32(max_history), F32(depth_tolerance), F32(normal_threshold)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # 1. the new pixel's features
        f = new_feat[..., 3]; n = new_feat[..., 4:7]; z = new_feat[..., 7]
        nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2]).astype(F32)
        alive = (f >= F32(0.5)) & (z > 0) & (nn > 0)
        marginal |= _near(f, F32(0.5), 0.5)
        # 2. the first hit: a miss and an emitter carry no history
        hf = np.maximum(hit_face, 0)
        alive &= (hit_face >= 0) & (hit_face < face.shape[0]) & ~np.asarray(emissive, bool)[np.minimum(hf, face.shape[0] - 1)]
        hf = np.where(alive, hf, 0)
        # 3. where the surface point was, from the old eye
        u, v = hit_uv[..., 0].astype(np.float64), hit_uv[..., 1].astype(np.float64)
        bw = 1.0 - u - v
        V = np.asarray(old_vertex, np.float64)[face[:, :, 0]][hf]; N = np.asarray(old_normal, np.float64)[face[:, :, 1]][hf]
        p_old = bw[..., None] * V[..., 0, :] + u[..., None] * V[..., 1, :] + v[..., None] * V[..., 2, :]
        vec = (p_old - np.asarray(centre, np.float64)) - co["eye"]
        # 4. the old shading normal, towards the old eye
        ns = bw[..., None] * N[..., 0, :] + u[..., None] * N[..., 1, :] + v[..., None] * N[..., 2, :]
        nl = np.sum(ns * ns, -1)
        alive &= nl > 0
        r64 = np.linalg.norm(vec, axis=-1)
        facing = np.sum(ns * vec, -1)
        marginal |= alive & (np.abs(facing) <= MARGIN * np.sqrt(nl) * r64)
        n_p = (ns / np.sqrt(nl)[..., None] * np.where(facing > 0, -1.0, 1.0)[..., None]).astype(F32)
        # 5. §13 steps 3 - 6 with r = |vec|
        sx, sy, c0 = project(co, inv, vec)
        marginal |= alive & (np.abs(c0) <= MARGIN * r64)
        alive &= c0 > 0
        inside = (sx > -1.0) & (sx < w) & (sy > -1.0) & (sy < h)
        marginal |= alive & (np.abs(sx - np.rint(sx)) <= whole_pixel_margin) | alive & (np.abs(sy - np.rint(sy)) <= whole_pixel_margin)
        alive &= inside
        sx = np.where(alive, sx, 0.0); sy = np.where(alive, sy, 0.0)
        r = r64.astype(F32)
        flx, fly = np.floor(sx), np.floor(sy)
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        fx, fy = (sx - flx).astype(F32), (sy - fly).astype(F32)
        ztol = (depth_tolerance * r).astype(F32)
        sw = np.zeros((h, w), F32); sc = np.zeros((h, w), F32); srgb = np.zeros((h, w, 3), F32)
        for t in range(4):
            qx, qy = x0 + (t & 1), y0 + (t >> 1)
            wq = ((fx if t & 1 else F32(1) - fx) * (fy if t >> 1 else F32(1) - fy)).astype(F32)
            ok = alive & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & (wq > 0)
            cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            qf = old_film[cy, cx]; qa = old_feat[cy, cx]
            cnt = qf[..., 3]
            ok &= cnt > 0
            marginal |= ok & _near(qa[..., 3], F32(0.5), 0.5)
            ok &= qa[..., 3] >= F32(0.5)
            dz = np.abs(qa[..., 7] - r).astype(F32)
            marginal |= ok & _near(dz, ztol, ztol)
            ok &= dz <= ztol
            qn = qa[..., 4:7]
            qq = (qn[..., 0] * qn[..., 0] + qn[..., 1] * qn[..., 1] + qn[..., 2] * qn[..., 2]).astype(F32)
            ok &= qq > 0
            cos = ((qn[..., 0] * n_p[..., 0] + qn[..., 1] * n_p[..., 1] + qn[..., 2] * n_p[..., 2]) * (F32(1) / np.sqrt(qq))).astype(F32)
            marginal |= ok & _near(cos, normal_threshold, normal_threshold)
            ok &= cos >= normal_threshold
            mean = np.where(np.isnan(qf[..., :3]), F32(0), qf[..., :3] / cnt[..., None]).astype(F32)      # NaN components zeroed like the render path
            wz = np.where(ok, wq, F32(0))
            sw += wz; sc += np.where(ok, wq * cnt, F32(0)); srgb += np.where(ok[..., None], wq[..., None] * mean, F32(0))
        marginal |= alive & _near(sw, F32(0.25), 0.25)
        alive &= sw >= F32(0.25)
        avg = (sc / sw).astype(F32)
        marginal |= alive & (np.abs(avg - np.floor(avg) - 0.5) <= MARGIN * np.maximum(avg, 1.0))
        nh = np.minimum(np.rint(avg), max_history).astype(F32)
        alive &= nh >= 1
        rgb = (srgb / sw[..., None] * nh[..., None]).astype(F32)
    out[..., :3] = np.where(alive[..., None], rgb, F32(0)); out[..., 3] = np.where(alive, nh, F32(0))
    return out, marginal
