"""numpy restatement of temporal reprojection (csrc/reproject.hip): fp64 projection, fp32 film arithmetic.

reproject_ref returns the film rp_reproject_kernel writes and a per-pixel *marginal* mask: a pixel is marginal when one of the kernel's
decisions is within 1e-4 (relative) of flipping, so that an fp64 rounding or an fp32 contraction on the device may legitimately decide it
the other way.  Tests compare the device on the non-marginal pixels and bound the share of marginal ones.

For probe-level checks the MARGIN mask is superseded by tests/reproject_edges_ref.py, which bounds each comparison by the rounding the device
may legitimately commit (about 1e-13 pixel, not 1e-4), follows both branches of a comparison inside its bound and leaves a pixel open only when
they differ; tests/test_reproject_edges.py re-runs this suite's probe cases against it.  The mask stays for the scene-level tests here.
"""
from __future__ import annotations

import math

import numpy as np

MARGIN = 1e-4
F32 = np.float32


def camera_constants(cam, centre=(0.0, 0.0, 0.0)):
    """scene_build.cpp camera_constants(): eye relative to `centre`, unit front, unit right = front x up, `up` as given, h = 2 tan(fovy / 2)."""
    eye = np.asarray(cam.eye, np.float64); lookat = np.asarray(cam.lookat, np.float64); up = np.asarray(cam.up, np.float64)
    front = lookat - eye; front = front * (1.0 / np.linalg.norm(front))
    right = np.cross(front, up); right = right * (1.0 / np.linalg.norm(right))
    return dict(eye=eye - np.asarray(centre, np.float64), front=front, right=right, up=up, h=math.tan(cam.fovy * math.pi / 180.0 * 0.5) * 2.0,
                width=int(cam.width), height=int(cam.height))


def centre_rays(c):
    """(height, width, 3) unit directions of the pixel-centre rays: cast_ray's arithmetic with xi = 0.5, the centre formed in fp64."""
    w, h = c["width"], c["height"]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    u = ((xs + 0.5) / w - 0.5) * c["h"] * w / h
    v = ((ys + 0.5) / h - 0.5) * c["h"]
    d = c["front"] + u[..., None] * c["right"] + v[..., None] * c["up"]
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def basis_inverse(c):
    """Inverse of [front | right | up]; None when singular (|det| below 1e-12 of the product of the column lengths)."""
    m = np.stack([c["front"], c["right"], c["up"]], axis=1)
    det = np.linalg.det(m)
    if not abs(det) >= 1e-12 * np.prod(np.linalg.norm(m, axis=0)) or not abs(det) > 0:
        return None
    f, r, u = c["front"], c["right"], c["up"]
    return np.stack([np.cross(r, u), np.cross(u, f), np.cross(f, r)]) / det


def project(c_old, inv, v):
    """Continuous old pixel coordinates (pixel centres at integer + 0.5) of the points old eye + v, and c0 (<= 0: behind the old eye)."""
    w, h = c_old["width"], c_old["height"]
    c = v @ inv.T
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = ((c[..., 1] / c[..., 0]) / (c_old["h"] * w / h) + 0.5) * w - 0.5
        sy = ((c[..., 2] / c[..., 0]) / c_old["h"] + 0.5) * h - 0.5
    return sx, sy, c[..., 0]


def _near(a, b, scale):
    return np.abs(a - b) <= MARGIN * scale


def reproject_ref(old_cam, new_cam, old_film, old_feat, new_feat, max_history=32.0, depth_tolerance=0.05, normal_threshold=0.9, centre=(0.0, 0.0, 0.0)):
    """(film (h, w, 4) float32, marginal (h, w) bool).  old_film: (h, w, 4) {sum rgb, count}; *_feat: (h, w, 8) features."""
    co, cn = camera_constants(old_cam, centre), camera_constants(new_cam, centre)
    w, h = cn["width"], cn["height"]
    old_film = np.asarray(old_film, F32).reshape(h, w, 4); old_feat = np.asarray(old_feat, F32).reshape(h, w, 8); new_feat = np.asarray(new_feat, F32).reshape(h, w, 8)
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
        n_p = n * (F32(1) / np.sqrt(nn))[..., None]
        # 2. the surface point, from the old eye
        v = (cn["eye"] - co["eye"]) + z.astype(np.float64)[..., None] * centre_rays(cn)
        # 3. into the old view
        sx, sy, c0 = project(co, inv, v)
        r64 = np.linalg.norm(v, axis=-1)
        marginal |= alive & (np.abs(c0) <= MARGIN * r64)
        alive &= c0 > 0
        inside = (sx > -1.0) & (sx < w) & (sy > -1.0) & (sy < h)
        marginal |= alive & (np.abs(sx - np.rint(sx)) <= MARGIN) | alive & (np.abs(sy - np.rint(sy)) <= MARGIN)
        alive &= inside
        sx = np.where(alive, sx, 0.0); sy = np.where(alive, sy, 0.0)
        # 4. bilinear gather
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
        # 5. the result
        avg = (sc / sw).astype(F32)
        marginal |= alive & (np.abs(avg - np.floor(avg) - 0.5) <= MARGIN * np.maximum(avg, 1.0))
        nh = np.minimum(np.rint(avg), max_history).astype(F32)
        alive &= nh >= 1
        rgb = (srgb / sw[..., None] * nh[..., None]).astype(F32)
    out[..., :3] = np.where(alive[..., None], rgb, F32(0)); out[..., 3] = np.where(alive, nh, F32(0))
    return out, marginal
