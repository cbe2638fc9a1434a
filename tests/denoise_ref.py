"""numpy restatement of the denoised-preview filter (csrc/denoise.hip dn_prep_kernel / dn_atrous_kernel).

film: (h, w, 4) records {sum r, g, b, count}; feat: (h, w, 8) {albedo rgb, coverage f, normal xyz, depth z} as mcpt_read_features
returns them; theta = 2 tan(fovy / 2) / height.  Returns the (h, w, 4) film {r, g, b, 1} the device writes ({0, 0, 0, 0} where count = 0).
"""
from __future__ import annotations

import math

import numpy as np

LUM = np.array([0.212671, 0.715160, 0.072169])
K5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
DEFAULTS = dict(iterations=5, sigma_color=4.0, sigma_normal=128.0, sigma_depth=4.0)


def pixel_angle(camera) -> float:
    """theta of the filter's depth term: the angle one pixel subtends, 2 tan(fovy / 2) / height."""
    return 2.0 * math.tan(math.radians(camera.fovy) * 0.5) / camera.height


def _shift(a: np.ndarray, dy: int, dx: int):
    """(a[y + dy, x + dx], inside) for every (y, x); zeros where the tap leaves the image."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((h, w), bool)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        ok[y0:y1, x0:x1] = True
    return out, ok


def denoise_ref(film, feat, theta, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0):
    film = np.asarray(film, np.float64); feat = np.asarray(feat, np.float64)
    L = iterations or DEFAULTS["iterations"]
    sc = sigma_color or DEFAULTS["sigma_color"]; sn = sigma_normal or DEFAULTS["sigma_normal"]; sz = sigma_depth or DEFAULTS["sigma_depth"]
    cnt = film[..., 3]
    a = feat[..., :3]
    valid = (cnt > 0) & (feat[..., 3] >= 0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(cnt[..., None] > 0, film[..., :3] / np.where(cnt > 0, cnt, 1)[..., None], 0.0)
        irr = np.where(a > 1e-3, c / np.where(a > 1e-3, a, 1.0), c)
    irr = np.where(valid[..., None], irr, 0.0)
    nrm = feat[..., 4:7]
    nl = np.sqrt((nrm * nrm).sum(-1, keepdims=True))
    nhat = np.where(nl > 0, nrm / np.where(nl > 0, nl, 1.0), 0.0)
    z = feat[..., 7]

    # 3x3 variance of the luminance over valid neighbours
    lum = irr @ LUM
    s1 = np.zeros_like(lum); s2 = np.zeros_like(lum); n = np.zeros_like(lum)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            lq, ok = _shift(lum, dy, dx); vq, _ = _shift(valid, dy, dx)
            m = ok & vq
            s1 += np.where(m, lq, 0); s2 += np.where(m, lq * lq, 0); n += m
    n = np.maximum(n, 1)
    var = np.where(valid, np.maximum(s2 / n - (s1 / n) ** 2, 0.0), 0.0)

    for i in range(L):
        h = 1 << i
        lum = irr @ LUM
        gv = np.zeros_like(lum); gw = np.zeros_like(lum)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, ok = _shift(var, dy, dx); mq, _ = _shift(valid, dy, dx)
                k = (2 - dx * dx) * (2 - dy * dy) * (ok & mq)
                gv += k * vq; gw += k
        sigma = sc * np.sqrt(gv / np.maximum(gw, 1)) + 1e-4
        sw = np.zeros_like(lum); si = np.zeros_like(irr); sv = np.zeros_like(lum)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                iq, ok = _shift(irr, h * dy, h * dx); mq, _ = _shift(valid, h * dy, h * dx)
                vq, _ = _shift(var, h * dy, h * dx); nq, _ = _shift(nhat, h * dy, h * dx); zq, _ = _shift(z, h * dy, h * dx)
                m = ok & mq & valid
                w = np.full_like(lum, K5[dx + 2] * K5[dy + 2])
                if dx or dy:
                    dist = math.sqrt(dx * dx + dy * dy)
                    nd = np.maximum((nhat * nq).sum(-1), 0.0)
                    w = w * np.exp(-np.abs(lum - iq @ LUM) / sigma) * nd ** sn \
                        * np.exp(-np.abs(z - zq) / (sz * h * dist * theta * z + 1e-4))
                w = np.where(m, w, 0.0)
                sw += w; si += w[..., None] * iq; sv += w * w * vq
        sw = np.where(valid, sw, 1.0)
        irr = np.where(valid[..., None], si / sw[..., None], 0.0)
        var = np.where(valid, sv / (sw * sw), 0.0)

    out = np.zeros(film.shape, np.float64)
    rem = np.where(a > 1e-3, irr * a, irr)
    out[..., :3] = np.where(valid[..., None], rem, c)
    out[..., 3] = np.where(cnt > 0, 1.0, 0.0)
    return out
