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


def decisions(film, feat):
    """What the device decides per pixel, decided as it decides it: on the fp32 inputs against the fp32 constants (dn_valid, dn_irr).
    float32(1e-3) is greater than the double 1e-3, so a test of the widened albedo against the double would divide out an albedo of exactly
    float32(1e-3) that the device keeps.  Returns (sampled = count > 0, valid = sampled and coverage >= 0.5, demod = albedo > 1e-3f per
    channel, passed = the fp32 mean float32(sum) / float32(count) of the sampled pixels, 0 elsewhere: what an invalid pixel passes through,
    and the device's division is correctly rounded)."""
    film = np.asarray(film, np.float32); feat = np.asarray(feat, np.float32)
    sampled = film[..., 3] > np.float32(0)
    valid = sampled & (feat[..., 3] >= np.float32(0.5))
    demod = feat[..., :3] > np.float32(1e-3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        passed = np.where(sampled[..., None], film[..., :3] / np.where(sampled, film[..., 3], np.float32(1))[..., None], np.float32(0))
    return sampled, valid, demod, passed.astype(np.float64)


def variance3x3(lum, valid):
    """Variance of `lum` over the valid pixels of every valid pixel's 3x3 neighbourhood, in two passes: their mean, then the mean of the squared
    deviations from it -- exactly 0 on a constant patch.  The device forms E[l^2] - E[l]^2 from single-pass fp32 sums, which cancels: nine equal
    luminances l can leave it sqrt(var) up to ~ 6e-4 l.  Measured through mcpt_probe_denoise on films without noise that costs at most 7e-5 of
    max(1, |out|), so the device is held to the exact variance, not to a restatement of its cancellation."""
    s1 = np.zeros_like(lum); n = np.zeros_like(lum)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            lq, ok = _shift(lum, dy, dx); vq, _ = _shift(valid, dy, dx)
            m = ok & vq
            s1 += np.where(m, lq, 0); n += m
    n = np.maximum(n, 1)
    mean = s1 / n
    s2 = np.zeros_like(lum)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            lq, ok = _shift(lum, dy, dx); vq, _ = _shift(valid, dy, dx)
            s2 += np.where(ok & vq, (lq - mean) ** 2, 0)
    return np.where(valid, s2 / n, 0.0)


def assert_identity_level(h, before, after):
    """From the level whose step h reaches the image's larger side every tap but the centre's leaves the image: the level is the identity on irr
    (up to the rounding of (w x) / w)."""
    if h >= max(before.shape[:2]):
        assert np.allclose(after, before, rtol=1e-14, atol=0.0), h


def denoise_ref(film, feat, theta, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0):
    sampled, valid, demod, passed = decisions(film, feat)
    film = np.asarray(film, np.float32).astype(np.float64); feat = np.asarray(feat, np.float32).astype(np.float64)
    L = iterations or DEFAULTS["iterations"]
    sc = sigma_color or DEFAULTS["sigma_color"]; sn = sigma_normal or DEFAULTS["sigma_normal"]; sz = sigma_depth or DEFAULTS["sigma_depth"]
    cnt = film[..., 3]
    a = feat[..., :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(sampled[..., None], film[..., :3] / np.where(sampled, cnt, 1)[..., None], 0.0)
        irr = np.where(demod, c / np.where(demod, a, 1.0), c)
    irr = np.where(valid[..., None], irr, 0.0)
    nrm = feat[..., 4:7]
    nl = np.sqrt((nrm * nrm).sum(-1, keepdims=True))
    nhat = np.where(nl > 0, nrm / np.where(nl > 0, nl, 1.0), 0.0)
    z = feat[..., 7]

    # 3x3 variance of the luminance over valid neighbours
    var = variance3x3(irr @ LUM, valid)

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
        before = irr
        irr = np.where(valid[..., None], si / sw[..., None], 0.0)
        assert_identity_level(h, before, irr)
        var = np.where(valid, sv / (sw * sw), 0.0)

    out = np.zeros(film.shape, np.float64)
    rem = np.where(demod, irr * a, irr)
    out[..., :3] = np.where(valid[..., None], rem, passed)
    out[..., 3] = np.where(sampled, 1.0, 0.0)
    return out
