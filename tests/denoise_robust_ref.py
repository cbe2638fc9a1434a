"""numpy restatement of the denoised-preview filter with its two opt-in flags (csrc/denoise.hip dn_prep_robust_kernel /
dn_atrous_kernel): the emission split and the firefly clamp.  flags = 0 is tests/denoise_ref.py, operation for operation.

film: (h, w, 4) records {sum r, g, b, count}; feat: (h, w, 8) as mcpt_read_features returns them; emis: (h, w, 4) as mcpt_read_emission
returns it (only read with SPLIT; may be None otherwise); theta = 2 tan(fovy / 2) / height.  Returns the (h, w, 4) film {r, g, b, 1} the
device writes ({0, 0, 0, 0} where count = 0).
"""
from __future__ import annotations

import math

import numpy as np

from tests.denoise_ref import DEFAULTS, K5, LUM, _shift, assert_identity_level, decisions, variance3x3

SPLIT = 0x1                    # MCPT_DENOISE_SPLIT_EMISSION
CLAMP = 0x2                    # MCPT_DENOISE_CLAMP_FIREFLIES
DEFAULT_FIREFLY_CLAMP = 4.0    # MCPT_DENOISE_DEFAULT_FIREFLY_CLAMP


def clamp_fireflies(irr, valid, k):
    """irr with every valid pixel whose luminance l exceeds k m scaled by k m / l, m = the largest UNCLAMPED l among the valid pixels of its
    3x3 neighbourhood other than itself; a pixel without such a neighbour is left alone.  Also returns the mask of the clamped pixels."""
    lum = irr @ LUM
    m = np.full(lum.shape, -np.inf); has = np.zeros(lum.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            lq, ok = _shift(lum, dy, dx); vq, _ = _shift(valid, dy, dx)
            nb = ok & vq
            m = np.where(nb, np.maximum(m, lq), m); has |= nb
    hot = valid & has & (lum > k * np.where(has, m, 0.0))
    scale = np.where(hot, k * np.where(has, m, 0.0) / np.where(hot, lum, 1.0), 1.0)
    return irr * scale[..., None], hot


def denoise_robust_ref(film, feat, emis, theta, flags=0, firefly_clamp=0.0, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0):
    sampled, valid, demod, passed = decisions(film, feat)
    film = np.asarray(film, np.float32).astype(np.float64); feat = np.asarray(feat, np.float32).astype(np.float64)
    L = iterations or DEFAULTS["iterations"]
    sc = sigma_color or DEFAULTS["sigma_color"]; sn = sigma_normal or DEFAULTS["sigma_normal"]; sz = sigma_depth or DEFAULTS["sigma_depth"]
    k = firefly_clamp or DEFAULT_FIREFLY_CLAMP
    cnt = film[..., 3]
    a = feat[..., :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(sampled[..., None], film[..., :3] / np.where(sampled, cnt, 1)[..., None], 0.0)
        refl = c
        if flags & SPLIT:
            e = np.asarray(emis, np.float32).astype(np.float64)[..., :3]
            refl = np.maximum(c - e, 0.0)
        irr = np.where(demod, refl / np.where(demod, a, 1.0), refl)
    irr = np.where(valid[..., None], irr, 0.0)
    if flags & CLAMP:
        irr, _ = clamp_fireflies(irr, valid, k)
    nrm = feat[..., 4:7]
    nl = np.sqrt((nrm * nrm).sum(-1, keepdims=True))
    nhat = np.where(nl > 0, nrm / np.where(nl > 0, nl, 1.0), 0.0)
    z = feat[..., 7]

    # 3x3 variance of the (clamped) luminance over valid neighbours
    var = variance3x3(irr @ LUM, valid)

    for i in range(L):
        h = 1 << i
        lum = irr @ LUM
        gv = np.zeros_like(lum); gw = np.zeros_like(lum)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, ok = _shift(var, dy, dx); mq, _ = _shift(valid, dy, dx)
                kk = (2 - dx * dx) * (2 - dy * dy) * (ok & mq)
                gv += kk * vq; gw += kk
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
    if flags & SPLIT:
        rem = rem + e
    out[..., :3] = np.where(valid[..., None], rem, passed)
    out[..., 3] = np.where(sampled, 1.0, 0.0)
    return out
