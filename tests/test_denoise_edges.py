"""The denoiser's filter on caller films at every decision edge (csrc/denoise.hip), through mcpt_probe_denoise.

Every case is a film, features and (with the split) an emission buffer built by hand so that one decision of the filter is met on its boundary
and on both sides of it: validity (count, coverage), the albedo threshold of the demodulation, zero / opposed / perpendicular normals, depth 0,
the luminance term on films without noise, stencils wider than the image, the firefly clamp at l = k m, the emission split at mean = E.  Ties are
exact in fp32: values are dyadic, factors are powers of two, and luminance ties come from scaling all three channels of a pixel by a power of two,
which commutes with dn_lum's rounding.  Near misses of computed quantities are 2^-10 away (asserted >= 2^-12 on the restatement); near misses of
inputs (coverage, albedo, count) are one ulp away.

CPU tests pin what is new in the restatements (tests/denoise_ref.py, tests/denoise_robust_ref.py: decisions in fp32, the variance in two passes,
identity levels) and run the restatement on every case, with the case's own expectation.  GPU tests hold the device to the restatement on every
pixel of every case, nothing forgiven: decisions exact, values within 1e-3 max(1, |ref|).
"""
from __future__ import annotations

import collections
import ctypes as C
import functools

import numpy as np
import pytest

from tests import kit
from tests.denoise_ref import LUM, decisions, denoise_ref, pixel_angle, variance3x3
from tests.denoise_robust_ref import CLAMP, SPLIT, clamp_fireflies, denoise_robust_ref

F32 = np.float32
A0 = F32(1e-3)                                                             # the demodulation threshold as the device holds it
TINY = np.nextafter(F32(0), F32(1))                                        # the smallest count there is
NEAR = 2.0 ** -10                                                          # how far "just off" a computed tie is
BOUND = 1e-3                                                               # |out - ref| <= BOUND max(1, |ref|), every pixel
SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (64, 4), (65, 5), (130, 9)]      # (w, h); blocks are 64 x 4


def up32(x):
    return np.nextafter(F32(x), F32(np.inf))


def down32(x):
    return np.nextafter(F32(x), F32(-np.inf))


# ------------------------------------------------------------------------------------------------------------------------ inputs
def _flat(w, h, irr=1.0, albedo=0.5, cnt=4.0, z=2.0):
    """A plane facing the camera: irradiance `irr` everywhere, full coverage, normal +z, depth z.  With the defaults every number is dyadic."""
    feat = np.zeros((h, w, 8), F32)
    feat[..., :3] = albedo; feat[..., 3] = 1.0; feat[..., 6] = 1.0; feat[..., 7] = z
    film = np.zeros((h, w, 4), F32)
    film[..., 3] = cnt
    _set_irr(film, feat, np.s_[:, :], irr)
    return film, feat


def _set_irr(film, feat, where, irr):
    """The sums of the pixels `where` such that their demodulated irradiance is `irr` (by the device's rule: channels of albedo <= 1e-3f keep the mean)."""
    a = feat[where][..., :3]
    film[where + (slice(0, 3),)] = (np.asarray(irr, F32) * np.where(a > A0, a, F32(1))) * film[where][..., 3:4]


def _varied(w, h, seed, tilt=0.15):
    """A film with something to filter everywhere: irradiance in [0.5, 1.5] per channel, albedo in [0.2, 0.9], counts 1 .. 8, normals tilted off
    +z by up to `tilt`, depth in [1.8, 2.2]."""
    rng = np.random.default_rng(seed)
    film, feat = _flat(w, h)
    feat[..., :3] = rng.uniform(0.2, 0.9, (h, w, 3))
    n = np.concatenate([rng.uniform(-tilt, tilt, (h, w, 2)), np.ones((h, w, 1))], -1)
    feat[..., 4:7] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    feat[..., 7] = rng.uniform(1.8, 2.2, (h, w))
    film[..., 3] = rng.integers(1, 9, (h, w))
    _set_irr(film, feat, np.s_[:, :], rng.uniform(0.5, 1.5, (h, w, 3)))
    return film, feat


def _mean(film):
    with np.errstate(divide="ignore", invalid="ignore"):
        return film[..., :3].astype(np.float64) / film[..., 3:].astype(np.float64)


class Case:
    """One probe input.  pins: the code of denoise.hip the case is about.  expect(out): what the case is built to show, asserted on the restatement
    (CPU) and on the device's output (GPU), beside the full comparison.  hot: the pixels (y, x) the firefly clamp must clamp, with CLAMP."""

    def __init__(self, size, pins, film, feat, emis=None, expect=None, hot=None, **opts):
        self.size, self.pins, self.film, self.feat, self.emis, self.expect, self.hot, self.opts = size, pins, film, feat, emis, expect, hot, opts
        assert size in SHAPES and film.shape == (size[1], size[0], 4) and feat.shape == (size[1], size[0], 8)
        assert film.dtype == F32 and feat.dtype == F32 and (emis is None or emis.dtype == F32)
        assert bool(opts.get("split_emission")) == (emis is not None)

    @property
    def flags(self):
        return (SPLIT if self.opts.get("split_emission") else 0) | (CLAMP if self.opts.get("clamp_fireflies") else 0)

    def ref(self, theta):
        kw = {k: v for k, v in self.opts.items() if k not in ("split_emission", "clamp_fireflies", "firefly_clamp")}
        if not self.flags:
            return denoise_ref(self.film, self.feat, theta, **kw)
        return denoise_robust_ref(self.film, self.feat, self.emis, theta, flags=self.flags, firefly_clamp=self.opts.get("firefly_clamp", 0.0), **kw)


def _keeps(pixels, film, rel=1e-5):
    """expect: the pixels (y, x) come out as their own mean."""
    want = _mean(film)

    def check(out):
        for q in pixels:
            assert np.all(np.abs(out[q][:3] - want[q]) <= rel * np.maximum(1.0, np.abs(want[q]))), (q, out[q], want[q])
    return check


def _all_zero(out):
    assert np.all(out[..., :3] == 0)


def _all_pixels(w, h):
    return [(y, x) for y in range(h) for x in range(w)]


@functools.lru_cache(maxsize=None)
def cases():
    S = collections.OrderedDict()

    # ---------------------------------------------------------------------------------------------------- validity
    pins = "dn_valid: film.w > 0.f && fa.w >= 0.5f; dn_atrous_kernel<LAST>: gp.w < 0.f -> fm.w > 0.f ? mean : {0, 0, 0, 0}"
    film, feat = _varied(5, 7, 1)
    feat[1, 1, 3] = 0.5; feat[3, 1, 3] = down32(0.5); feat[5, 1, 3] = up32(0.5); feat[3, 3, 3] = 0.0
    S["coverage-edges"] = Case((5, 7), pins, film, feat)
    film, feat = _flat(5, 7)
    film[1, 1] = (3.0, 5.0, 7.0, 0.0)                                        # sums without a count: nothing to show
    film[3, 1] = (1 * TINY, 2 * TINY, 3 * TINY, TINY); feat[3, 1, 3] = down32(0.5)          # the smallest count, passed through: mean (1, 2, 3)
    film[5, 3] = (1 * TINY, 1 * TINY, 1 * TINY, TINY)                        # ... and valid: irradiance 2 among irradiance 1
    film[0, 4] = 0.0; feat[0, 4, 3] = 0.25                                   # no count and no coverage
    S["count-edges"] = Case((5, 7), pins, film, feat)
    film, feat = _varied(65, 5, 2)
    ys, xs = np.mgrid[0:5, 0:65]
    feat[(xs + ys) % 2 == 1, 3] = 0.25
    S["checkerboard"] = Case((65, 5), pins + "; every tap loop: if (gq.w < 0.f) continue", film, feat)
    film, feat = _varied(5, 7, 3)
    feat[..., 3] = 0.25; feat[3, 2, 3] = 1.0
    S["lone-valid"] = Case((5, 7), "dn_prep_kernel: cnt = 1, var = 0; dn_atrous_kernel: sw = the centre tap's 9 / 64 alone", film, feat, expect=_keeps([(3, 2)], film))
    film, feat = _varied(65, 5, 4)
    feat[..., 3] = 0.25; film[2, 10:20] = 0.0; film[4, 64] = 0.0
    S["all-invalid"] = Case((65, 5), pins, film, feat)
    film, feat = _varied(130, 9, 5)
    for k, q in enumerate([(0, 0), (0, 129), (8, 0), (8, 129), (1, 63), (6, 64), (3, 20), (4, 100), (3, 63), (4, 64)]):
        if k % 2:
            film[q] = 0.0
        else:
            feat[q][3] = down32(0.5)
    S["invalid-at-corners-and-seams"] = Case((130, 9), pins + "; x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y", film, feat)

    # ---------------------------------------------------------------------------------------------------- albedo threshold
    pins = "dn_irr: fa.x > 1e-3f ? c.x / fa.x : c.x; dn_atrous_kernel<LAST>: fa.x > 1e-3f ? r.x * fa.x : r.x"
    film, feat = _flat(5, 7)
    choice = np.array([A0, up32(A0), 0.0, 0.5, down32(A0)], F32)
    ys, xs = np.mgrid[0:7, 0:5]
    for c in range(3):
        feat[..., c] = choice[(xs + 2 * ys + c) % 5]
    _set_irr(film, feat, np.s_[:, :], 1.0)                                   # flat by the device's rule: a wrong decision is a factor of 1000
    S["albedo-threshold"] = Case((5, 7), pins, film, feat, expect=_keeps(_all_pixels(5, 7), film))
    film, feat = _flat(65, 5)
    feat[..., :3] = np.random.default_rng(6).uniform(0.05, 0.95, (5, 65, 3))
    _set_irr(film, feat, np.s_[:, :], 0.75)
    S["textured-flat"] = Case((65, 5), pins, film, feat, expect=_keeps(_all_pixels(65, 5), film))

    # ---------------------------------------------------------------------------------------------------- normals
    pins = "dn_prep_kernel: inv = nn > 0.f ? 1.f / sqrtf(nn) : 0.f; dn_atrous_kernel: nd = fmaxf(dot, 0.f), pow_pos(nd, p.sigma_n)"
    film, feat = _varied(5, 7, 7)
    feat[3, 2, 4:7] = 0.0                                                    # at the centre: only its own tap survives; as a neighbour: weight 0
    S["normal-zero"] = Case((5, 7), pins, film, feat, expect=_keeps([(3, 2)], film))
    film, feat = _flat(5, 7)
    for x, n in enumerate([(0, 0, 1), (0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 1, 0)]):
        feat[:, x, 4:7] = n
        _set_irr(film, feat, np.s_[:, x:x + 1], 0.25 * 2 ** x)
    S["normal-opposed-perpendicular"] = Case((5, 7), pins, film, feat, sigma_color=1e6, expect=_keeps([(y, x) for y in range(7) for x in (2, 3, 4)], film))
    film, feat = _varied(5, 7, 8, tilt=0.6)
    for name, s in (("1", 1.0), ("0.3", 0.3), ("7", 7.0)):
        f = feat.copy(); f[..., 4:7] *= F32(s)
        S["normals-x" + name] = Case((5, 7), pins, film, f)
    for sn in (1.0, 128.0):
        S["sigma-normal-%g" % sn] = Case((5, 7), pins, film, feat, sigma_normal=sn)

    # ---------------------------------------------------------------------------------------------------- depth
    pins = "dn_atrous_kernel: zs = p.sigma_z * h * p.theta * gp.w; ez = fabsf(gp.w - gq.w) / (zs * dist + 1e-4f)"
    film, feat = _varied(5, 7, 9)
    feat[..., 7] = 2.0; feat[3, 2, 7] = 0.0                                  # zs = 0: the others are 2 / 1e-4 away
    S["depth-zero-centre"] = Case((5, 7), pins, film, feat, expect=_keeps([(3, 2)], film))
    film, feat = _flat(65, 5)
    feat[:, 32:, 7] = 200.0
    _set_irr(film, feat, np.s_[:, 32:], 0.25)
    S["depth-step-100x"] = Case((65, 5), pins, film, feat, sigma_color=1e6,
                                 expect=_keeps([(y, x) for y in range(5) for x in range(32)], film, rel=1e-3))     # (exp(-198 / (zs dist)) leaks ~ 1e-4 at h = 16)
    film, feat = _varied(65, 5, 10)
    S["sigma-depth-tiny"] = Case((65, 5), pins, film, feat, sigma_depth=1e-6)
    S["sigma-depth-huge"] = Case((65, 5), pins, film, feat, sigma_depth=1e9)

    # ---------------------------------------------------------------------------------------------------- luminance term and variance
    pins = "dn_prep_kernel: the 3x3 variance of the luminance; dn_atrous_kernel: sigma = p.sigma_c * sqrtf(gv / gw) + 1e-4f, el = fabsf(lp - lq) * inv_sigma"
    for step in (1e-3, 1e-2, 0.5):
        for sc in (4.0, 1e-3):
            film, feat = _flat(65, 5, irr=1.3, albedo=1.0)                   # (1.3: a luminance whose square is not exact in fp32)
            _set_irr(film, feat, np.s_[:, 32:], 1.3 + step)
            S["step-%g-sigma-color-%g" % (step, sc)] = Case((65, 5), pins, film, feat, sigma_color=sc)
    film, feat = _flat(65, 5, irr=20.8, albedo=1.0)                          # where single-pass sums hurt most: the step the cancelled sigma just lets through
    _set_irr(film, feat, np.s_[:, 32:], 20.8 * (1 + 2.6e-3))
    S["step-at-the-cancellation-sigma"] = Case((65, 5), pins, film, feat)
    for level in (0.1, 1.0, 10.0):
        film, feat = _flat(65, 5, albedo=1.0)
        _set_irr(film, feat, np.s_[:, :], (level * (1 + 1e-3 * np.arange(65)))[None, :, None] * np.ones((5, 1, 3)))
        S["ramp-%g" % level] = Case((65, 5), pins, film, feat)
    film, feat = _flat(65, 5, irr=1.3, albedo=1.0)
    _set_irr(film, feat, np.s_[2:3, 40:41], 1.95)
    S["one-pixel-off"] = Case((65, 5), pins, film, feat)

    # ---------------------------------------------------------------------------------------------------- stencil against borders and levels
    pins = "dn_atrous_kernel: qx = x + h * dx, if (qx < 0 || qx >= p.width) continue; launch_dn_filter: h = 1 << lv, the ping-pong of iv0 / iv1"
    for (w, h), its in (((5, 7), (1, 5, 10)), ((65, 5), (1, 5, 10)), ((130, 9), (10,)), ((1, 1), (5,)), ((1, 9), (5,)), ((9, 1), (5,)), ((64, 4), (5,))):
        film, feat = _varied(w, h, 11 + w)
        for it in its:
            S["levels-%d-%dx%d" % (it, w, h)] = Case((w, h), pins, film, feat, iterations=it)

    # ---------------------------------------------------------------------------------------------------- firefly clamp
    pins = "dn_prep_robust_kernel<CLAMP>: if (m != -INFINITY && l > p.clamp_k * m) lc = p.clamp_k * m; sc = lc / lr"
    for k in (2.0, 4.0):
        kw = dict(clamp_fireflies=True, firefly_clamp=k)
        film, feat = _flat(5, 7, irr=0.5)
        _set_irr(film, feat, np.s_[3:4, 2:3], 0.5 * k)                       # l == k m exactly
        S["firefly-tie-k%g" % k] = Case((5, 7), pins, film, feat, hot=[], **kw)
        film, feat = _flat(5, 7, irr=0.5)
        _set_irr(film, feat, np.s_[3:4, 2:3], 0.5 * k * (1 + NEAR))
        S["firefly-above-k%g" % k] = Case((5, 7), pins, film, feat, hot=[(3, 2)], **kw)
        film, feat = _flat(5, 7, irr=0.5)
        feat[2:5, 1:4, 3] = 0.25; feat[3, 2, 3] = 1.0
        _set_irr(film, feat, np.s_[3:4, 2:3], 512.0)                         # an island: no valid neighbour, never clamped
        S["firefly-island-k%g" % k] = Case((5, 7), pins + "; l = -INFINITY marks an invalid or outside pixel", film, feat, hot=[], expect=_keeps([(3, 2)], film), **kw)
        film, feat = _flat(1, 1, irr=512.0)
        S["firefly-1x1-k%g" % k] = Case((1, 1), pins, film, feat, hot=[], expect=_keeps([(0, 0)], film), **kw)
        film, feat = _flat(5, 7, irr=0.0)
        _set_irr(film, feat, np.s_[3:4, 2:3], 8.0)                           # m == 0 with l > 0: clamped to 0; everywhere else l == m == 0
        S["firefly-m-zero-k%g" % k] = Case((5, 7), pins, film, feat, hot=[(3, 2)], expect=_all_zero, **kw)
        film, feat = _flat(5, 7, irr=0.5)
        _set_irr(film, feat, np.s_[3:4, 2:4], 64.0)                          # two of them side by side: m is the RAW maximum, each shields the other
        S["firefly-pair-k%g" % k] = Case((5, 7), pins, film, feat, hot=[], **kw)
        # against the 68 x 8 raw and 66 x 6 clamped LDS tiles of block (0, 0): a firefly whose brightest neighbour (2, against 0.5 around) lies in the
        # other block, and one in the clamped tile's halo whose brightest neighbour lies in the raw tile's outer ring
        for (fy, fx), (by, bx) in (((0, 0), (1, 1)), ((3, 63), (4, 64)), ((4, 64), (5, 65)), ((8, 129), (7, 128))):
            film, feat = _flat(130, 9, irr=0.5)
            _set_irr(film, feat, np.s_[by:by + 1, bx:bx + 1], 2.0)
            _set_irr(film, feat, np.s_[fy:fy + 1, fx:fx + 1], 64.0)
            S["firefly-at-%d-%d-k%g" % (fx, fy, k)] = Case((130, 9), pins + "; s_raw, s_cl", film, feat, hot=[(fy, fx)], **kw)

    # ---------------------------------------------------------------------------------------------------- emission split
    pins = "dn_irr_split<SPLIT>: fmaxf(c.x - e.x, 0.f); dn_atrous_kernel<LAST, SPLIT>: o.x += e.x"
    for name, extra in (("", {}), ("-clamp", dict(clamp_fireflies=True, firefly_clamp=2.0))):
        film, feat = _flat(5, 7)                                             # mean 0.5 everywhere
        emis = np.zeros((7, 5, 4), F32)
        emis[1, 1, :3] = 0.5                                                 # mean == E: the reflected part is 0, the pixel comes out as E
        emis[3, 3, :3] = (0.75, 0.5, 0.625)                                  # mean < E (and ==): clamped at 0, E added back in full
        emis[5, 2, :3] = 0.25                                                # half of the pixel is emitted
        emis[..., 3] = np.where(emis[..., 0] > 0, 0.25, 0.0)

        def expect(out, emis=emis):                                           # the reflected part starts at 0 in every channel and takes up the same
            for q in ((1, 1), (3, 3)):                                       # grey from its neighbours: what is left after E is one number, >= 0
                rest = out[q][:3] - emis[q][:3]
                assert rest.min() >= 0 and np.ptp(rest) <= 1e-6, (q, out[q])
        S["split-mean-and-E" + name] = Case((5, 7), pins, film, feat, emis=emis, expect=expect, hot=[] if extra else None, split_emission=True, **extra)
        film, feat = _flat(65, 5, irr=0.8)                                   # a light's edge across the 0.5 validity line
        emis = np.zeros((5, 65, 4), F32)
        for cols, cov in ((np.s_[30:32], 0.25), (np.s_[32:34], 0.75)):       # emitter coverage 0.25: a surface pixel; 0.75: passed through
            emis[:, cols, :3] = np.asarray((6.0, 4.0, 2.0), F32) * F32(cov); emis[:, cols, 3] = cov
            feat[:, cols, :3] = 0.5 * (1 - cov); feat[:, cols, 3] = 1 - cov
            film[:, cols, :3] = (F32(0.5 * (1 - cov) * 0.8) + emis[:, cols, :3]) * film[:, cols, 3:4]
        S["split-band" + name] = Case((65, 5), pins, film, feat, emis=emis, expect=_keeps(_all_pixels(65, 5), film), hot=[] if extra else None, split_emission=True, **extra)
    return S


def _theta(pkg, size):
    return pixel_angle(pkg.scenes.cornell_box_small(*size).camera)


def _irr_of(c):
    """(irradiance before the clamp, valid) of a case, by the restatement's rule."""
    sampled, valid, demod, _ = decisions(c.film, c.feat)
    m = np.where(sampled[..., None], _mean(np.where(sampled[..., None], c.film, F32(1))), 0.0)
    if c.flags & SPLIT:
        m = np.maximum(m - c.emis[..., :3].astype(np.float64), 0.0)
    irr = np.where(demod, m / np.where(demod, c.feat[..., :3].astype(np.float64), 1.0), m)
    return np.where(valid[..., None], irr, 0.0), valid


# ------------------------------------------------------------------------------------------------------------------------ CPU: the restatements
def test_library_exports_the_probe(pkg):
    kit.assert_exports(pkg, ["mcpt_probe_denoise"], ["probe_denoise"])
    p = np.zeros(8, F32).ctypes.data_as(C.c_void_p)
    assert pkg.load_library().mcpt_probe_denoise(None, p, p, None, None, p) == 1


@pytest.mark.parametrize("flags", [0, SPLIT | CLAMP])
def test_ref_decides_the_albedo_threshold_in_fp32(flags):
    """float32(1e-3) is 0.001000000047...: greater than the double 1e-3 and not greater than itself.  The device keeps the mean of such a channel
    (fa.x > 1e-3f is false); a restatement that tests the widened albedo against the double divides it out: a factor of 1000."""
    assert float(A0) > 1e-3 and not A0 > F32(1e-3)
    film, feat = _flat(1, 1, irr=1.0)
    emis = np.zeros((1, 1, 4), F32)
    for a, demodulated in ((down32(A0), False), (A0, False), (up32(A0), True)):
        feat[0, 0, :3] = (a, 0.5, a)
        film[0, 0, :3] = (2.0, 2.0, 2.0)                                     # mean 0.5
        assert decisions(film, feat)[2][0, 0].tolist() == [demodulated, True, demodulated]
        out = denoise_robust_ref(film, feat, emis, 0.1, flags=flags)
        assert np.allclose(out[0, 0, :3], 0.5, rtol=1e-12)                   # a 1 x 1 image comes out as it went in, whichever way
    # where it shows: the channel's irradiance is the mean (0.5), not mean / albedo (500), next to a neighbour of irradiance 0.5
    film, feat = _flat(2, 1, irr=0.5)
    feat[0, 0, 0] = A0; film[0, 0, 0] = 0.5 * 4
    out = denoise_robust_ref(film, feat, np.zeros((1, 2, 4), F32), 0.1, flags=flags)
    assert abs(out[0, 0, 0] - 0.5) <= 1e-9 and abs(out[0, 1, 0] - 0.25) <= 1e-9
    feat[0, 0, 0] = up32(A0)                                                 # one ulp up it is divided out: 500 against 0.5
    out = denoise_robust_ref(film, feat, np.zeros((1, 2, 4), F32), 0.1, flags=flags, sigma_color=1e9)
    assert out[0, 1, 0] > 1.0


@pytest.mark.parametrize("flags", [0, SPLIT | CLAMP])
def test_ref_decides_coverage_and_count_in_fp32(flags):
    film, feat = _flat(3, 1, irr=1.0)
    film[0, 1, :3] = (1.0, 3.0, 5.0); film[0, 1, 3] = 3.0                    # a mean that is not exact: 1/3, 1, 5/3
    emis = np.zeros((1, 3, 4), F32)
    for cov, valid in ((down32(0.5), False), (F32(0.5), True), (up32(0.5), True)):
        feat[0, 1, 3] = cov
        assert bool(decisions(film, feat)[1][0, 1]) == valid
        out = denoise_robust_ref(film, feat, emis, 0.1, flags=flags)
        passed = film[0, 1, :3] / film[0, 1, 3]                              # the fp32 quotient, bit for bit
        assert np.array_equal(out[0, 1, :3], passed.astype(np.float64)) != valid and out[0, 1, 3] == 1.0
    feat[0, 1, 3] = 0.25
    for cnt, shown in ((F32(0), False), (TINY, True)):
        film[0, 1] = (2 * cnt, 4 * cnt, 6 * cnt, cnt)
        out = denoise_robust_ref(film, feat, emis, 0.1, flags=flags)
        assert out[0, 1].tolist() == ([2.0, 4.0, 6.0, 1.0] if shown else [0.0, 0.0, 0.0, 0.0])


def test_ref_variance_is_zero_on_a_constant_patch_and_exact_on_a_known_one():
    lum = np.full((5, 6), 1.3 * float(LUM.sum()))
    valid = np.ones((5, 6), bool)
    assert np.all(variance3x3(lum, valid) == 0.0)
    lum = np.arange(30, dtype=np.float64).reshape(5, 6)
    var = variance3x3(lum, valid)
    assert abs(var[2, 2] - np.var(lum[1:4, 1:4])) < 1e-12 and abs(var[0, 0] - np.var(lum[0:2, 0:2])) < 1e-12
    valid[2, 2] = False
    assert var[2, 2] > 0 and variance3x3(lum, valid)[2, 2] == 0.0
    assert abs(variance3x3(lum, valid)[1, 1] - np.var(np.delete(lum[0:3, 0:3].ravel(), 8))) < 1e-12


@pytest.mark.parametrize("name", list(cases()))
def test_ref_on_the_case(pkg, name):
    """The restatement alone on every case: finite, what the case is built to show, the margins of its near misses, and (inside denoise_ref)
    that a level whose step reaches the image's larger side is the identity."""
    c = cases()[name]
    out = c.ref(_theta(pkg, c.size))
    assert np.all(np.isfinite(out))
    if c.expect:
        c.expect(out)
    if c.flags & CLAMP:
        irr, valid = _irr_of(c)
        k = c.opts["firefly_clamp"]
        _, hot = clamp_fireflies(irr, valid, k)
        assert sorted(zip(*np.nonzero(hot))) == sorted(c.hot)
        lum = irr @ LUM
        for y, x in zip(*np.nonzero(valid)):
            nb = [lum[q] for q in _all_pixels(*c.size) if q != (y, x) and abs(q[0] - y) <= 1 and abs(q[1] - x) <= 1 and valid[q]]
            if nb and max(nb) > 0:
                ratio = lum[y, x] / (k * max(nb))
                assert ratio == 1.0 or abs(ratio - 1.0) >= 2.0 ** -12, (y, x, ratio)


def test_cases_meet_every_edge_they_name():
    """The inputs themselves: every decision is taken both ways and on its boundary somewhere in the set."""
    S = cases()
    cov = np.concatenate([c.feat[..., 3].ravel() for c in S.values()])
    assert {float(down32(0.5)), 0.5, float(up32(0.5))} <= set(cov.tolist())
    cnt = np.concatenate([c.film[..., 3].ravel() for c in S.values()])
    assert {0.0, float(TINY)} <= set(cnt.tolist())
    alb = S["albedo-threshold"].feat[..., :3]
    for a in (down32(A0), A0, up32(A0), F32(0)):
        assert np.any(alb == a)
    assert np.any(np.all(S["normal-zero"].feat[..., 4:7] == 0, -1)) and np.any(S["depth-zero-centre"].feat[..., 7] == 0)
    assert {c.size for c in S.values()} == set(SHAPES)
    assert all(c.feat[..., 7].min() >= 0 for c in S.values())                # the probe's precondition


# ------------------------------------------------------------------------------------------------------------------------ GPU
_CTX = {}


def _renderer(pkg, size):
    """A context of that film size; it renders nothing."""
    if size not in _CTX:
        _CTX[size] = pkg.Renderer(pkg.scenes.cornell_box_small(*size), max_depth=2)
    return _CTX[size]


@pytest.fixture(scope="module", autouse=True)
def _close_renderers():
    yield
    for r in _CTX.values():
        r.close()
    _CTX.clear()


def verdict(name, out, ref, film, feat):
    """Every pixel, none left out.  Decisions exact: a pixel the restatement passes through is the fp32 mean bit for bit, a pixel without a count
    {0, 0, 0, 0}, alpha exactly 1 elsewhere.  Values: |out - ref| <= 1e-3 max(1, |ref|)."""
    sampled, valid, _, passed = decisions(film, feat)
    assert out.dtype == F32 and np.all(np.isfinite(out))
    assert np.all(out[~sampled] == 0)
    assert np.all(out[sampled][:, 3] == 1)
    thru = sampled & ~valid
    assert np.array_equal(kit.bits(out[thru][:, :3]), kit.bits(passed[thru].astype(F32)))
    err = np.abs(out.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    worst = np.unravel_index(np.argmax(err), err.shape)
    print("[denoise edges] %-34s worst |out - ref| / max(1, |ref|) = %.3e at (y, x, c) = %s  (%d valid, %d passed through, %d empty)" % (
        name, err[worst], worst, valid.sum(), thru.sum(), (~sampled).sum()))
    assert err[worst] <= BOUND, (name, worst, float(out[worst]), float(ref[worst]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases()))
def test_probe_matches_the_restatement(pkg, name):
    c = cases()[name]
    r = _renderer(pkg, c.size)
    out = r.probe_denoise(c.film, c.feat, c.emis, **c.opts)
    verdict(name, out, c.ref(_theta(pkg, c.size)), c.film, c.feat)
    if c.expect:
        c.expect(out.astype(np.float64))


@pytest.mark.gpu
def test_unnormalised_normals_filter_like_normalised_ones(pkg):
    S = cases()
    r = _renderer(pkg, (5, 7))
    outs = [r.probe_denoise(S[n].film, S[n].feat, **S[n].opts).astype(np.float64) for n in ("normals-x1", "normals-x0.3", "normals-x7")]
    for o in outs[1:]:
        assert np.all(np.abs(o - outs[0]) <= BOUND * np.maximum(1.0, np.abs(outs[0])))
        assert np.abs(o - outs[0]).max() <= 1e-4                                # (rounding of the scaled components: ~ 128 * 2^-23)


@pytest.mark.gpu
@pytest.mark.parametrize("clamp", [False, True])
def test_zero_emission_splits_to_the_same_bits(pkg, clamp):
    """SPLIT with E = 0 is fmaxf(c - 0, 0) = c and o + 0: the same bits as the probe without the split (dn_prep_robust_kernel's variance sums
    in dn_prep_kernel's order)."""
    kw = dict(clamp_fireflies=True, firefly_clamp=2.0) if clamp else {}
    for size, seed in (((5, 7), 21), ((130, 9), 22)):
        film, feat = _varied(*size, seed)
        feat[0, 0, 3] = 0.25; film[-1, -1] = 0.0
        r = _renderer(pkg, size)
        plain = r.probe_denoise(film, feat, **kw)
        split = r.probe_denoise(film, feat, np.zeros(film.shape, F32), split_emission=True, **kw)
        assert np.array_equal(kit.bits(split), kit.bits(plain))


@pytest.mark.gpu
def test_probe_refusals_leave_the_output_untouched(pkg):
    r = _renderer(pkg, (5, 7))
    film, feat = _varied(5, 7, 23)
    emis = np.zeros((7, 5, 4), F32)
    out = np.full((7, 5, 4), 7.5, F32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def status(film=film, feat=feat, emis=None, out=out, opts=True, **fields):
        o = pkg.DenoiseOpts(); o.struct_size = C.sizeof(pkg.DenoiseOpts)
        for k, v in fields.items():
            setattr(o, k, v)
        return r.lib.mcpt_probe_denoise(r.ctx, vp(film), vp(feat), vp(emis), C.byref(o) if opts else None, vp(out))

    def spoilt(a, where, value):
        b = a.copy(); b[where] = value
        return b

    refused = [dict(film=None), dict(feat=None), dict(out=None), dict(flags=SPLIT), dict(emis=emis), dict(emis=emis, flags=CLAMP), dict(emis=emis, opts=False),
               dict(feat=spoilt(feat, (3, 2, 0), np.nan)), dict(feat=spoilt(feat, (3, 2, 5), np.inf)), dict(feat=spoilt(feat, (6, 4, 7), -np.inf)),
               dict(feat=spoilt(feat, (6, 4, 7), -1e-30)), dict(feat=spoilt(feat, (0, 0, 7), -2.0)),
               dict(emis=spoilt(emis, (6, 4, 3), np.nan), flags=SPLIT), dict(emis=spoilt(emis, (0, 0, 0), np.inf), flags=SPLIT),
               # the options, as mcpt_denoise refuses them
               dict(iterations=11), dict(sigma_color=-1.0), dict(sigma_normal=float("nan")), dict(sigma_depth=-0.5), dict(flags=0x4), dict(flags=0x80000001, emis=emis),
               dict(flags=CLAMP, firefly_clamp=0.5), dict(flags=CLAMP, firefly_clamp=float("inf")), dict(firefly_clamp=-1.0), dict(struct_size=C.sizeof(pkg.DenoiseOpts) - 4)]
    b = r.info().device_bytes
    for bad in refused:
        assert status(**bad) == 1, bad
        assert np.all(out == 7.5), bad
    assert b"depth" in (status(feat=spoilt(feat, (0, 0, 7), -2.0)), r.lib.mcpt_last_error())[1]
    assert status(opts=False) == 0 and status(emis=emis, flags=SPLIT) == 0 and status(feat=spoilt(feat, (0, 0, 7), 0.0)) == 0
    assert np.all(out[..., 3] == 1) and r.info().device_bytes == b
    with pytest.raises(pkg.McptError):
        r.features()                                                          # the context still holds nothing of its own
    with pytest.raises(pkg.McptError):
        r.denoised_device_ptr()


@pytest.mark.gpu
def test_probe_leaves_the_context_alone_and_equals_denoise(pkg):
    """A probe between render_features + denoise calls changes nothing the context holds; probe_denoise(read_accum(), features()) is denoise()
    of the same context bit for bit, with and without the flags: what the cases above pin is the shipped path."""
    scene = pkg.scenes.cornell_box_small(65, 5)
    r = pkg.Renderer(scene, max_depth=4)
    r.render(4, seed=7); r.render_features(spp=4, seed=7)
    robust = dict(split_emission=True, clamp_fireflies=True, firefly_clamp=2.0)
    want_robust = r.denoise(**robust)
    want = r.denoise(iterations=3)
    film, feat, emis, b = r.read_accum(), r.features(), r.emission(), r.info().device_bytes
    other_film, other_feat = _varied(65, 5, 24)
    r.probe_denoise(other_film, other_feat, np.ones((5, 65, 4), F32), iterations=1, **robust)
    got = np.zeros_like(want)
    r._check(r.lib.mcpt_read_denoised(r.ctx, got.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(kit.bits(got), kit.bits(want))
    assert np.array_equal(kit.bits(r.features()), kit.bits(feat)) and np.array_equal(kit.bits(r.emission()), kit.bits(emis))
    assert np.array_equal(kit.bits(r.read_accum()), kit.bits(film)) and r.info().device_bytes == b
    assert np.array_equal(kit.bits(r.probe_denoise(film, feat, iterations=3)), kit.bits(want))
    assert np.array_equal(kit.bits(r.probe_denoise(film, feat, emis, **robust)), kit.bits(want_robust))
    assert np.array_equal(kit.bits(r.denoise(iterations=3)), kit.bits(want))
    r.close()
