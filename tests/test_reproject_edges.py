"""Reprojection at every decision boundary: rp_gather's chain of comparisons, each pinned on both sides of its boundary and
on it, against tests/reproject_edges_ref.py -- a per-pixel restatement that decides instead of forgiving (no marginal mask).

Inputs are built so that the restatement alone decides every pixel: two cameras at the same eye whose image planes differ by a factor of two
land every new pixel on a quarter, half or whole old pixel (within 1e-14), and films and features lie on a dyadic lattice (counts 1 .. 4, means in
eighths, axis normals, depth 4) on which every fp32 product and sum is exact whatever the contraction.  CPU tests check the restatement and
the inputs (no undecided pixel; every comparison taken both ways and on its boundary); GPU tests run the same inputs through
Renderer.probe_reproject and probe_reproject_motion, and re-check the random-camera cases of the two older suites without their 1e-4 mask.
"""
from __future__ import annotations

import collections
import functools
import math

import numpy as np
import pytest

from tests import test_reproject as t_cam
from tests import test_reproject_motion as t_mot
from tests.kit import Cam
from tests.reproject_edges_ref import Expected, compare_decided, reproject_edges_ref, reproject_motion_edges_ref
from tests.reproject_motion_ref import emissive_faces
from tests.reproject_ref import reproject_ref

F32 = np.float32
EYE, LOOK, UP, SKEW_UP = (0.25, 0.5, 4.0), (0.25, 0.5, 0.0), (0.0, 1.0, 0.0), (0.3, 1.7, 0.4)
WIDE, NARROW = 90.0, math.degrees(2.0 * math.atan(0.5))                     # h = 2 tan(fovy / 2) = 2 and 1
OPTS = dict(max_history=32.0, depth_tolerance=0.5, normal_threshold=1.0)
TINY = float(np.nextafter(F32(0), F32(1)))                                  # the smallest normal_threshold the options accept
INF, NAN = float("inf"), float("nan")


def up32(x):
    return np.nextafter(F32(x), F32(np.inf))


def down32(x):
    return np.nextafter(F32(x), F32(-np.inf))


def _cam(fovy, w, h, lookat=LOOK, up=UP):
    return Cam(EYE, lookat, up, fovy, w, h)


def _lattice(w, h):
    """(film, features) on the dyadic lattice: counts 1 .. 4, means multiples of 1/8 that differ from pixel to pixel, full coverage, normal +z,
    depth 4."""
    ys, xs = np.mgrid[0:h, 0:w]
    cnt = (1 + (xs + 2 * ys) % 4).astype(F32)
    film = np.zeros((h, w, 4), F32)
    for c in range(3):
        film[..., c] = cnt * (((3 * xs + 5 * ys + 2 * c) % 8 + 1) / 8.0)
    film[..., 3] = cnt
    feat = np.zeros((h, w, 8), F32)
    feat[..., :3] = 0.5; feat[..., 3] = 1.0; feat[..., 6] = 1.0; feat[..., 7] = 4.0
    return film, feat


class Scenario:
    """One probe input.  expect: {(y, x) of a new pixel: the count it must get} -- what the scenario is about, beside the full comparison."""

    def __init__(self, pair, w, h, opts=None, **cams):
        old_fovy, new_fovy = {"quarter": (WIDE, NARROW), "whole": (NARROW, WIDE), "half": (NARROW, WIDE), "same": (NARROW, NARROW)}[pair]
        self.old_cam = cams.get("old_cam") or _cam(old_fovy, w, h)
        self.new_cam = cams.get("new_cam") or _cam(new_fovy, w, h)
        self.film, self.old_feat = _lattice(w, h)
        self.new_feat = _lattice(w, h)[1]
        self.opts = dict(OPTS); self.opts.update(opts or {})
        self.expect = {}
        self.size = (w, h)


def _whole_tap(x, y):
    """(row, column) of the old pixel the new pixel (x, y) of the 7 x 5 whole-pixel pair lands on: sx = 2 x - 3, sy = 2 y - 2."""
    return 2 * y - 2, 2 * x - 3


def _half_taps(x, y):
    """The two old pixels of weight 1/2 under the new pixel (x, y) of the 8 x 5 half-pixel pair: sx = 2 x - 3.5, sy = 2 y - 2."""
    return (2 * y - 2, 2 * x - 4), (2 * y - 2, 2 * x - 3)


def _set_count(s, q, count):
    """A new sample count for the old pixel q, its mean kept."""
    mean = s.film[q][:3] / s.film[q][3]
    s.film[q][:3] = mean * F32(count) if np.isfinite(count) and count > 0 else mean
    s.film[q][3] = count


@functools.lru_cache(maxsize=None)
def scenarios():
    S = collections.OrderedDict()
    # ---- quarter pixels: sx = x / 2 + 1.75, sy = y / 2 + 0.75; weights 1/16, 3/16, 3/16, 9/16
    S["quarter-plain"] = s = Scenario("quarter", 8, 4)
    s.expect = {(y, x): None for y in range(4) for x in range(8)}           # (None: written, the count left to the reference)
    # the new pixel (2, 1) lands on (2.75, 1.25): taps (2,1) 3/16, (3,1) 9/16, (2,2) 1/16, (3,2) 3/16 [as (x, y)]
    S["quarter-floor-3/16"] = s = Scenario("quarter", 8, 4)
    keep = s.film[1, 2].copy(); s.film[...] = 0; s.film[1, 2] = keep
    s.expect = {(1, 2): 0, (1, 1): 1}                                        # 3/16 < 1/4 dropped; the neighbour sees the same tap with 9/16
    S["quarter-floor-1/4"] = s = Scenario("quarter", 8, 4)
    keep = s.film[1:3, 2].copy(); s.film[...] = 0; s.film[1:3, 2] = keep
    s.expect = {(1, 2): 2}                                                   # sw = 3/16 + 1/16 = 1/4 kept; (3 * 1 + 1 * 3) / 4 = 1.5 -> 2
    S["quarter-floor-9/16"] = s = Scenario("quarter", 8, 4)
    keep = s.film[1, 3].copy(); s.film[...] = 0; s.film[1, 3] = keep
    s.expect = {(1, 2): 2}                                                   # sw = 9/16, the one tap's count
    # ---- whole pixels: the new pixels x = 2, 3, 4 / y = 1, 2, 3 land on one old pixel each; x = 1 on sx = -1, x = 5 on sx = W
    S["whole-plain"] = s = Scenario("whole", 7, 5)
    s.expect = {(y, x): (float(s.film[_whole_tap(x, y)][3]) if x in (2, 3, 4) and y in (1, 2, 3) else 0) for y in range(5) for x in range(7)}
    S["whole-coverage"] = s = Scenario("whole", 7, 5)
    for x, cov, kept in ((2, F32(0.5), True), (3, down32(0.5), False), (4, up32(0.5), True)):
        q = _whole_tap(x, 1)
        s.old_feat[q][3] = cov; s.expect[(1, x)] = float(s.film[q][3]) if kept else 0
        s.new_feat[2, x, 3] = cov; s.expect[(2, x)] = float(s.film[_whole_tap(x, 2)][3]) if kept else 0
    S["whole-depth"] = s = Scenario("whole", 7, 5)
    # r = 4, tolerance 0.5: |z - 4| <= 2.  Below, 4 - nextafter(2, 0) = 2 + 2^-23 is a tie that rounds to 2 (kept); the next float down is dropped
    for (x, y), z, kept in (((2, 1), F32(6), True), ((3, 1), up32(6), False), ((4, 1), F32(2), True), ((2, 2), down32(2), True),
                            ((3, 2), down32(down32(2)), False), ((4, 2), F32(5), True)):
        q = _whole_tap(x, y)
        s.old_feat[q][7] = z; s.expect[(y, x)] = float(s.film[q][3]) if kept else 0
    for name, thr in (("whole-cosine-one", 1.0), ("whole-cosine-least", TINY)):
        S[name] = s = Scenario("whole", 7, 5, dict(normal_threshold=thr))
        for (x, y), n, kept in (((2, 1), (0, 0, 2), True), ((3, 1), (1, 0, 0), False), ((4, 1), (0, 0, -1), False), ((2, 2), (0, 2, 0), False)):
            q = _whole_tap(x, y)
            s.old_feat[q][4:7] = n; s.expect[(y, x)] = float(s.film[q][3]) if kept else 0
        s.new_feat[2, 3, 4:7] = (0, 0, 2); s.expect[(2, 3)] = float(s.film[_whole_tap(3, 2)][3])
        s.new_feat[2, 4, 4:7] = (0, 2, 0); s.old_feat[_whole_tap(4, 2)][4:7] = (0, 1, 0); s.expect[(2, 4)] = float(s.film[_whole_tap(4, 2)][3])
    S["whole-counts"] = s = Scenario("whole", 7, 5)
    # the landing's own tap spoiled: the three stray taps (weight 0) stay valid and must not count
    for (x, y), count, want in (((2, 1), 0.0, 0), ((3, 1), 1e-40, 0), ((4, 1), -0.0, 0), ((2, 2), -2.0, 0), ((3, 2), NAN, 0), ((4, 2), INF, 32)):
        _set_count(s, _whole_tap(x, y), count); s.expect[(y, x)] = want
    s.film[_whole_tap(3, 1)][:3] = 0                                        # (a denormal count: the mean of anything else would overflow)
    s.film[_whole_tap(2, 3)][1] = NAN; s.expect[(3, 2)] = float(s.film[_whole_tap(2, 3)][3])
    s.film[_whole_tap(3, 3)][:3] *= -1; s.expect[(3, 3)] = float(s.film[_whole_tap(3, 3)][3])
    S["whole-normals"] = s = Scenario("whole", 7, 5)
    for x, n in ((2, (0, 0, 0)), (3, (1e-23, 1e-23, 1e-23)), (4, (1e20, 1e20, 1e20))):
        s.new_feat[1, x, 4:7] = n; s.expect[(1, x)] = 0
        s.old_feat[_whole_tap(x, 2)][4:7] = n; s.expect[(2, x)] = 0
        s.expect[(3, x)] = float(s.film[_whole_tap(x, 3)][3])
    S["whole-new-depth"] = s = Scenario("whole", 7, 5)
    for (x, y), z in (((2, 1), 0.0), ((3, 1), -0.0), ((4, 1), -4.0), ((2, 2), INF), ((3, 2), NAN)):
        s.new_feat[y, x, 7] = z; s.expect[(y, x)] = 0
    s.expect[(2, 4)] = float(s.film[_whole_tap(4, 2)][3])
    # ---- half pixels in x: two taps of weight 1/2
    for name, cap in (("half-counts", 32.0), ("half-cap-equal", 4.0), ("half-cap-below", 3.0), ("half-cap-fraction", 2.5)):
        S[name] = s = Scenario("half", 8, 5, dict(max_history=cap))
        pairs = {(2, 1): ((1, 2), 2), (3, 1): ((2, 3), 2), (4, 1): ((3, 4), 4), (5, 1): ((0.25, 0.75), 0), (2, 2): ((0.5, 0.75), 1),
                 (3, 2): ((0.0, 2), 2), (4, 2): ((-0.0, 2), 2), (5, 2): ((-1.0, 2), 2), (2, 3): ((NAN, 2), 2), (3, 3): ((INF, 2), INF)}
        for (x, y), (counts, want) in pairs.items():
            for q, c in zip(_half_taps(x, y), counts):
                _set_count(s, q, c)
            s.expect[(y, x)] = min(want, cap) if want >= 1 else 0
        a, b = _half_taps(4, 3)
        _set_count(s, a, 2); _set_count(s, b, 2); s.film[a][0] = NAN; s.expect[(3, 4)] = 2
        a, b = _half_taps(5, 3)
        _set_count(s, a, 3); _set_count(s, b, 3); s.film[a][:3] *= -1; s.expect[(3, 5)] = min(3, cap)
        s.expect[(0, 1)] = 0                                                 # sx = -1.5: outside
    # ---- the identity: every pixel on itself, across the 64-wide and 4-high block edges
    for name, up in (("identity-ortho", UP), ("identity-skew", SKEW_UP)):
        c = _cam(NARROW, 130, 9, up=up)
        S[name] = s = Scenario("same", 130, 9, old_cam=c, new_cam=c)
        s.expect = {(y, x): float(s.film[y, x, 3]) for y in range(9) for x in range(130)}
    # ---- turned about `up` at the same eye: 90 degrees puts the centre column of an odd width on c0 = 0, 180 degrees everything behind the eye
    S["turned-90-axes"] = s = Scenario("same", 7, 5, new_cam=_cam(NARROW, 7, 5, lookat=(EYE[0] - 4.0, 0.5, 4.0)))      # c0 = 0 exactly
    s.expect = {(y, x): 0 for y in range(5) for x in range(7)}
    old = _cam(NARROW, 7, 5, lookat=(1.0, 0.75, 0.5))                       # front (0.75, 0.25, -3.5) / |.|; turned: (-3.5, 0.25, -0.75)
    S["turned-90"] = s = Scenario("same", 7, 5, old_cam=old, new_cam=_cam(NARROW, 7, 5, lookat=(-3.25, 0.75, 3.25)))   # c0 = 0 +- rounding
    s.expect = {(y, 3): 0 for y in range(5)}
    S["turned-180"] = s = Scenario("same", 7, 5, old_cam=old, new_cam=_cam(NARROW, 7, 5, lookat=(-0.5, 0.25, 7.5)))
    s.expect = {(y, x): 0 for y in range(5) for x in range(7)}
    return S


NAMES = ["quarter-plain", "quarter-floor-3/16", "quarter-floor-1/4", "quarter-floor-9/16", "whole-plain", "whole-coverage", "whole-depth",
         "whole-cosine-one", "whole-cosine-least", "whole-counts", "whole-normals", "whole-new-depth", "half-counts", "half-cap-equal",
         "half-cap-below", "half-cap-fraction", "identity-ortho", "identity-skew", "turned-90-axes", "turned-90", "turned-180"]


@functools.lru_cache(maxsize=None)
def _expected(name, centre=(0.0, 0.0, 0.0)):
    s = scenarios()[name]
    return reproject_edges_ref(s.old_cam, s.new_cam, s.film, s.old_feat, s.new_feat, centre=centre, **s.opts)


# ------------------------------------------------------------------------------------------------------------------------ motion inputs
MOTION_EYE, MOTION_LOOK = (2.0, 0.0, 4.0), (2.0, 0.0, 0.0)
WALL, QUAD, LAMP = 0, 2, 4                                                   # a face of each part of test_reproject_motion's world


class MotionScenario:
    """test_reproject_motion's world (the context's scene) under an 8 x 4 camera whose old pixels are one world unit wide on the plane z = 0 (two
    with the WIDE old camera), and caller-made old vertices and hit records: the old wall triangle is A, A + 8 x, A + 8 y with A the point under
    old pixel (0, 0), so a hit (u, v) on it WAS at the old pixel coordinates (8 u, 8 v) -- (4 u + 1.75, 4 v + 0.75) for the WIDE camera -- exactly.
    By default the new pixel (x, y) hits (x / 8, y / 8): every pixel lands on itself."""

    def __init__(self, pkg, old_fovy=NARROW, shift=(0.0, 0.0, 0.0)):
        w, h = 8, 4
        self.size = (w, h)
        self.old_cam = Cam(MOTION_EYE, MOTION_LOOK, UP, old_fovy, w, h); self.new_cam = Cam(MOTION_EYE, MOTION_LOOK, UP, NARROW, w, h)
        self.scene = t_mot._world(pkg, w, h, self.new_cam)
        self.face, self.emissive = self.scene.face, emissive_faces(self.scene)
        assert list(self.face[WALL, :, 0]) == [0, 1, 2] and list(self.face[QUAD, :, 0]) == [4, 5, 6] and self.emissive[LAMP] and not self.emissive[:LAMP].any()
        self.old_v, self.old_n = self.scene.vertex.copy(), self.scene.normal.copy()
        A = np.array([MOTION_EYE[0] - 3.5, MOTION_EYE[1] - 1.5, 0.0])
        self.old_v[0] = A; self.old_v[1] = A + (8, 0, 0); self.old_v[2] = A + (0, 8, 0)
        self.old_v[:3] += shift
        self.film, self.old_feat = _lattice(w, h)
        self.old_feat[..., 7] = 5.0                                          # r runs from 4 to 6.2 over the image: |5 - r| <= r / 2 throughout
        self.new_feat = _lattice(w, h)[1]
        ys, xs = np.mgrid[0:h, 0:w]
        self.hit_face = np.full((h, w), WALL, np.int32)
        self.hit_uv = np.stack([xs / 8.0, ys / 8.0], -1).astype(F32)
        self.opts = dict(OPTS)
        self.expect = {}

    def hit(self, x, y, face, u=0.0, v=0.0):
        self.hit_face[y, x] = face; self.hit_uv[y, x] = (u, v)


@functools.lru_cache(maxsize=None)
def motion_scenarios():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    S = collections.OrderedDict()
    S["motion-lattice"] = s = MotionScenario(pkg)
    s.expect = {(y, x): float(s.film[y, x, 3]) for y in range(4) for x in range(8)}         # u = 0 down column 0, v = 0 along row 0, a corner at (0, 0)
    s.hit(1, 1, WALL, 0.75, 0.25); s.expect[(1, 1)] = float(s.film[2, 6, 3])                 # u + v = 1
    s.hit(2, 1, WALL, 1.0, 0.0); s.expect[(1, 2)] = 0                                        # the corner V1: sx = W
    s.hit(3, 1, WALL, 0.875, 0.25); s.expect[(1, 3)] = float(s.film[2, 7, 3])                # outside the triangle (w = -1/8), inside the image
    s.hit(4, 1, WALL, 2.75 / 8, 1.25 / 8); s.expect[(1, 4)] = None                           # quarter weights
    s.hit(5, 1, -1); s.expect[(1, 5)] = 0                                                    # a miss
    s.hit(6, 1, LAMP, 0.25, 0.25); s.expect[(1, 6)] = 0                                      # an emitter
    s.hit(1, 2, WALL, -0.125, 0.25); s.expect[(2, 1)] = 0                                    # outside the triangle: sx = -1
    s.hit(2, 2, WALL, 2.5 / 8, 1.0 / 8); s.expect[(2, 2)] = None                             # half weights
    s.hit(4, 2, WALL, -0.25, 0.25); s.expect[(2, 4)] = 0                                     # sx = -2
    s.hit(5, 2, WALL, 1.25, 0.25); s.expect[(2, 5)] = 0                                      # sx = 10
    # an old normal exactly perpendicular to the view vector: the point under the eye, normal +x.  Turned either way it is perpendicular to the
    # taps' +z normals, so both branches end without history
    s.old_v[4] = (2, 0, 0); s.old_v[5] = (3, 0, 0); s.old_v[6] = (2, 1, 0); s.old_n[4:7] = (1, 0, 0)
    s.hit(3, 2, QUAD, 0.0, 0.0); s.expect[(2, 3)] = 0
    S["motion-zero-normal"] = s = MotionScenario(pkg)
    s.old_n[1] = (0, 0, -1)                                                  # the normal at (u, v) is (1 - 2 u) z: zero at u = 1/2, turned over beyond
    s.expect = {(y, x): (0 if x == 4 else float(s.film[y, x, 3])) for y in range(4) for x in range(8)}
    S["motion-whole-pixel-shift"] = s = MotionScenario(pkg, shift=(1.0, 0.0, 0.0))
    s.expect = {(y, x): (0 if x == 7 else float(s.film[y, x + 1, 3])) for y in range(4) for x in range(8)}
    S["motion-quarter"] = s = MotionScenario(pkg, old_fovy=WIDE)
    s.expect = {(y, x): None for y in range(4) for x in range(8)}
    # old vertices equal to the current ones, hits of the scene's own centre rays (test_reproject_motion's identity world)
    k = t_mot._plain_world(pkg, 20, 12, "identity")
    k.size, k.opts, k.expect = (20, 12), {}, {}
    S["motion-at-rest"] = k
    return S


MOTION_NAMES = ["motion-lattice", "motion-zero-normal", "motion-whole-pixel-shift", "motion-quarter", "motion-at-rest"]


@functools.lru_cache(maxsize=None)
def _motion_expected(name, centre=(0.0, 0.0, 0.0)):
    s = motion_scenarios()[name]
    return reproject_motion_edges_ref(s.old_cam, s.new_cam, s.film, s.old_feat, s.new_feat, s.hit_face, s.hit_uv, s.face, s.emissive, s.old_v, s.old_n,
                                      centre=centre, **s.opts)


def _check_expectations(s, want):
    for (y, x), count in s.expect.items():
        if count is None:
            assert want.film[y, x, 3] >= 1, (y, x)
        else:
            assert want.film[y, x, 3] == count, ((y, x), want.film[y, x, 3], count)


# ------------------------------------------------------------------------------------------------------------------------ CPU: inputs and reference
def test_the_scenario_lists_are_complete():
    assert list(scenarios()) == NAMES


def test_the_camera_pairs_land_where_stated():
    """The same-eye pairs of the module docstring, in the older restatement's own projection: within 1e-14 of the stated positions."""
    from tests.reproject_ref import basis_inverse, camera_constants, centre_rays, project
    for name, fx, fy in (("quarter-plain", lambda x: x / 2 + 1.75, lambda y: y / 2 + 0.75), ("whole-plain", lambda x: 2 * x - 3, lambda y: 2 * y - 2),
                         ("half-counts", lambda x: 2 * x - 3.5, lambda y: 2 * y - 2), ("identity-ortho", lambda x: x, lambda y: y),
                         ("identity-skew", lambda x: x, lambda y: y)):
        s = scenarios()[name]
        co, cn = camera_constants(s.old_cam), camera_constants(s.new_cam)
        sx, sy, c0 = project(co, basis_inverse(co), 4.0 * centre_rays(cn))
        ys, xs = np.mgrid[0:s.size[1], 0:s.size[0]]
        tol = 1e-14 if s.size[0] < 100 else 1e-12                            # (the wide film's coordinates are a hundred times larger)
        assert np.all(c0 > 0) and np.abs(sx - fx(xs)).max() < tol and np.abs(sy - fy(ys)).max() < tol, name


@pytest.mark.parametrize("name", NAMES)
def test_reference_decides_every_pixel_of_the_constructed_inputs(name):
    s, want = scenarios()[name], _expected(name)
    print("[edges] %s: %d pixels, %d evaluations, %d undecided" % (name, want.undecided.size, want.branches, int(want.undecided.sum())))
    assert not want.undecided.any()
    _check_expectations(s, want)
    if name in ("quarter-plain", "whole-plain", "half-counts", "quarter-floor-1/4"):
        assert want.exact.all() and not want.tol.any()                       # the lattice: bit for bit


def test_quarter_weights_and_ties_of_the_reference():
    """The restatement itself on values worked out by hand."""
    s, want = scenarios()["quarter-plain"], _expected("quarter-plain")
    # new pixel (2, 1) -> (2.75, 1.25): 3/16 (2,1) + 9/16 (3,1) + 1/16 (2,2) + 3/16 (3,2)
    w = {(1, 2): 3 / 16, (1, 3): 9 / 16, (2, 2): 1 / 16, (2, 3): 3 / 16}
    avg = sum(wq * s.film[q][3] for q, wq in w.items())
    assert want.film[1, 2, 3] == round(avg)
    for c in range(3):
        assert want.film[1, 2, c] == sum(wq * s.film[q][c] / s.film[q][3] for q, wq in w.items()) * round(avg)
    half = _expected("half-counts")
    assert [half.film[1, x, 3] for x in (2, 3, 4, 5)] == [2, 2, 4, 0] and half.film[2, 2, 3] == 1      # 1.5, 2.5, 3.5, 0.5 and 0.625 rounded half to even
    assert _expected("half-cap-fraction").film[1, 4, 3] == 2.5 and _expected("half-cap-below").film[1, 4, 3] == 3
    inf = _expected("whole-counts").film[2, 4]
    assert list(inf) == [0, 0, 0, 32]                                        # an infinite count: the mean reads 0, the count caps


BOTH_WAYS = ["new coverage >= 0.5", "new depth > 0", "new normal length > 0", "in front of the old eye", "sx > -1", "sx < W", "sy > -1", "sy < H",
             "tap inside the image", "tap weight > 0", "old count > 0", "old coverage >= 0.5", "depth within tolerance", "tap normal length > 0",
             "cosine >= threshold", "sw >= 0.25", "count above the cap", "history >= 1"]
ON_THE_BOUNDARY = ["new coverage >= 0.5", "new depth > 0", "new normal length > 0", "in front of the old eye", "tap weight > 0", "old count > 0",
                   "old coverage >= 0.5", "depth within tolerance", "tap normal length > 0", "cosine >= threshold", "sw >= 0.25", "count above the cap",
                   "history >= 1"]
WITHIN_BOUND = ["in front of the old eye", "sx > -1", "sx < W", "floor sx takes the upper cell", "floor sy takes the upper cell"]


def test_every_boundary_is_taken_both_ways_and_on_it():
    total = collections.Counter()
    for name in NAMES:
        total.update(_expected(name).stats)
    for name in BOTH_WAYS:
        print("[edges] %-28s true %5d  false %5d  equal %4d  within bound %4d" % (name, total[(name, True)], total[(name, False)], total[(name, "equal")],
                                                                                 total[(name, "within bound")]))
        assert total[(name, True)] > 0 and total[(name, False)] > 0, name
    for name in ON_THE_BOUNDARY:
        assert total[(name, "equal")] > 0, name
    for name in WITHIN_BOUND:
        assert total[(name, "within bound")] > 0, name
    assert total[("rint", "tie")] >= 4 and total[("rint", "up")] > 0 and total[("rint", "down")] > 0 and total[("rint", "whole")] > 0
    # the motion kernel's own decisions
    motion = collections.Counter()
    for name in MOTION_NAMES:
        motion.update(_motion_expected(name).stats)
    for name in ("first hit names a triangle", "first hit is no emitter", "old normal length > 0", "old normal faces away from the old eye", "sx > -1", "sx < W"):
        print("[edges] %-40s true %5d  false %5d  equal %4d" % (name, motion[(name, True)], motion[(name, False)], motion[(name, "equal")]))
        assert motion[(name, True)] > 0 and motion[(name, False)] > 0, name
    assert motion[("old normal length > 0", "equal")] > 0 and motion[("old normal faces away from the old eye", "equal")] > 0


@pytest.mark.parametrize("name", MOTION_NAMES)
def test_reference_decides_every_pixel_of_the_motion_inputs(name):
    s, want = motion_scenarios()[name], _motion_expected(name)
    print("[edges] %s: %d pixels, %d evaluations, %d undecided" % (name, want.undecided.size, want.branches, int(want.undecided.sum())))
    assert not want.undecided.any()
    _check_expectations(s, want)
    if name == "motion-at-rest":
        surface = s.new_feat[..., 3] >= 0.5
        assert 0.5 < surface.mean() < 1.0 and np.array_equal(want.film[..., 3] > 0, surface)


def _old_cases():
    """The random-camera probe cases of the two older suites: (id, the new reference given a centre, the old reference (film, marginal mask))."""
    for case in t_cam.PROBE_CASES:
        ca, cb, film, fa, fb, opts = t_cam._probe_case(*case)
        a = (ca, cb, film, fa, fb)
        yield ("camera", case), (lambda c, a=a, o=opts: reproject_edges_ref(*a, centre=c, **o)), (lambda a=a, o=opts: reproject_ref(*a, **o))
    for case in t_mot.PROBE_CASES:
        k = t_mot._probe_case(*case)
        a = (k.old_cam, k.new_cam, k.film, k.old_feat, k.new_feat, k.hit_face, k.hit_uv, k.face, k.emissive, k.old_v, k.old_n)
        yield ("motion", case), (lambda c, a=a, o=k.opts: reproject_motion_edges_ref(*a, centre=c, **o)), (lambda k=k: t_mot._ref(k))


@functools.lru_cache(maxsize=None)
def _old_case_expected(kind, case, centre=(0.0, 0.0, 0.0)):
    for key, ref, _ in _old_cases():
        if key == (kind, case):
            return ref(centre)
    raise KeyError((kind, case))


def test_random_cases_leave_fewer_pixels_undecided_than_the_margin_did():
    undecided = marginal = 0
    for (kind, case), _, old_ref in _old_cases():
        old, marg = old_ref()
        want = _old_case_expected(kind, case)
        print("[edges] %s %s: undecided %d, marginal under the old rule %d" % (kind, case, int(want.undecided.sum()), int(marg.sum())))
        assert want.undecided.sum() <= marg.sum()
        ok = ~marg & ~want.undecided                                         # where both speak they say the same
        assert np.array_equal(old[ok][:, 3], want.film[ok][:, 3])
        assert np.allclose(old[ok][:, :3], want.film[ok][:, :3], rtol=1e-5, atol=1e-7)
        undecided += int(want.undecided.sum()); marginal += int(marg.sum())
    print("[edges] in total: undecided %d, marginal %d" % (undecided, marginal))
    assert undecided < marginal


def test_compare_decided_rejects_what_it_should():
    s, want = scenarios()["half-counts"], _expected("half-counts")
    good = want.film.astype(F32)
    n = int((good[..., 3] > 0).sum())
    none = np.zeros(want.undecided.shape, bool)
    compare_decided(good, n, want, none)
    for change in ("count", "colour", "reused", "ghost", "minus zero"):
        bad = good.copy(); reused = n
        if change == "count":
            bad[1, 3, 3] = 3                                                 # 2.5 rounded away from zero
        elif change == "colour":
            bad[1, 2, 0] = np.nextafter(bad[1, 2, 0], F32(9))                # one ulp on a pixel that must match bit for bit
        elif change == "reused":
            reused = n + 1
        elif change == "ghost":
            bad[0, 0] = (0.5, 0.5, 0.5, 0)                                   # colour in a pixel without history
        else:
            bad[0, 0, 0] = -0.0
        with pytest.raises(AssertionError):
            compare_decided(bad, reused, want, none)
    # a tolerance pixel: inside the bound passes, twice the bound does not
    rnd = _old_case_expected("camera", t_cam.PROBE_CASES[0])
    film = rnd.film.astype(F32)
    y, x = np.argwhere((rnd.film[..., 3] > 0) & ~rnd.exact & ~rnd.undecided)[0]
    count = int((film[..., 3] > 0).sum())
    und = rnd.undecided
    compare_decided(film, count, rnd, und)
    film[y, x, 0] = F32(rnd.film[y, x, 0] + 2.5 * rnd.tol[y, x, 0])
    with pytest.raises(AssertionError):
        compare_decided(film, count, rnd, und)
    assert isinstance(rnd, Expected)


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_probe_at_the_boundaries(pkg, name):
    s = scenarios()[name]
    r = pkg.Renderer(pkg.scenes.cornell_box_small(*s.size), max_depth=2)
    centre = tuple(float(c) for c in r.info().centre)
    got, reused = r.probe_reproject(s.old_cam, s.new_cam, s.film, s.old_feat, s.new_feat, **s.opts)
    r.close()
    want = _expected(name, centre)
    assert not want.undecided.any()
    _check_expectations(s, want)
    compare_decided(got, reused, want, want.undecided)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MOTION_NAMES)
def test_motion_probe_at_the_boundaries(pkg, name):
    s = motion_scenarios()[name]
    r = pkg.Renderer(s.scene, max_depth=2, flags=pkg.FLAG_DYNAMIC)
    centre = tuple(float(c) for c in r.info().centre)
    got, reused = r.probe_reproject_motion(s.old_cam, s.new_cam, s.film, s.old_feat, s.new_feat, s.hit_face, s.hit_uv, old_vertex=s.old_v, old_normal=s.old_n,
                                           **s.opts)
    r.close()
    want = _motion_expected(name, centre)
    print("[edges] %s: centre %s, %d undecided" % (name, centre, int(want.undecided.sum())))
    assert not want.undecided.any()
    compare_decided(got, reused, want, want.undecided)


@pytest.mark.gpu
@pytest.mark.parametrize("case", t_cam.PROBE_CASES, ids=lambda c: "%dx%d-%s-%s" % (c[0][0], c[0][1], c[1], c[2]))
def test_random_camera_cases_without_the_margin(pkg, case):
    ca, cb, film, fa, fb, opts = t_cam._probe_case(*case)
    r = pkg.Renderer(pkg.scenes.cornell_box_small(*case[0]), max_depth=2)
    centre = tuple(float(c) for c in r.info().centre)
    got, reused = r.probe_reproject(ca, cb, film, fa, fb, **opts)
    r.close()
    want = _old_case_expected("camera", case, centre)
    compare_decided(got, reused, want, want.undecided)


@pytest.mark.gpu
@pytest.mark.parametrize("case", t_mot.PROBE_CASES, ids=lambda c: "%dx%d-%s-%s" % (c[0][0], c[0][1], c[1], c[2]))
def test_random_motion_cases_without_the_margin(pkg, case):
    k = t_mot._probe_case(*case)
    r = pkg.Renderer(k.scene, max_depth=2, flags=pkg.FLAG_DYNAMIC)
    centre = tuple(float(c) for c in r.info().centre)
    got, reused = r.probe_reproject_motion(k.old_cam, k.new_cam, k.film, k.old_feat, k.new_feat, k.hit_face, k.hit_uv, old_vertex=k.old_v, old_normal=k.old_n,
                                           **k.opts)
    r.close()
    want = _old_case_expected("motion", case, centre)
    compare_decided(got, reused, want, want.undecided)
