"""Dual-quaternion skinning on the device: mcpt_set_skin_mode / mcpt_get_skin_mode, the two kernels sk_dq_vertices_kernel and
sk_dq_normals_kernel of csrc/skin.hip behind mcpt_update_skin, mcpt_update_skin_reproject and mcpt_update_morph with bones, and their public
surfaces.

The oracle throughout is §16's: a second context of the same scene WITHOUT the feature, moved with mcpt_update_vertices to the arrays
tests/skin_dq_ref.py computes (numpy, the kernels' association): fp64 multiply, add, subtract, divide and sqrt are correctly rounded on both
sides, so the two contexts hold the same device arrays and everything downstream is compared BIT FOR BIT, without a tolerance.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from tests import deform_kit as K, kit, morph_ref as M, normals_ref as NR, skin_dq_ref as D, skin_ref as S, transform_ref as T
from tests.deform_kit import CENTRE, FLAGS, H, INVALID, LAMP, M_LAMP, M_LOW, N_BONES, SPHERE, UNSUPPORTED, W, clean
from tests.kit import bits, render_film

NEW_SYMBOLS = ["mcpt_set_skin_mode", "mcpt_get_skin_mode"]
DYADIC = (0.5, 0.25, 0.125, 0.125)                                           # every partial sum and every product with 0 or 1 is exact
EPS = np.finfo(np.float64).eps
# A single influence against the bone's own A p + t: the worst error of the restatement against numpy.longdouble over 20 000 random rigid bones,
# |t| and |p| spanning 1e-3 .. 1e3 (seed 0), relative to |p|inf + |t|inf, was 1.641e-15 (five other seeds: 1.30e-15 .. 1.44e-15); 8 x that
# covers other seeds.  test_restatement_single_influence_is_the_bones_own_transform measures it again.
SINGLE_WORST = 1.641e-15
SINGLE_TOLERANCE = 8.0 * SINGLE_WORST


# test_skin.py's bend with the scalings taken out (dual-quaternion mode takes rigid bones only; M_LOW and M_LAMP are rigid as they are), and a twist
M_HIGH = clean(T.about(T.rotation((0, 0, 1), 25.0), (0.5, 0.1, 0.5), (0.03, 0.08, -0.04)))
M_THIRD = clean(T.about(T.rotation((1, 2, 3), 20.0), CENTRE, (0.01, 0.05, -0.02)))
M_OTHER = clean(T.about(T.rotation((0, 1, 0), -75.0), CENTRE, (-0.02, 0.05, 0.03)))
M_TWIST = clean(T.about(T.rotation((0, 1, 0), 170.0), CENTRE, (0.0, 0.05, 0.0)))   # linear blending leaves the sphere's waist at 0.087 of its radius
M_LIFT = clean(T.about(np.eye(3), CENTRE, (0.0, 0.05, 0.0)))
M_PLUS100 = clean(T.about(T.rotation((0, 1, 0), 100.0), CENTRE, (0.0, 0.05, 0.0)))
M_270 = clean(T.about(T.rotation((0, 1, 0), 270.0), CENTRE, (0.0, 0.06, 0.0)))   # the host's sign rule makes it -90 degrees
M_UNUSED = clean(T.about(np.eye(3), (5, 5, 5), (6e16, 0, 0)))                # a rigid bone without members: validated against R_b = 0, never read
M_SCALED = clean(T.about(T.rotation((0, 0, 1), 25.0) @ np.diag([0.9, 0.95, 0.9]), (0.5, 0.1, 0.5)))
M_MIRRORED = clean(T.about(T.rotation((0, 0, 1), 25.0) @ np.diag([1.0, 1.0, -1.0]), CENTRE))
M_SHEARED = clean(T.about(T.rotation((0, 0, 1), 25.0) @ np.array([[1.0, 0.01, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), CENTRE))


def _half_turn(axis):
    """The rotation by 180 degrees about a unit axis, 2 a a^T - I: symmetric to the last bit, so Shepperd's w comes out as exactly 0."""
    a = np.asarray(axis, np.float64)
    return 2.0 * np.outer(a, a) - np.eye(3)


# three half turns about axes 120 degrees apart whose sum is zero: their quaternions are (0, a_k) -- Shepperd's method makes the largest
# component positive, which is a_k's own here -- and a third of each is the degenerate blend
OPPOSED = [clean(T.about(_half_turn(np.array(a) / np.sqrt(1.5)), CENTRE)) for a in ((1.0, -0.5, -0.5), (-0.5, 1.0, -0.5), (-0.5, -0.5, 1.0))]
N_FOUR = 8                                                                   # the five bones above, then the three opposed ones


@functools.lru_cache(maxsize=None)
def _four(pkg):
    """Every sphere vertex with four random weights normalised in fp64 over bones 1 .. 3, a third of the slots exactly 0 with a random id of ANY
    of the eight bones in them -- slot 0, the pivot, included; walls on bone 0, lamp on bone 4.  The LAST record of the array is the constructed
    degenerate one: slot 0 of weight 0 on bone 0, then the three opposed bones at a third each."""
    s = K.scene(pkg); sphere, lamp = K.parts(pkg); n = int(sphere.sum())
    rng = np.random.default_rng(23)
    vb, vw = S.single(np.where(lamp, 4, 0))
    r = rng.uniform(0.05, 1.0, (n, 4)); ids = rng.integers(1, 4, (n, 4))
    zero = rng.uniform(size=(n, 4)) < 1.0 / 3.0
    zero[:, 3] &= ~zero.all(1)                                               # at least one slot carries weight
    r[zero] = 0.0; ids[zero] = rng.integers(0, N_FOUR, int(zero.sum()))
    w = r / r.sum(1, keepdims=True)
    assert (w == 0.0).sum() == zero.sum() > n and np.abs(S.weight_sums(w) - 1.0).max() <= 4 * EPS and (w[:, 0] == 0.0).sum() > n // 5
    vb[sphere] = ids; vw[sphere] = w
    last = s.vertex.shape[0] - 1
    assert sphere[last]
    vb[last] = (0, 5, 6, 7); vw[last] = (0.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)
    return (vb, vw) + tuple(pkg.skin_normals_from_faces(s, vb, vw))


def _mats(low=None, high=None, lamp=None, third=None, n=N_BONES):
    """deform_kit.mats with this suite's rigid far-away bone 3, and with the three opposed bones where there are eight."""
    m = K.mats(low, high, lamp, M_UNUSED if third is None else third, n)
    if n == N_FOUR: m[5:] = OPPOSED
    return m


BEND = _mats(low=M_LOW, high=M_HIGH, lamp=M_LAMP)
BEND2 = _mats(low=M_OTHER, high=M_THIRD)
TWIST = _mats(low=M_LIFT, high=M_TWIST, lamp=M_LAMP)                        # the lower bone only lifts the sphere off the floor, the upper one twists it too
FOUR = _mats(low=M_PLUS100, high=M_270, third=M_THIRD, lamp=M_LAMP, n=N_FOUR)


def _ref(pkg, matrices, skin=None, rest=None, small=False):
    """The arrays the bones give in dual-quaternion mode, by the restatement."""
    s = K.scene(pkg, small); vb, vw, nb, nw = K.bend(pkg, small) if skin is None else skin
    rv, rn = (s.vertex, s.normal) if rest is None else rest
    return D.skin_vertices(rv, vb, vw, matrices), D.skin_normals(rn, nb, nw, matrices)


def _ring(angle, mode):
    """A ring vertex at radius 0.7 about y, weight 1/2 on the identity and 1/2 on a rotation about y: (radius / rest radius, degrees turned)."""
    m = np.stack([T.identity(1)[0], clean(T.about(T.rotation((0, 1, 0), angle), (0, 0, 0)))])
    p = np.array([[0.7, 0.2, 0.0]])
    f = D.skin_vertices if mode == D.DUAL_QUATERNION else S.skin_vertices
    v = f(p, [[0, 1, 0, 0]], [[0.5, 0.5, 0.0, 0.0]], m)[0]
    assert v[1] == 0.2
    return float(np.hypot(v[0], v[2]) / 0.7), float(np.degrees(np.arctan2(-v[2], v[0])))


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_skin_mode_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, ("set_skin_mode", "skin_mode"))
    assert (pkg.SKIN_LINEAR, pkg.SKIN_DUAL_QUATERNION) == (D.LINEAR, D.DUAL_QUATERNION) == (0, 1)


def test_null_arguments_are_invalid_for_the_skin_mode_calls(pkg):
    lib = pkg.load_library()
    mode = C.c_uint32(77)
    assert lib.mcpt_set_skin_mode(None, pkg.SKIN_DUAL_QUATERNION) == INVALID
    assert lib.mcpt_get_skin_mode(None, C.byref(mode)) == INVALID and mode.value == 77
    assert lib.mcpt_get_skin_mode(None, None) == INVALID


def test_the_modes_have_the_headers_values(pkg, tmp_path):
    c, py, modes = K.c_layout(pkg.SkinInfo, "mcpt_skin_info", tmp_path, macros=("MCPT_SKIN_LINEAR", "MCPT_SKIN_DUAL_QUATERNION"))
    assert modes == [0, 1] and c[0] == C.sizeof(pkg.SkinInfo)


def test_restatement_a_twisted_ring_keeps_its_radius():
    """The defect and the remedy in numbers: linear blending shrinks a ring between two bones that differ by a twist, the dual-quaternion blend
    keeps its radius and turns it by half the angle -- by the SHORT way round: 270 degrees blend as -90."""
    for angle, turned in ((90.0, 45.0), (170.0, 85.0), (180.0, 90.0), (270.0, -45.0)):
        radius, degrees = _ring(angle, D.DUAL_QUATERNION)
        assert abs(radius - 1.0) <= 1e-12 and abs(degrees - turned) <= 1e-9, (angle, radius, degrees)
    assert abs(_ring(90.0, D.LINEAR)[0] - np.sqrt(0.5)) <= 1e-12
    assert _ring(170.0, D.LINEAR)[0] < 0.09                                   # the defect, pinned
    assert _ring(180.0, D.LINEAR)[0] < 1e-15
    # the same rule on the device's side of the contract: the pivot at +100 degrees and a bone at -100 have quaternions in opposite hemispheres
    # (both with w > 0), so the second enters negated and the blend is the half turn between them, not the identity
    m = np.stack([clean(T.about(T.rotation((0, 1, 0), 100.0), (0, 0, 0))), clean(T.about(T.rotation((0, 1, 0), -100.0), (0, 0, 0)))])
    q = D.dualquats(m)
    assert (q[:, 0] > 0).all() and D.signed_weights([[0, 1, 0, 0]], [[0.5, 0.5, 0.0, 0.0]], q)[0].tolist() == [0.5, -0.5, 0.0, 0.0]
    v = D.skin_vertices([[0.7, 0.2, 0.0]], [[0, 1, 0, 0]], [[0.5, 0.5, 0.0, 0.0]], m)[0]
    assert abs(v[0] + 0.7) <= 1e-15 and abs(v[2]) <= 1e-15 and v[1] == 0.2


def test_restatement_identity_bones_give_the_rest_pose(pkg):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    rng = np.random.default_rng(4)
    ids_v = rng.integers(0, 3, (nv, 4)); ids_n = rng.integers(0, 3, (nn, 4))
    dy_v = np.tile(DYADIC, (nv, 1)); dy_n = np.tile(DYADIC, (nn, 1))
    q = D.dualquats(T.identity(3))
    assert np.array_equal(q, np.tile([1.0, 0, 0, 0, 0, 0, 0, 0], (3, 1)))
    assert np.array_equal(D.skin_vertices(s.vertex, ids_v, dy_v, T.identity(3)), s.vertex)       # by value: a -0 may become +0
    unit = D.skin_normals(s.normal, ids_n, dy_n, T.identity(3))
    assert np.array_equal(bits(unit), bits(T.transform_normals(s.normal, np.zeros(nn, int), T.identity(1))))
    again = D.skin_normals(unit, ids_n, dy_n, T.identity(3))                  # normalised once: a fixed point in the fp32 numbers the shading streams hold
    assert np.array_equal(bits(again.astype(np.float32)), bits(unit.astype(np.float32)))


def _random_rigid(rng, n):
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.normal(size=(n, 3)); t /= np.abs(t).max(1, keepdims=True); t *= 10.0 ** rng.uniform(-3, 3, (n, 1))
    return np.concatenate([D.rotation_of(q), t[:, :, None]], 2)


@pytest.mark.parametrize("seed", [0, 12])
def test_restatement_single_influence_is_the_bones_own_transform(seed):
    """One influence of weight 1: the quaternion round trip gives the bone's own A p + t, to rounding.  The error is MEASURED against
    numpy.longdouble (relative to |p|inf + |t|inf); SINGLE_TOLERANCE is 8 x the worst seen with seed 0."""
    n = 20000
    rng = np.random.default_rng(seed)
    m = _random_rigid(rng, n)
    p = rng.normal(size=(n, 3)); p /= np.abs(p).max(1, keepdims=True); p *= 10.0 ** rng.uniform(-3, 3, (n, 1))
    assert D.rigid(m).all() and np.bincount(D.shepperd_branch(m), minlength=4).min() > n // 20
    b, w = S.single(np.arange(n))
    got = D.skin_vertices(p, b, w, m)
    L = np.longdouble
    want = (m[:, :, :3].astype(L) * p.astype(L)[:, None, :]).sum(2) + m[:, :, 3].astype(L)
    err = float((np.abs(got.astype(L) - want).max(1) / (np.abs(p).max(1) + np.abs(m[:, :, 3]).max(1))).max())
    print("\n[skin_dq] single influence, seed %d: worst relative error %.3e (tolerance %.3e)" % (seed, err, SINGLE_TOLERANCE))
    assert EPS / 4 < err <= SINGLE_TOLERANCE
    # unit rest normals come out unit within 4 ulp
    nrm = D.skin_normals(p / np.linalg.norm(p, axis=1, keepdims=True), b, w, m)
    assert np.abs(np.sqrt((nrm * nrm).sum(1)) - 1.0).max() <= 4 * EPS


def test_restatement_four_influences_and_the_degenerate_record(pkg):
    s = K.scene(pkg); vb, vw, nb, nw = _four(pkg); sphere = K.parts(pkg)[0]
    q = D.dualquats(FOUR)
    assert D.rigid(FOUR).all()
    ws = D.signed_weights(vb, vw, q)
    assert (ws[sphere] < 0.0).sum() > 100 and np.array_equal(np.abs(ws), vw)  # the antipodal rule fires on the device's side, often
    n2 = D.norm2(D.blend(vb, vw, q))
    last = s.vertex.shape[0] - 1
    # the constructed degenerate record: the pivot (weight 0) is the identity, the three half turns have w = 0 exactly, so no sign is turned
    assert np.array_equal(q[5:, 0], np.zeros(3)) and ws[last].tolist() == vw[last].tolist() and n2[last] < 2.0 ** -8 and n2[last] < 1e-28
    assert D.regular(np.delete(n2, last)).all() and np.delete(n2, last)[sphere[:-1]].min() > 0.05   # nothing else comes near the floor of 1/256
    v, n = _ref(pkg, FOUR, _four(pkg))
    assert np.array_equal(bits(v[last]), bits(s.vertex[last])) and np.array_equal(bits(n[last]), bits(s.normal[last]))   # the rest record, bit for bit
    long = s.normal.copy(); long[last] *= 2.0                                # ... its normal copied, NOT normalised
    assert np.array_equal(bits(D.skin_normals(long, nb, nw, FOUR)[last]), bits(long[last])) and abs(np.linalg.norm(long[last]) - 2.0) < 1e-15
    moved = sphere.copy(); moved[last] = False
    assert v[moved].min() > 0.01 and v[moved].max() < 0.99 and np.abs(v[moved] - s.vertex[moved]).max(1).min() > 0
    assert np.abs(np.sqrt((n * n).sum(1))[moved] - 1.0).max() <= 4 * EPS
    # two bones can never be degenerate: n2 >= w0^2 + w1^2 >= 1/2
    rng = np.random.default_rng(3); m = _random_rigid(rng, 2000); w = rng.uniform(0, 1, 1000)
    b = np.stack([np.arange(1000), 1000 + np.arange(1000), np.zeros(1000, int), np.zeros(1000, int)], 1)
    assert D.norm2(D.blend(b, np.stack([w, 1.0 - w, 0 * w, 0 * w], 1), D.dualquats(m))).min() >= 0.5 - 4 * EPS


def test_restatement_refusals(pkg):
    s = K.scene(pkg); vb, vw, nb, nw = K.bend(pkg)
    radius = S.bone_radius(s.vertex, vb, vw, T.used_vertices(s), N_BONES)
    assert radius[3] == 0.0 and radius[1] > 0 and radius[2] > 0
    for m in (BEND, BEND2, TWIST, _mats()):
        assert D.accepts_dq(m, radius) and S.accepts(_mats(third=T.identity(1)[0]), radius)
    assert D.accepts_dq(FOUR, np.ones(N_FOUR))
    for bad in (M_SCALED, M_MIRRORED, M_SHEARED):                            # linear blending takes them, the dual-quaternion mode does not
        assert S.accepts(_mats(high=bad, third=T.identity(1)[0]), radius) and not D.accepts_dq(_mats(high=bad), radius)
        assert not D.accepts_dq(_mats(third=bad), radius)                    # ... nor on a bone without members
    r32 = T.rotation((3, -1, 2), 77.0).astype(np.float32).astype(np.float64)  # a rotation built in fp32: off the identity by ~1e-7, accepted
    off = np.abs(D.gram(T.about(r32, CENTRE)) - [1, 0, 0, 1, 0, 1]).max()
    assert 1e-9 < off < 1e-6 and D.accepts_dq(_mats(high=clean(T.about(r32, CENTRE))), radius)
    for scale, ok in ((1.0 + 4.9e-7, True), (1.0 + 5.1e-7, False), (1.0 - 4.9e-7, True), (1.0 - 5.1e-7, False)):   # |A^T A - I| <= 1e-6
        assert D.accepts_dq(_mats(high=clean(T.about(T.rotation((0, 0, 1), 25.0) * scale, CENTRE))), radius) == ok, scale
    assert S.accepts(_mats(third=clean(T.about(np.diag([1e6, 2.0, 3.0]), (5, 5, 5), (1e17, 0, 0)))), radius)   # test_skin's far bone: linear only
    assert not D.accepts_dq(_mats(third=clean(T.about(np.diag([1e6, 2.0, 3.0]), (5, 5, 5), (1e17, 0, 0)))), radius)
    # the reach (1 + 2^-16) (2 R_b + 16 |t|_1): just under and just over 1e18, on a bone with members and on the one without
    for b in (2, 3):
        limit = (1e18 / D.SLACK - 2.0 * radius[b]) / 16.0
        for factor, ok in ((1.0 - 2.0 ** -40, True), (1.0 + 2.0 ** -40, False)):
            m = _mats(); m[b, 0, 3] = limit * factor
            assert D.accepts_dq(m, radius) == ok, (b, factor)
            m = _mats(); m[b, :, 3] = (-limit * factor / 2, limit * factor / 4, -limit * factor / 4)
            assert D.accepts_dq(m, radius) == ok, (b, factor)
    for bad in (np.nan, np.inf):
        m = _mats(); m[2, 1, 2] = bad
        assert not D.accepts_dq(m, radius)
        m = _mats(); m[2, 1, 3] = bad
        assert not D.accepts_dq(m, radius)
    assert not D.accepts_dq(T.identity(N_BONES - 1), radius)
    # with a morph in the same call E stands for every R_b: the bone without members is then held to it too
    assert D.accepts_dq(_mats(), np.full(N_BONES, 1e16)) and not D.accepts_dq(_mats(), np.full(N_BONES, 2e17))


def _host_check_cases():
    """(matrices, radii): every Shepperd branch, exact ties between the candidates, half turns about each axis, quaternions whose w comes out
    negative before the sign rule, translations up to 1e17, reaches at the limit, and bones that are not rigid."""
    rng = np.random.default_rng(5)
    rot = _random_rigid(rng, 600)
    rot[:, :, 3] *= 10.0 ** rng.integers(-3, 15, (600, 1))
    quarter_x = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])            # trace = a00 = 1: the trace wins
    ties = [np.eye(3), quarter_x, _half_turn((np.sqrt(0.5), np.sqrt(0.5), 0.0)), _half_turn((0.0, np.sqrt(0.5), np.sqrt(0.5))), _half_turn((np.sqrt(0.5), 0.0, np.sqrt(0.5))),
            np.array([[0.0, 0, 1.0], [1.0, 0, 0], [0, 1.0, 0]]),              # 120 degrees about (1, 1, 1): trace = a00 = a11 = a22 = 0
            np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])]
    for axis in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3), (-3, 1, 1)):
        for deg in (179.0, 180.0, 181.0, 270.0, 359.0, -120.0):
            ties.append(T.rotation(axis, deg))
    special = np.stack([np.concatenate([r, [[1e17], [-3e16], [0.25]]], 1) for r in ties])
    near = np.stack([clean(T.about(T.rotation((0, 0, 1), 25.0) * sc, CENTRE)) for sc in (1.0 + 4.9e-7, 1.0 + 5.1e-7, 1.0 - 4.9e-7, 1.0 - 5.1e-7)])
    loose = np.stack([M_SCALED, M_MIRRORED, M_SHEARED, np.zeros((3, 4)), T.identity(1)[0] * 1e160])
    edge = T.identity(2); limit = (1e18 / D.SLACK - 1.6) / 16.0
    edge[0, 0, 3] = limit * (1.0 - 2.0 ** -40); edge[1, 0, 3] = limit * (1.0 + 2.0 ** -40)
    m = np.concatenate([special, rot, near, loose, edge])
    radius = np.concatenate([np.full(len(special), 0.8), rng.uniform(0.0, 2.0, len(rot)), np.full(len(near) + len(loose) + len(edge), 0.8)])
    return m, radius, len(special), len(edge)


@K.needs_hipcc
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_dual_quaternions_rigid_check_and_reach_are_the_restatement_bit_for_bit(tmp_path, sanitized):
    """The host half of the feature -- sk_bone_dualquat, sk_bone_gram, sk_bone_rigid and sk_dq_reach of csrc/skin.hip, what mcpt_update_skin
    validates and stages with -- built into the stand-alone program tests/skin_dq_host_check.cpp (no device is touched) against
    tests/skin_dq_ref.py: the same bits.  `sanitized`: the same program under the host's address and undefined-behaviour sanitizers, which must
    stay silent."""
    exe = K.build_host_check("skin_dq_host_check", ["skin.hip", "transform.hip"], tmp_path, sanitized)
    m, radius, n_special, n_edge = _host_check_cases()
    np.concatenate([m.reshape(-1, 12), radius[:, None]], 1).tofile(str(tmp_path / "in.bin"))
    K.run_host_check(exe, tmp_path, sanitized)
    got = np.fromfile(str(tmp_path / "out.bin")).reshape(-1, 16)
    with np.errstate(all="ignore"):
        is_rigid = D.rigid(m)
        assert np.array_equal(bits(got[:, 8:14]), bits(D.gram(m)))
        assert np.array_equal(got[:, 14], is_rigid.astype(np.float64))
        assert np.array_equal(bits(got[:, 15]), bits(D.reach(m, radius)))
        q = D.dualquats(m)
    assert np.array_equal(bits(got[is_rigid, :8]), bits(q[is_rigid]))        # (a bone that is not rigid is refused before it is converted)
    # the inputs are what the docstring says
    branch = D.shepperd_branch(m[is_rigid]); raw = D.raw_quaternion(m[is_rigid])
    assert np.bincount(branch, minlength=4).min() >= 30 and (raw[:, 0] < 0).sum() >= 30 and (q[is_rigid, 0] >= 0).all()
    assert is_rigid[:n_special].all() and D.shepperd_branch(m[:6]).tolist() == [0, 0, 1, 2, 1, 0]
    assert np.array_equal(q[6:9, :4], [[0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])
    assert np.abs(m[is_rigid][:, :, 3]).max() == 1e17 and is_rigid[-n_edge - 9:].tolist() == [True, False, True, False] + [False] * 5 + [True] * 2
    assert D.reach(m, radius)[-2] <= 1e18 < D.reach(m, radius)[-1]


# ------------------------------------------------------------------------------------------------------------------------ GPU helpers
DQ = lambda pkg: pkg.SKIN_DUAL_QUATERNION


def _pair(pkg, extra=0, skin="bend", small=False, mode_first=True):
    """The context under test, in dual-quaternion mode (with the five-bone bend, or `skin` = (records..., n_bones), or none), and its oracle."""
    def setup(R):
        if mode_first:
            R.set_skin_mode(DQ(pkg))
        if skin is not None:
            R.set_vertex_skin(*(K.bend(pkg, small) + (N_BONES,) if skin == "bend" else skin))
        if not mode_first:
            R.set_skin_mode(DQ(pkg))

    R, O = K.pair(pkg, setup, extra=extra, max_depth=8, scene=K.scene(pkg, small))
    assert R.skin_mode() == DQ(pkg) and O.skin_mode() == pkg.SKIN_LINEAR
    return R, O


def _check_against_oracle(pkg, R, O, matrices, skin=None, rest=None, small=False, film=True):
    v, n = _ref(pkg, matrices, skin, rest, small)
    R.update_skin(matrices); O.update_vertices(v, n)
    a, b = K.state(pkg, R, film, arrays=True), K.state(pkg, O, film, arrays=True)
    assert np.array_equal(bits(a["vertex"]), bits(v)) and np.array_equal(bits(a["normal"]), bits(n))   # probe_vertices: the restated arrays
    K.assert_same(a, b)
    return a


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("gpu_tree", [False, True])
@pytest.mark.parametrize("small", [False, True])
def test_bend_and_twist_of_the_sphere_with_a_moved_lamp(pkg, gpu_tree, small):
    R, O = _pair(pkg, extra=pkg.FLAG_GPU_BVH_BUILD if gpu_tree else 0, small=small, mode_first=gpu_tree)
    s = K.scene(pkg, small); sphere, lamp = K.parts(pkg, small)
    assert s.vertex.shape[0] == s.normal.shape[0] == (349 if small else 1249)
    rest = K.state(pkg, R, film=False, arrays=True)
    before = R.probe_lights()
    for k, m in enumerate((BEND, TWIST)):
        v, _ = _ref(pkg, m, small=small)
        assert v[sphere].min() > 0.01 and v[sphere].max() < 0.99 and not np.array_equal(v[sphere], s.vertex[sphere])   # moved, inside the room
        assert np.array_equal(v[~sphere & ~lamp], s.vertex[~sphere & ~lamp])                                         # the walls stay
        moved = _check_against_oracle(pkg, R, O, m, small=small)
        assert not np.array_equal(rest["t"], moved["t"])
        assert np.array_equal(before[0], moved["light_face"]) and not np.array_equal(before[2], moved["light_pos"])
        want = (v[s.face[moved["light_face"], :, 0]] - np.array(list(R.info().centre))).reshape(-1, 9)   # the nine fp64 positions per light
        assert np.array_equal(bits(want), bits(moved["light_pos"]))
        info = R.update_info(); si = R.skin_info()
        assert info.updates == k + 1 and info.last_update_ms > 0 and (si.n_bones, si.updates) == (N_BONES, k + 1) and 0 < si.last_ms <= info.last_update_ms
    # the twist: every ring of the sphere keeps its radius about the axis (linear blending takes the waist to 0.087 of it)
    axis = CENTRE[[0, 2]]
    ring = lambda a: np.hypot(*(a[sphere][:, [0, 2]] - axis).T)
    r0, r1 = ring(s.vertex), ring(moved["vertex"])
    lbs = ring(S.skin_vertices(s.vertex, *K.bend(pkg, small)[:2], TWIST))
    assert np.abs(r1 - r0).max() <= 1e-12 and (lbs / np.maximum(r0, 1e-300))[r0 > 0.1].min() < 0.1
    # ... and the half turn, which linear blending collapses onto the axis, comes out at full radius on the device
    half = _mats(low=M_LIFT, high=clean(T.about(T.rotation((0, 1, 0), 180.0), CENTRE, (0.0, 0.05, 0.0))), lamp=M_LAMP)
    R.update_skin(half)
    assert np.abs(ring(R.vertices()[0]) - r0).max() <= 1e-12
    assert (ring(S.skin_vertices(s.vertex, *K.bend(pkg, small)[:2], half)) / np.maximum(r0, 1e-300))[r0 > 0.1].min() < 1e-14
    R.validate_trees()
    R.close(); O.close()


@pytest.mark.gpu
def test_four_influences_zero_weight_slots_the_antipodal_rule_and_the_degenerate_record(pkg):
    skin = _four(pkg)
    s = K.scene(pkg); last = s.vertex.shape[0] - 1
    long = s.normal.copy(); long[last] *= 2.0                                # the degenerate record's rest normal is not of unit length: it must come back as it is
    R, O = _pair(pkg, skin=None)
    R.update_vertices(s.vertex, long); O.update_vertices(s.vertex, long)
    R.set_vertex_skin(*skin, N_FOUR)
    moved = _check_against_oracle(pkg, R, O, FOUR, skin, (s.vertex, long))
    assert np.array_equal(bits(moved["vertex"][last]), bits(s.vertex[last])) and np.array_equal(bits(moved["normal"][last]), bits(long[last]))
    assert not np.array_equal(moved["vertex"][last - 1], s.vertex[last - 1])
    R.close(); O.close()


@pytest.mark.gpu
def test_identity_bones_leave_the_scene_as_it_was(pkg):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    R, O = _pair(pkg, skin=None)
    rest = K.unit_rest(pkg)
    R.update_vertices(*rest); O.update_vertices(*rest)                       # unit-length normals: see deform_kit.unit_rest
    before = K.state(pkg, R, arrays=True)
    rng = np.random.default_rng(8)
    vb = rng.integers(0, 3, (nv, 4)); nb = rng.integers(0, 3, (nn, 4))         # dyadic weights on any mix of identity bones: the identity exactly
    skin = (vb, np.tile(DYADIC, (nv, 1)), nb, np.tile(DYADIC, (nn, 1)))
    R.set_vertex_skin(*skin, 3)
    K.assert_same(before, K.state(pkg, R, arrays=True))                      # setting a skin moves nothing
    after = _check_against_oracle(pkg, R, O, T.identity(3), skin, rest)
    assert np.array_equal(after["vertex"], before["vertex"])                 # by value: a -0 may become +0
    # (the normals went through v / |v| once more: the same fp32 numbers, as test_restatement_identity_bones_give_the_rest_pose shows)
    assert np.array_equal(after["normal"].astype(np.float32), before["normal"].astype(np.float32))
    for k in before:
        if k not in ("vertex", "normal"):
            assert np.array_equal(bits(before[k]), bits(after[k])), k        # traces, shading normals, lights and film: as they were
    R.close(); O.close()


@pytest.mark.gpu
def test_single_influence_is_update_transforms_within_the_measured_tolerance(pkg):
    s = K.scene(pkg)
    R, X = _pair(pkg, skin=None)
    vg, ng = pkg.groups_from_faces(s, np.where(s.face[:, 0, 3] == SPHERE, 1, np.where(s.face[:, 0, 3] == LAMP, 2, 0)))
    X.set_vertex_groups(vg, ng, 3)
    R.set_vertex_skin(*S.single(vg), *S.single(ng), 3)
    m = np.stack([T.identity(1)[0], M_THIRD, M_LAMP])
    R.update_skin(m); X.update_transforms(m)
    (v, n), (xv, xn) = R.vertices(), X.vertices()
    scale = np.abs(s.vertex).max(1) + np.abs(m[vg][:, :, 3]).max(1)
    err = np.abs(v - xv).max(1)
    print("\n[skin_dq] single influence on the device against update_transforms: worst relative difference %.3e (tolerance %.3e)" % (
        (err[scale > 0] / scale[scale > 0]).max(), SINGLE_TOLERANCE))
    assert (err <= SINGLE_TOLERANCE * scale).all() and not np.array_equal(v, s.vertex)   # (the room's corners at the origin: scale 0, error 0)
    assert np.abs(n - xn).max() <= SINGLE_TOLERANCE * 2                       # unit vectors: |n|inf + 0 <= 1 on either side
    R.validate_trees()
    R.close(); X.close()


@pytest.mark.gpu
def test_mode_state_device_bytes_and_back_to_linear(pkg):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    R, O = _pair(pkg, skin=None)                                             # the mode first, no skin yet: nothing is allocated
    L = pkg.Renderer(s, max_depth=8, flags=FLAGS(pkg))                       # a context that never leaves linear mode
    base = O.info().device_bytes                                             # (O goes through the same probes and renders as R: what those allocate is in both)
    assert R.info().device_bytes == base and R.skin_info().n_bones == 0
    per_record = 24 + 16 + 32                                                # rest pose, ids, weights
    linear = per_record * (nv + nn) + 96 * N_BONES
    R.set_vertex_skin(*K.bend(pkg), N_BONES); L.set_vertex_skin(*K.bend(pkg), N_BONES)
    assert R.info().device_bytes - O.info().device_bytes == linear + 64 * N_BONES and L.info().device_bytes - base == linear and R.skin_mode() == DQ(pkg)
    R.set_vertex_skin(*K.bend(pkg), N_BONES + 4)                             # another n_bones: the mode stays, the table is resized
    assert R.info().device_bytes - O.info().device_bytes == linear + 96 * 4 + 64 * (N_BONES + 4) and R.skin_mode() == DQ(pkg) and R.skin_info().n_bones == N_BONES + 4
    more = T.identity(N_BONES + 4); more[:N_BONES] = BEND
    _check_against_oracle(pkg, R, O, more, film=False)
    R.set_vertex_skin(*_four(pkg), N_FOUR)                                   # (takes the bent scene as its rest pose; replaced again below)
    assert R.info().device_bytes - O.info().device_bytes == per_record * (nv + nn) + (96 + 64) * N_FOUR
    R.update_vertices(s.vertex, s.normal); O.update_vertices(s.vertex, s.normal)
    R.set_vertex_skin(*K.bend(pkg), N_BONES)
    assert R.info().device_bytes - O.info().device_bytes == linear + 64 * N_BONES
    R.set_skin_mode(DQ(pkg))                                                 # the mode it has: nothing changes
    assert R.info().device_bytes - O.info().device_bytes == linear + 64 * N_BONES
    dq = _check_against_oracle(pkg, R, O, BEND)
    # LINEAR -> DQ -> LINEAR: §18's arrays bit for bit, and device_bytes is back
    R.set_skin_mode(pkg.SKIN_LINEAR)
    assert R.skin_mode() == pkg.SKIN_LINEAR and R.info().device_bytes - O.info().device_bytes == linear
    K.assert_same(K.state(pkg, R, film=False, arrays=True), {k: v for k, v in dq.items() if k != "film"})   # changing the mode moves nothing
    R.update_skin(BEND); L.update_skin(BEND)
    lin = K.state(pkg, R, arrays=True)
    K.assert_same(lin, K.state(pkg, L, arrays=True))
    assert np.array_equal(bits(lin["vertex"]), bits(S.skin_vertices(s.vertex, *K.bend(pkg)[:2], BEND))) and not np.array_equal(lin["vertex"], dq["vertex"])
    R.update_skin(_mats(high=M_SCALED)); L.update_skin(_mats(high=M_SCALED))  # a scaled bone is linear mode's to take again
    K.assert_same(K.state(pkg, R, film=False, arrays=True), K.state(pkg, L, film=False, arrays=True))
    R.set_skin_mode(DQ(pkg))                                                 # the mode AFTER the skin: the table comes with it
    assert R.info().device_bytes - O.info().device_bytes == linear + 64 * N_BONES
    _check_against_oracle(pkg, R, O, BEND2, film=False)
    assert R.skin_info().updates == 5 and R.update_info().updates == 6
    R.close(); O.close(); L.close()


@pytest.mark.gpu
def test_bones_are_not_cumulative(pkg):
    R, O = _pair(pkg, skin=None)
    rest = K.unit_rest(pkg)
    R.update_vertices(*rest); O.update_vertices(*rest)                       # unit-length normals: see deform_kit.unit_rest
    R.set_vertex_skin(*K.bend(pkg), N_BONES)
    original = K.state(pkg, R, arrays=True)
    R.update_skin(BEND)
    moved = _check_against_oracle(pkg, R, O, BEND2, rest=rest)               # M1 then M2 = M2 alone (the lamp is back, too)
    assert not np.array_equal(moved["film"], original["film"])
    R.update_skin(BEND2)                                                     # the same bones twice: the same scene
    K.assert_same(K.state(pkg, R, arrays=True), moved)
    back = _check_against_oracle(pkg, R, O, _mats(), rest=rest)              # M then identity: what the restatement says ...
    for k in original:
        if k not in ("vertex", "normal"):
            assert np.array_equal(bits(original[k]), bits(back[k])), k       # ... which is the original film, traces, shading normals and lights
    assert np.array_equal(original["vertex"], back["vertex"])
    assert R.skin_info().updates == 4 and R.update_info().updates == 5 and O.update_info().updates == 3
    R.close(); O.close()


@functools.lru_cache(maxsize=None)
def _targets(pkg):
    """Two morph targets over the sphere: a swell about its centre with normal deltas of its own, and a sparse lift of the cap."""
    s = K.scene(pkg); sphere = K.parts(pkg)[0]
    rng = np.random.default_rng(31)
    si = np.flatnonzero(sphere); cap = si[s.vertex[si, 1] > 0.45]
    vt = [(si, s.vertex[si] - CENTRE), (cap, np.tile((0.0, 0.05, 0.0), (len(cap), 1)))]
    nt = [(si, rng.uniform(-0.3, 0.3, (len(si), 3))), (cap, rng.uniform(-0.3, 0.3, (len(cap), 3)))]
    return vt, nt


@pytest.mark.gpu
def test_morph_then_skin_in_dual_quaternion_mode(pkg):
    s = K.scene(pkg); vb, vw, nb, nw = K.bend(pkg)
    R, O = _pair(pkg)
    vt, nt = _targets(pkg)
    R.set_vertex_morph(vt, nt)
    weights = np.array([-0.2, 0.7])
    mv, mn = M.morph_vertices(s.vertex, vt, weights), M.morph_normals(s.normal, nt, weights)
    for bones in (TWIST, BEND):
        v, n = D.skin_vertices(mv, vb, vw, bones), D.skin_normals(mn, nb, nw, bones)
        assert v[K.parts(pkg)[0]].min() > 0.01 and v[K.parts(pkg)[0]].max() < 0.99
        R.update_morph(weights, bones); O.update_vertices(v, n)
        a = K.state(pkg, R, arrays=True)
        assert np.array_equal(bits(a["vertex"]), bits(v)) and np.array_equal(bits(a["normal"]), bits(n))
        K.assert_same(a, K.state(pkg, O, arrays=True))
    lv, ln = M.morph_then_skin(s.vertex, s.normal, vt, nt, weights, K.bend(pkg), TWIST)
    assert not np.array_equal(lv, D.skin_vertices(mv, vb, vw, TWIST))        # (the linear route gives other arrays)
    cam = pkg.scenes.Camera((0.62, 0.55, 2.25), (0.5, 0.45, 0.0), (0.0, 1.0, 0.0), 40.0, W, H)
    opts = dict(feature_spp=4, feature_seed=3, max_history=16.0)
    v, n = D.skin_vertices(mv, vb, vw, BEND2), D.skin_normals(mn, nb, nw, BEND2)
    for r in (R, O):
        r.clear(); r.render(8, seed=5)
    R.update_morph_reproject(weights, BEND2, camera=cam, **opts); O.update_vertices_reproject(v, n, camera=cam, **opts)
    assert np.array_equal(bits(R.read_accum()), bits(O.read_accum()))
    K.assert_same(K.state(pkg, R, film=False, arrays=True), K.state(pkg, O, film=False, arrays=True))
    # the reach bound with E in R_b's place, on the bone without members too; a bone that is not rigid is refused here as well
    used = T.used_vertices(s)
    e = M.reach(M.rest_radius(s.vertex, used), weights, M.target_delta(vt, used))
    far = _mats(); far[3, 0, 3] = (1e18 / D.SLACK - 2.0 * e) / 16.0 * (1.0 + 2.0 ** -40)
    near = _mats(); near[3, 0, 3] = (1e18 / D.SLACK - 2.0 * e) / 16.0 * (1.0 - 2.0 ** -40)
    assert D.accepts_dq(near, np.full(N_BONES, e)) and not D.accepts_dq(far, np.full(N_BONES, e))
    updates = R.update_info().updates
    for bad in (far, _mats(high=M_SCALED)):
        for call in (lambda: R.update_morph(weights, bad), lambda: R.update_morph_reproject(weights, bad)):
            with pytest.raises(pkg.McptError) as err:
                call()
            assert "status %d" % INVALID in str(err.value)
    assert R.update_info().updates == updates and (R.skin_info().updates, R.morph_info().updates) == (3, 3)
    R.update_morph(weights, near)
    R.close(); O.close()


@pytest.mark.gpu
def test_groups_and_skin_on_one_context(pkg):
    s = K.scene(pkg)
    R, O = _pair(pkg, skin=None)
    vg, ng = pkg.groups_from_faces(s, np.where(s.face[:, 0, 3] == SPHERE, 1, np.where(s.face[:, 0, 3] == LAMP, 2, 0)))
    gm = np.stack([T.identity(1)[0], clean(T.about(T.rotation((0, 1, 0), 15.0), CENTRE, (0.05, 0.0, 0.05))), M_LAMP])

    def groups_oracle(m):
        O.update_vertices(T.transform_vertices(s.vertex, vg, m), T.transform_normals(s.normal, ng, m))
        K.assert_same(K.state(pkg, R, film=False, arrays=True), K.state(pkg, O, film=False, arrays=True))

    R.set_vertex_groups(vg, ng, 3)                                           # the groups' rest pose: the scene as created
    R.update_transforms(gm); groups_oracle(gm)
    posed = (T.transform_vertices(s.vertex, vg, gm), T.transform_normals(s.normal, ng, gm))
    R.set_vertex_skin(*K.bend(pkg), N_BONES)                                 # the skin's OWN rest pose: the scene as the groups left it
    small = _mats(low=clean(T.about(T.rotation((0, 0, 1), 5.0), CENTRE)), high=clean(T.about(T.rotation((0, 1, 0), -160.0), CENTRE, (0.0, 0.04, 0.0))))
    _check_against_oracle(pkg, R, O, small, rest=posed)
    R.update_transforms(gm); groups_oracle(gm)                               # each call overwrites the other's result and reads its own rest pose
    assert R.transform_info().updates == 2 and R.skin_info().updates == 1 and R.update_info().updates == 3
    R.close(); O.close()


@pytest.mark.gpu
def test_auto_normals_follow_the_dual_quaternion_route(pkg):
    s = K.scene(pkg); sphere = K.parts(pkg)[0]
    R, O = _pair(pkg)
    mask = np.zeros(s.normal.shape[0], np.uint8); mask[np.unique(s.face[s.face[:, 0, 3] == SPHERE][:, :, 1])] = 1
    R.set_auto_normals(mask)
    offset, entry = NR.per_record(s.face, s.normal.shape[0], s.vertex, s.normal, mask)
    for m in (TWIST, BEND):
        v, n = _ref(pkg, m)
        n = NR.apply(offset, entry, v, n)                                    # the chosen records from the deformed faces, the rest as the kernel wrote them
        R.update_skin(m); O.update_vertices(v, n)
        a = K.state(pkg, R, arrays=True)
        assert np.array_equal(bits(a["vertex"]), bits(v)) and np.array_equal(bits(a["normal"]), bits(n))
        K.assert_same(a, K.state(pkg, O, arrays=True))
    assert R.normals_info().updates == 2 and int(mask.sum()) == int(sphere.sum())
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_camera", [False, True])
def test_reprojection_follows_the_dual_quaternion_skin(pkg, with_camera):
    R, O = _pair(pkg)
    cam = pkg.scenes.Camera((0.62, 0.55, 2.25), (0.5, 0.45, 0.0), (0.0, 1.0, 0.0), 40.0, W, H) if with_camera else None
    m = _mats(low=clean(T.about(T.rotation((0, 0, 1), 3.0), CENTRE)), high=clean(T.about(T.rotation((0, 1, 0), -20.0), CENTRE, (0.02, 0.02, 0.0))))
    v, n = _ref(pkg, m)
    opts = dict(feature_spp=4, feature_seed=3, max_history=16.0)
    for r in (R, O):
        r.clear(); r.render(8, seed=5)
    R.update_skin_reproject(m, camera=cam, **opts)
    O.update_vertices_reproject(v, n, camera=cam, **opts)
    assert np.array_equal(bits(R.read_accum()), bits(O.read_accum()))
    ia, ib = R.reproject_info(), O.reproject_info()
    assert (ia.reprojections, ia.pixels_reused) == (ib.reprojections, ib.pixels_reused) == (1, ib.pixels_reused) and ia.pixels_reused > 0.5 * W * H
    assert np.array_equal(bits(R.features()), bits(O.features()))          # the context holds the new scene's features
    assert R.update_info().updates == 1 and R.skin_info().updates == 1
    K.assert_same(K.state(pkg, R, film=False, arrays=True), K.state(pkg, O, film=False, arrays=True))
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["own", "side"])
def test_update_between_renders_without_a_sync(pkg, which):
    import torch
    R, O = _pair(pkg)
    O.set_skin_mode(DQ(pkg)); O.set_vertex_skin(*K.bend(pkg), N_BONES)
    if which == "side":
        stream = torch.cuda.Stream()
        R.set_torch_stream(stream)
    R.clear()
    R.render(4, seed=9, first_sample=0); R.update_skin(TWIST); R.render(4, seed=9, first_sample=4)   # nothing in between
    R.update_skin(BEND2); R.update_skin(BEND)                                # back-to-back calls through the one stage keep their order
    R.render(2, seed=9, first_sample=8)
    got = R.read_accum()
    O.clear()
    O.render(4, seed=9, first_sample=0); O.sync(); O.update_skin(TWIST); O.sync(); O.render(4, seed=9, first_sample=4); O.sync()
    O.update_skin(BEND2); O.sync(); O.update_skin(BEND); O.sync()
    O.render(2, seed=9, first_sample=8); O.sync()
    assert np.array_equal(bits(got), bits(O.read_accum())) and np.all(got[..., 3] == 10)
    v, n = _ref(pkg, BEND)
    assert np.array_equal(bits(R.vertices()[0]), bits(v)) and np.array_equal(bits(R.vertices()[1]), bits(n))
    if which == "side":
        R.set_stream(0)
    R.close(); O.close()


@pytest.mark.gpu
def test_clone_rebuild_and_bookkeeping(pkg):
    R, O = _pair(pkg)
    R.update_skin(TWIST)
    clone = R.clone()
    assert clone.skin_mode() == DQ(pkg) and clone.info().device_bytes == R.info().device_bytes
    si = clone.skin_info()
    assert (si.n_bones, si.updates) == (N_BONES, 0)
    K.assert_same(K.state(pkg, clone, arrays=True), K.state(pkg, R, arrays=True))   # the clone is the twisted scene ...
    _check_against_oracle(pkg, clone, O, BEND2)                              # ... with the ORIGINAL rest pose, the skin, the mode and the table
    with pytest.raises(pkg.McptError):
        clone.update_skin(_mats(high=M_SCALED))                              # (the mode travelled: a scaled bone is refused)
    plain = pkg.Renderer(K.scene(pkg), max_depth=8, flags=FLAGS(pkg)); plain.set_skin_mode(DQ(pkg))
    c2 = plain.clone()                                                       # the mode travels without a skin, too
    assert c2.skin_mode() == DQ(pkg) and c2.info().device_bytes == plain.info().device_bytes
    c2.close(); plain.close()
    v, n = _ref(pkg, TWIST)
    O.update_vertices(v, n)
    K.assert_same(K.state(pkg, R, arrays=True), K.state(pkg, O, arrays=True))   # the source did not move with its clone
    for builder in (pkg.REBUILD_HOST, pkg.REBUILD_DEVICE):                   # a rebuild keeps mode, table, skin and rest pose
        R.rebuild(builder); O.rebuild(builder)
        assert R.skin_mode() == DQ(pkg) and R.skin_info().n_bones == N_BONES
        K.assert_same(K.state(pkg, R, film=False, arrays=True), K.state(pkg, O, film=False, arrays=True))
        _check_against_oracle(pkg, R, O, BEND if builder == pkg.REBUILD_HOST else TWIST)
    R.update_skin(_mats()); R.update_skin_reproject(_mats())
    si = R.skin_info()
    assert (si.n_bones, si.updates) == (N_BONES, 5) and si.last_ms > 0 and R.update_info().updates == 5
    assert clone.skin_info().updates == 1 and clone.update_info().updates == 1
    assert R.update_info().last_update_ms >= si.last_ms                      # the refit's bracket spans the table's copy and the skinning kernels
    clone.close(); R.close(); O.close()


@pytest.mark.gpu
def test_skin_mode_and_dual_quaternion_refusals(pkg):
    s = K.scene(pkg); vb, vw, nb, nw = K.bend(pkg)
    plain = pkg.Renderer(s, max_depth=8, flags=pkg.FLAG_DETERMINISTIC)
    for mode in (pkg.SKIN_DUAL_QUATERNION, pkg.SKIN_LINEAR, 7):
        with pytest.raises(pkg.McptError) as e:
            plain.set_skin_mode(mode)
        assert "status %d" % UNSUPPORTED in str(e.value)
    assert plain.skin_mode() == pkg.SKIN_LINEAR and plain.lib.mcpt_get_skin_mode(plain.ctx, None) == INVALID
    plain.close()
    R = pkg.Renderer(s, max_depth=8, flags=FLAGS(pkg))
    o, d = K.rays(pkg)
    film = render_film(R, 4, 5); trace = R.probe_trace4(o, d); arrays = R.vertices()
    expect = {"n_bones": 0, "mode": pkg.SKIN_LINEAR, "bytes": R.info().device_bytes}

    def unchanged():
        si = R.skin_info()
        assert R.update_info().updates == 0 and (si.n_bones, si.updates) == (expect["n_bones"], 0) and R.reproject_info().reprojections == 0
        assert R.skin_mode() == expect["mode"] and R.info().device_bytes == expect["bytes"]
        assert np.array_equal(bits(render_film(R, 4, 5)), bits(film))
        for x, y in zip(tuple(trace) + tuple(arrays), tuple(R.probe_trace4(o, d)) + tuple(R.vertices())):
            assert np.array_equal(bits(x), bits(y))

    def refused(call, status=INVALID):
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % status in str(e.value)
        unchanged()
        return str(e.value)

    for mode in (2, 7, 0xFFFFFFFF):                                          # an unknown mode, in either mode
        refused(lambda: R.set_skin_mode(mode))
    assert R.lib.mcpt_get_skin_mode(R.ctx, None) == INVALID
    R.set_skin_mode(DQ(pkg)); expect["mode"] = DQ(pkg)
    unchanged()
    refused(lambda: R.set_skin_mode(2))
    assert "no skin is set" in refused(lambda: R.update_skin(_mats()))       # no skin is set
    refused(lambda: R.update_skin_reproject(_mats()))
    R.set_vertex_skin(vb, vw, nb, nw, N_BONES)
    expect["n_bones"] = N_BONES; expect["bytes"] += (24 + 16 + 32) * (len(vb) + len(nb)) + (96 + 64) * N_BONES
    unchanged()
    radius = S.bone_radius(s.vertex, vb, vw, T.used_vertices(s), N_BONES)
    nan = _mats(); nan[1, 2, 1] = np.nan
    inf = _mats(); inf[2, 0, 3] = np.inf
    flat = _mats(low=T.about(np.diag([1.0, 0.0, 1.0]), CENTRE))               # det A = 0: the check both modes share
    far = _mats(); far[2, 0, 3] = (1e18 / D.SLACK - 2.0 * radius[2]) / 16.0 * (1.0 + 2.0 ** -40)
    edge = _mats(); edge[3, 1, 3] = -(1e18 / D.SLACK) / 16.0 * (1.0 + 2.0 ** -40)   # on the bone without members: R_b = 0
    loose = [_mats(high=M_SCALED), _mats(low=M_MIRRORED), _mats(high=M_SHEARED), _mats(third=M_SCALED),
             _mats(high=clean(T.about(T.rotation((0, 0, 1), 25.0) * (1.0 + 5.1e-7), CENTRE)))]
    for m in [nan, inf, flat, far, edge] + loose:
        assert not D.accepts_dq(m, radius)                                   # the restatement of the validation agrees
        refused(lambda: R.update_skin(m))
        refused(lambda: R.update_skin_reproject(m))
    for m in loose:
        msg = refused(lambda: R.update_skin(m))
        assert "rigid" in msg and "MCPT_SKIN_LINEAR" in msg and "bone %d" % (1 if m is loose[1] else 3 if m is loose[3] else 2) in msg
    refused(lambda: R.update_skin(T.identity(N_BONES - 1)))                  # another n_bones
    refused(lambda: R.update_skin(T.identity(N_BONES + 1)))
    assert R.lib.mcpt_update_skin(R.ctx, None, N_BONES) == INVALID and R.lib.mcpt_update_skin_reproject(R.ctx, None, N_BONES, None, None) == INVALID
    unchanged()
    # the order: the entries before the determinant, the determinant before the rigid rule, the rigid rule before the reach
    both = nan.copy(); both[2] = M_SCALED
    assert "not finite" in refused(lambda: R.update_skin(both))
    both = flat.copy(); both[2] = M_SCALED
    assert "det A" in refused(lambda: R.update_skin(both))
    both = far.copy(); both[1] = M_SHEARED
    assert "rigid" in refused(lambda: R.update_skin(both))
    assert "1e18" in refused(lambda: R.update_skin(far))
    # _reproject: the matrices first, then the camera
    cam = s.camera
    with pytest.raises(pkg.McptError) as e:
        R.update_skin_reproject(loose[0], camera=pkg.scenes.Camera(cam.eye, cam.eye, cam.up, cam.fovy, W, H))
    assert "rigid" in str(e.value)
    refused(lambda: R.update_skin_reproject(BEND, camera=pkg.scenes.Camera(cam.eye, cam.eye, cam.up, cam.fovy, W, H)))
    unchanged()
    near = _mats(); near[2, 0, 3] = (1e18 / D.SLACK - 2.0 * radius[2]) / 16.0 * (1.0 - 2.0 ** -40)
    assert D.accepts_dq(near, radius) and D.accepts_dq(BEND, radius)
    R.validate_trees()
    R.update_skin(BEND)                                                      # and the context still works
    assert R.update_info().updates == 1 and R.skin_info().updates == 1
    R.close()


@pytest.mark.gpu
def test_facade_skin_dq(pkg, tmp_path):
    exe = kit.build_facade("facade_skin_dq.cpp", tmp_path)
    a = pkg.scenes.cornell_box(44, 30, sphere_lon=24, sphere_lat=12)
    obj = a.write(str(tmp_path / "a"))
    vb, vw, nb, nw = K.height_skin(pkg, a, a.face[:, 0, 3] == SPHERE)
    m = np.stack([T.identity(1)[0], M_LOW, M_TWIST])
    vb.astype(np.uint32).tofile(str(tmp_path / "b.bin")); vw.tofile(str(tmp_path / "w.bin")); m.tofile(str(tmp_path / "m.bin"))
    D.skin_vertices(a.vertex, vb, vw, m).tofile(str(tmp_path / "v.bin")); D.skin_normals(a.normal, nb, nw, m).tofile(str(tmp_path / "n.bin"))
    outs = [str(tmp_path / n) for n in ("sk.bin", "upd.bin", "rp.bin")]
    k = 4
    line = kit.run_facade(exe, [obj, str(k)] + [str(tmp_path / n) for n in ("b.bin", "w.bin", "m.bin", "v.bin", "n.bin")] + outs)
    w, h = int(line[0]), int(line[1])
    assert (w, h, int(line[2])) == (44, 30, k)
    sk, upd, rp = [np.fromfile(p, np.float32).reshape(h, w, 4) for p in outs]
    assert np.all(sk[..., 3] == k) and sk[..., :3].sum() > 0                 # the picture started again and ends at k samples
    assert np.array_equal(bits(sk), bits(upd))                             # bones on the device = the restated arrays through update()
    assert np.all(rp[..., 3] >= 1) and np.all(rp[..., 3] <= 5) and (rp[..., 3] > 1).mean() > 0.5   # history capped at 4, plus the new frame


@pytest.mark.gpu
@pytest.mark.parametrize("reproject", [False, True])
def test_cli_bend_dual_quat(pkg, tmp_path, reproject):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    out = str(tmp_path / "img")
    base = [obj, "--turntable", "3", "--spp", "4", "--depth", "5", "--seed", "3", "--deterministic", "--out", out]
    extra = ["--reproject", "8"] if reproject else []
    p = kit.run_cli(base + ["--bend", "glossy", "170", "--dual-quat"] + extra)
    assert p.returncode == 0, p.stderr[-2000:]
    imgs = kit.turntable_frames(out)
    assert imgs[0] != imgs[1] and imgs[1] != imgs[2]
    q = kit.run_cli(base + ["--bend", "glossy", "170"] + extra)              # the same frames by linear blending: the bent ones differ
    assert q.returncode == 0, q.stderr[-2000:]
    lin = kit.turntable_frames(out)
    assert lin[1] != imgs[1] and lin[2] != imgs[2] and (reproject or lin[0] == imgs[0])   # (frame 0 is the rest pose: sin 0 = 0)
    if not reproject:                                                        # clean errors
        for args in (base + ["--dual-quat"], [obj, "--dual-quat"], base + ["--dual-quat", "--swell", "glossy", "0.1"], base + ["--dual-quat", "--spin", "glossy"]):
            q = kit.run_cli(args)
            assert q.returncode == 2 and "--dual-quat" in q.stderr and "--bend" in q.stderr
        q = kit.run_cli(base + ["--bend", "glossy", "25", "--dual-quat", "--swell", "glossy", "0.1", "--auto-normals", "--rebuild-above", "1.0"])
        assert q.returncode == 0, q.stderr[-2000:]


@pytest.mark.gpu
def test_dual_quaternion_update_is_not_slower_on_the_device_than_the_upload_it_replaces(pkg):
    """S-bath detail 160 (0.59 M triangles), the fixtures twisted by two bones: device time (mcpt_update_info::last_update_ms, HIP events:
    everything from the first copy to the end of the refit) of mcpt_update_skin in dual-quaternion mode against mcpt_update_vertices fed the
    identical restated arrays, in the same process, medians of 20 after 3 warm-ups, alternating.  The one claim: the new route's device time is
    not larger.  The figures are in DESIGN.md §21 and profiles/skin_dq_probe.json (tools/skin_dq_probe.py)."""
    scene = pkg.scenes.bathroom_stress(64, 36, detail=160, tex_size=16)
    part = np.isin(scene.face[:, 0, 3], (5, 6))
    vb, vw, nb, nw = K.height_skin(pkg, scene, part)
    pivot = scene.vertex[np.unique(scene.face[part][:, :, 0])].mean(0)
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    R.set_vertex_skin(vb, vw, nb, nw, 3)
    R.set_skin_mode(DQ(pkg))
    sk, up = [], []
    for i in range(23):
        m = np.stack([T.identity(1)[0], T.identity(1)[0], T.about(T.rotation((0, 1, 0), 7.0 * (i + 1)), pivot)])
        v, n = D.skin_vertices(scene.vertex, vb, vw, m), D.skin_normals(scene.normal, nb, nw, m)
        R.update_skin(m); sk.append(R.update_info().last_update_ms)
        R.update_vertices(v, n); up.append(R.update_info().last_update_ms)
    R.validate_trees()
    R.close()
    a, b = float(np.median(sk[3:])), float(np.median(up[3:]))
    print("\n[skin_dq] %d vertices + %d normals: update_skin (dual quaternions) %.3f ms, update_vertices %.3f ms on the device (medians of 20), ratio %.3f" % (
        scene.vertex.shape[0], scene.normal.shape[0], a, b, a / b))
    assert 0 < a <= b
