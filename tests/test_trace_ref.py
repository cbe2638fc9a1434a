"""CPU only: tests/trace_ref.py itself -- the measurement of its K, what its ray families hold, that the admissible sets are not vacuous, that they
agree with the brute-force tracers the suite already has, and that a planted fault fails the check tests/test_trace_edges.py applies to the kernels;
the same conditions for the hard poses tests/test_refit_hard.py refits a live scene into."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import kit
from tests import trace_ref as R

F32 = np.float32
SCENE_NAMES = list(R.SCENES)
SINGLE = ("axis", "near_axis", "generic", "slivers", "grazing")                        # >= 90 % of their rays have exactly one admissible answer
FEW = ("axis_on_planes", "edges", "corners", "in_wall", "start_near", "det")          # >= 90 % have at most 8


def test_k_is_measured():
    """K of trace_ref is the next power of two at or above twice the worst |x32 - x64| / (2^-24 abs-form) of a million random pairs, where x32 is the
    fp32 restatement of tri_test (its fma chains, the reciprocal off by -1, 0 or +1 ulp); the worst ratio stays at or below K / 2."""
    worst = R.k_trial(1_000_000)
    print("\nworst |x32 - x64| / (2^-24 abs-form): " + ", ".join("%s %.2f" % kv for kv in worst.items()))
    w = max(worst.values())
    assert R.K == 2.0 ** np.ceil(np.log2(2.0 * w)), (w, R.K)
    assert w <= R.K / 2


def test_tri_test32_lies_within_the_bounds():
    """tri_test32 (fma chains, reciprocal) on generic pairs aimed into the triangle: a, t, u, v within the bounds of mt64."""
    rng = np.random.default_rng(3)
    tri = rng.uniform(-1, 1, (200, 3, 3)); o = rng.uniform(-1, 1, (200, 3)) + np.array([0, 0, 4.0]); d = R._aim(o, tri.mean(1))
    a, t, u, v = R.tri_test32(tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], o, d)
    m = R.mt64(R._r(tri[:, 0]), R._r(tri[:, 1] - tri[:, 0]), R._r(tri[:, 2] - tri[:, 0]), R._r(o), R._r(d))
    for got, x in ((a, "a"), (t, "t"), (u, "u"), (v, "v")):
        assert np.all(np.abs(got - m[x]) <= m["b" + x])


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_families_hold_what_they_are_for(pkg, name):
    scene, rays, rs = R.case(pkg, name)
    fam = rays["family"]; room = name in R.ROOMS
    v0, e1, e2, o, d = R.records(scene, rays["origin"], rays["direction"])
    assert rs.n < 25_000 and np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).any(1).all()
    # the probes see exactly the fp32 values the generators chose
    assert np.array_equal(o.astype(np.float64) + R.centre_of(scene), rays["origin"]) and np.array_equal(d.astype(np.float64), rays["direction"])
    want = {"axis", "near_axis", "start_near", "edges", "generic", "t2"} | ({"axis_on_planes", "in_wall", "corners"} if room else {"slivers", "det", "grazing"})
    assert set(fam) == want
    for f in want:
        assert 500 <= (fam == f).sum() <= 2000, f
    # axis: +-e_i, every combination of +0.0 and -0.0 in the other two
    ax = d[fam == "axis"]
    assert ((ax != 0).sum(1) == 1).all() and set(np.abs(ax[ax != 0])) == {1.0} and {-1.0, 1.0} <= set(ax[ax != 0])
    zero_signs = {tuple(np.signbit(row[row == 0]).tolist()) for row in ax}
    assert zero_signs == {(False, False), (False, True), (True, False), (True, True)}
    # near_axis: both sides of the 1e-30 switch, the switch itself, a denormal; either sign
    na = d[fam == "near_axis"]; small = na[np.abs(na) < 1e-7]
    tiny = F32(1e-30)
    for val in (tiny, np.nextafter(tiny, F32(0)), np.nextafter(tiny, F32(1)), F32(1e-38), F32(1e-31), F32(1.0000001e-30), F32(1e-29), F32(1e-20), F32(1e-8)):
        assert (small == val).any() and (small == -val).any(), val
    assert F32(1.0000001e-30) > tiny > np.nextafter(tiny, F32(0))
    # start_near: triangles at, just below and just above the 1e-4 start of the ray, and origins on a surface
    sn = fam == "start_near"
    m = R.mt64(v0[None], e1[None], e2[None], o[sn][:, None, :], d[sn][:, None, :])
    with np.errstate(invalid="ignore"):
        ts = m["t"][(m["u"] > 0.01) & (m["v"] > 0.01) & (m["w"] > 0.01)]
    for lo_, hi_ in ((-1e-6, 1e-6), (0.4e-4, 0.6e-4), (0.99e-4, R.T_MIN), (R.T_MIN, 1.01e-4), (1.9e-4, 2.1e-4), (0.99e-3, 1.01e-3), (-1.01e-3, -0.99e-4)):
        assert ((ts >= lo_) & (ts < hi_)).sum() >= 10, (lo_, hi_)
    # t2: every kind, and the limits are the fp32 neighbours where they are meant to be
    t2 = fam == "t2"
    assert set(rays["t2_kind"][t2]) == set(R.T2_KINDS) and (rays["t2"][~t2] == 1e300).all()
    assert set(fam[rays["source"][t2]]) == want - {"t2"}
    by = lambda k: rays["t2"][t2 & (rays["t2_kind"] == k)]
    assert (by("3e38") == 3.0e38).all() and (by(">3e38") > 3.0e38).all() and np.array_equal(by("t/2").astype(F32).astype(np.float64), by("t/2"))
    t_of = dict(zip(rays["source"][t2 & (rays["t2_kind"] == "t/2")].tolist(), (2 * by("t/2")).tolist()))
    for kind, fn in (("t", lambda t: t), ("t-", lambda t: np.nextafter(F32(t), F32(0))), ("t+", lambda t: np.nextafter(F32(t), F32(np.inf)))):
        idx = np.nonzero(t2 & (rays["t2_kind"] == kind))[0]
        assert idx.size >= 50 and all(rays["t2"][i] == float(fn(t_of[int(rays["source"][i])])) for i in idx), kind
    if room:
        g = scene.meta["grid"]; s = scene.meta["scale"]
        cell = lambda x: (x.astype(np.float64) / s + 0.5) * g                          # device coordinate -> lattice units, exactly
        assert fam[0] == "axis_on_planes" and (fam[:1000] == "axis_on_planes").all()  # whole waves of them at the head of the list
        op = cell(o[fam == "axis_on_planes"]); dp = d[fam == "axis_on_planes"]
        on = (op == np.rint(op)) & (dp == 0)
        assert (on.sum(1) >= 1).all() and (on.sum(1) == 2).sum() >= 200 and (on.sum(1) == 1).sum() >= 200
        assert ((dp != 0).sum(1) == 1).all() and np.signbit(dp[dp == 0]).any()
        ow = cell(o[fam == "in_wall"]); dw = d[fam == "in_wall"]
        assert ((((ow == 0) | (ow == g)) & (dw == 0)).any(1)).all()
        oc = cell(o[fam == "corners"]); dc = d[fam == "corners"]
        along = (dc != 0).sum(1) == 1
        assert along.sum() >= 200 and ((((oc == 0) | (oc == g)) & (dc == 0)).sum(1)[along] == 2).all() and (~along).sum() >= 200
        info_free = R.displaced(scene) if name == "room16" else None
        if info_free is not None:                                                   # the refit pose keeps the bounding box and moves the wall interiors
            assert np.array_equal(R.centre_of(info_free), R.centre_of(scene)) and (info_free.vertex != scene.vertex).any(1).mean() > 0.7
    else:
        m = R.mt64(v0[None], e1[None], e2[None], o[fam == "det"][:, None, :], d[fam == "det"][:, None, :])
        with np.errstate(invalid="ignore"):
            aa = np.abs(m["a"][(m["u"] > 0.2) & (m["v"] > 0.2) & (m["w"] > 0.2)])      # the triangle the ray was aimed into
        for lo_, hi_ in ((1e-7, R.A_ANY), (R.A_ANY, R.A_CLOSEST), (R.A_CLOSEST, 1e-4)):
            assert ((aa > lo_) & (aa < hi_)).sum() >= 50, (lo_, hi_)
        # between the two thresholds the any-hit rule accepts what the closest-hit rule rejects
        det = np.isin(rs.ray, np.nonzero(fam == "det")[0])
        assert ((rs.sa[det] == R.SURE) & (rs.sc[det] == R.REJ)).sum() >= 20


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_admissible_sets_are_not_vacuous(pkg, name):
    """The restatement alone decides: >= 90 % of the rays of SINGLE have exactly one admissible closest-hit answer, >= 90 % of the rays of FEW at most 8,
    and >= 40 % of the t2 family have a forced any-hit verdict."""
    scene, rays, rs = R.case(pkg, name)
    rows = R.family_table(rs, rays)
    R.print_table("%s: %d triangles, %d rays" % (name, scene.face.shape[0], rs.n), rows)
    for f, n, one, few, forced, _ in rows:
        if f in SINGLE: assert one >= 0.9, (f, one)
        if f in FEW: assert few >= 0.9, (f, few)
        if f == "t2": assert forced >= 0.4, forced
    assert (rs.n_admissible >= 1).all()                                               # every ray has an admissible answer


def _brute(scene, o, d, dtype, centre=None):
    """kit.brute_force_trace, the rays in eight slices side by side."""
    cut = np.linspace(0, o.shape[0], 9).astype(int)
    with ThreadPoolExecutor(8) as pool:
        parts = list(pool.map(lambda k: kit.brute_force_trace(scene, o[cut[k]:cut[k + 1]], d[cut[k]:cut[k + 1]], dtype, chunk=32, centre=centre), range(8)))
    return tuple(np.concatenate(x) for x in zip(*parts))


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_agrees_with_the_brute_force_tracers(pkg, name):
    """Where a ray has a single admissible answer, kit.brute_force_trace(np.float64) names it; kit.brute_force_trace(np.float32) -- fp32 arithmetic on
    the device's records, separate roundings and a true division -- is admissible on EVERY ray, its t, u, v within the bounds."""
    scene, rays, rs = R.case(pkg, name)
    o, d = rays["origin"], rays["direction"]
    one = rs.single()
    _, f64, _, _ = _brute(scene, o, d, np.float64)
    m = one > -2
    wrong = np.nonzero(m & (f64 != one))[0]
    assert wrong.size == 0, "fp64 brute force names face %d; %s" % (f64[wrong[0]], R.describe(rs, rays, wrong[0], f64[wrong[0]]))
    t, f, u, v = _brute(scene, o, d, np.float32)
    bad, ratio = rs.check_closest(f, t, u, v)
    print("\n%s: fp32 brute force, worst error / bound %.3f" % (name, ratio.max()))
    assert not bad.any(), R.describe(rs, rays, np.nonzero(bad)[0][0], f[np.nonzero(bad)[0][0]])


def _closest32(scene, o, d, drop=None, centre=None):
    """The fp32 restatement's closest hit of a few rays (tri_test32 + tri_accept_closest), leaving triangle drop[i] out for ray i."""
    v0, e1, e2, ol, dl = R.records(scene, o, d, centre)
    a, t, u, v = R.tri_test32(v0[None], e1[None], e2[None], ol[:, None, :], dl[:, None, :])
    with np.errstate(invalid="ignore"):
        ok = (np.abs(a) >= F32(1e-5)) & (t >= F32(1e-4)) & (t < F32(3.0e38)) & (u >= 0) & (v >= 0) & (F32(1) - u - v >= 0)
    if drop is not None: ok[np.arange(o.shape[0]), drop] = False
    tt = np.where(ok, t, np.inf); k = tt.argmin(1); rows = np.arange(o.shape[0]); hit = np.isfinite(tt[rows, k])
    return np.where(hit, tt[rows, k], 0).astype(F32), np.where(hit, k, -1), np.where(hit, u[rows, k], 0).astype(F32), np.where(hit, v[rows, k], 0).astype(F32)


@pytest.mark.parametrize("name", ["room16", "soup"])
def test_planted_faults_fail_the_check(pkg, name):
    """Negative controls, on the fp32 restatement's own answers: the nearest surely accepted triangle dropped on 1 ray in 2 000, u moved by 16 bounds, a blocked verdict flipped -- each makes exactly the tampered rays fail."""
    _plant_faults(*R.case(pkg, name))


def _plant_faults(scene, rays, rs, centre=None, single_answer=False):
    """single_answer: the ray that loses its triangle is the first from the usual one on whose only admissible answer is that triangle (in a pose of
    overlapping slivers the second-nearest triangle of a ray may well be admissible too)."""
    o, d = rays["origin"], rays["direction"]
    pick = np.nonzero(rs.sure_closest > 0)[0][:2000]
    t, f, u, v = _closest32(scene, o[pick], d[pick], centre=centre)
    sub = lambda face, t_, u_, v_: _sub_check(rs, pick, face, t_, u_, v_)
    bad, _ = sub(f, t, u, v)
    assert not bad.any()
    # 1 in 2 000: one ray of these 2 000 loses its nearest surely accepted triangle
    j = 1234 % pick.size
    if single_answer: j += int(np.argmax(rs.n_admissible[pick[j:]] == 1))
    nearest_sure = rs.face[(rs.ray == pick[j]) & (rs.sc == R.SURE)][np.argmin(rs.t[(rs.ray == pick[j]) & (rs.sc == R.SURE)])]
    tj, fj, uj, vj = _closest32(scene, o[pick[j:j + 1]], d[pick[j:j + 1]], drop=np.array([nearest_sure]), centre=centre)
    t2_, f2, u2, v2 = t.copy(), f.copy(), u.copy(), v.copy(); t2_[j], f2[j], u2[j], v2[j] = tj[0], fj[0], uj[0], vj[0]
    bad, _ = sub(f2, t2_, u2, v2)
    assert bad[j] and bad.sum() == 1
    # u moved by 16 bounds
    full_f = np.full(rs.n, -1); full_f[pick] = f
    rep = np.arange(rs.n, dtype=np.int64) * rs.n_faces + np.maximum(full_f, 0)
    bu = rs.bu[np.searchsorted(rs.key, rep[pick])]
    bad, _ = sub(f, t, (u.astype(np.float64) + 16 * bu), v)
    assert bad.all()
    bad, _ = sub(f, t, (u.astype(np.float64) - 16 * bu), v)
    assert bad.all()
    # a verdict flipped where it is forced
    verdict = rs.sure_any > 0
    assert not rs.check_any(verdict).any()
    forced = np.nonzero(rs.forced_any)[0]
    assert (rs.sure_any[forced] > 0).any() and (rs.sure_any[forced] == 0).any()
    for i in (forced[np.argmax(rs.sure_any[forced] > 0)], forced[np.argmax(rs.sure_any[forced] == 0)]):
        flipped = verdict.copy(); flipped[i] = not flipped[i]
        bad = rs.check_any(flipped)
        assert bad[i] and bad.sum() == 1


def _sub_check(rs, pick, face, t, u, v):
    """check_closest for the rays `pick` only (the others report their own single answer or a miss and are masked out)."""
    F = np.full(rs.n, -1); T = np.zeros(rs.n); U = np.zeros(rs.n); V = np.zeros(rs.n)
    F[pick] = face; T[pick] = t; U[pick] = u; V[pick] = v
    bad, ratio = rs.check_closest(F, T, U, V)
    return bad[pick], ratio[pick]


# ------------------------------------------------------------------------------------------------------------------------ hard poses
HIT_POSES = ("scramble", "stretch", "far", "mirror", "fold", "third-degenerate")


@pytest.mark.parametrize("name,pose", R.POSE_CASES)
def test_poses_are_what_they_say(pkg, name, pose):
    scene, moved, rays, rs = R.pose_case(pkg, name, pose)
    c = R.centre_of(scene); v, w = scene.vertex, moved.vertex
    used = R._used(scene)
    assert np.array_equal(w, w.astype(F32)) and np.array_equal(moved.face, scene.face) and rs.n_faces == scene.face.shape[0]
    # the probes see fp32 origins about the CREATION centre
    o = R.records(moved, rays["origin"], rays["direction"], c)[3]
    assert np.array_equal(o.astype(np.float64) + c, rays["origin"]) and (rs.n_admissible >= 1).all()
    p = w[moved.face[:, :, 0]]; area2 = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    ext = lambda x: x[used].max(0) - x[used].min(0)
    if pose == "scramble":
        assert np.array_equal(np.sort(w[used], 0), np.sort(v[used], 0)) and np.array_equal(R.centre_of(moved), c) and (w[used] != v[used]).any(1).mean() > 0.99
        if name == "room16":                                                          # every triangle spans the scene: the median box covers a twentieth of its volume
            assert np.median(np.prod(p.max(1) - p.min(1), axis=1)) > 0.05
    if pose == "stretch":
        assert np.all(ext(w)[0] / ext(w)[2] >= 2.0 ** 23) and np.allclose(R.centre_of(moved), c, atol=1e-3)
    if pose == "far":
        assert np.allclose(R.centre_of(moved) - c, R.FAR, rtol=0, atol=1e-5) and np.abs(w[used] - c).max() > 128
    if pose == "mirror":
        q = v[scene.face[:, :, 0]]; n0 = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]); n1 = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert np.all(n0[:, 0] * n1[:, 0] >= 0) and np.all(n0[:, 1] * n1[:, 1] <= 0) and np.all(n0[:, 2] * n1[:, 2] <= 0) and np.array_equal(R.centre_of(moved), c)
    if pose == "fold":
        assert np.all(ext(w)[1:] > ext(v)[1:] + R.FOLD)
    if pose in R.COLLAPSED:
        flat = {"plane": [2], "line": [1, 2], "point": [0, 1, 2]}[pose]
        assert np.array_equal(w[used][:, flat], np.broadcast_to(c.astype(F32).astype(np.float64)[flat], (used.size, len(flat))))
        assert (area2 == 0).all() if pose != "plane" else (area2 > 0).any()
    if pose == "third-degenerate":
        assert (area2[::3] == 0).all() and (area2[1::3] > 0).all() and (area2[2::3] > 0).all()


@pytest.mark.parametrize("name,pose", R.POSE_CASES)
def test_pose_admissible_sets_are_not_vacuous(pkg, name, pose):
    """Conditions on the restatement alone, so that the GPU test of a pose is not vacuous.  Poses that keep triangles: at least half the base rays (the t2
    family excluded) of soup and room16 have a single admissible answer that is a hit (one / two, which most rays of the list miss: at least a
    family's worth, 500).  line, point: a miss is every ray's only answer and no verdict may be "blocked".  plane: at least 5 % of the rays have a
    surely accepted triangle."""
    scene, moved, rays, rs = R.pose_case(pkg, name, pose)
    base = rays["family"] != "t2"
    one = rs.single()
    share = float((one[base] >= 0).mean()); sure = float((rs.sure_closest > 0).mean())
    print("\n%s in pose %s: %d rays, single admissible hit %.3f of the base rays, single miss %.3f, a surely accepted triangle %.3f of all rays" % (
        name, pose, rs.n, share, float((one[base] == -1).mean()), sure))
    R.print_table("%s, %s" % (name, pose), R.family_table(rs, rays))
    if pose in HIT_POSES:
        if name in ("one", "two"): assert (one[base] >= 0).sum() >= R.N_FAMILY
        else: assert share >= 0.5, share
        assert rs.forced_any[~base].mean() >= 0.4
    elif pose == "plane":
        assert sure >= 0.05, sure
    else:
        assert (one == -1).all() and (rs.open_any == 0).all() and rs.key.size == 0


@pytest.mark.parametrize("name,pose", R.POSE_CASES)
def test_poses_agree_with_the_fp32_brute_force_tracer(pkg, name, pose):
    """kit.brute_force_trace(np.float32) on the posed scene's records about the creation centre is admissible on EVERY ray of every pose."""
    scene, moved, rays, rs = R.pose_case(pkg, name, pose)
    t, f, u, v = _brute(moved, rays["origin"], rays["direction"], np.float32, centre=R.centre_of(scene))
    bad, ratio = rs.check_closest(f, t, u, v)
    print("\n%s in pose %s: fp32 brute force, worst error / bound %.3f, %.3f of the rays hit" % (name, pose, ratio.max(), (f >= 0).mean()))
    assert not bad.any(), R.describe(rs, rays, np.nonzero(bad)[0][0], f[np.nonzero(bad)[0][0]])


@pytest.mark.parametrize("name,pose", [("room16", "scramble"), ("soup", "stretch"), ("soup", "far"), ("two", "far"), ("room16", "mirror"), ("soup", "fold"),
                                       ("soup", "plane"), ("soup", "third-degenerate")])
def test_planted_faults_fail_the_check_in_a_pose(pkg, name, pose):
    """test_planted_faults_fail_the_check's faults on the posed scenes' restatements."""
    scene, moved, rays, rs = R.pose_case(pkg, name, pose)
    _plant_faults(moved, rays, rs, centre=R.centre_of(scene), single_answer=True)


@pytest.mark.parametrize("name,pose", [("room16", "line"), ("soup", "point")])
def test_planted_faults_fail_the_check_in_a_collapsed_pose(pkg, name, pose):
    """Where nothing can be hit: one reported hit, one "blocked" -- each fails exactly its ray."""
    scene, moved, rays, rs = R.pose_case(pkg, name, pose)
    f = np.full(rs.n, -1); z = np.zeros(rs.n)
    assert not rs.check_closest(f, z, z, z)[0].any() and not rs.check_any(np.zeros(rs.n, bool)).any()
    f[1234] = 5
    bad = rs.check_closest(f, z, z, z)[0]
    assert bad[1234] and bad.sum() == 1
    blocked = np.zeros(rs.n, bool); blocked[4321] = True
    bad = rs.check_any(blocked)
    assert bad[4321] and bad.sum() == 1
