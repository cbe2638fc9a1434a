"""-m gpu: "a large deformation makes traversal slower, never wrong" (mcpt.h, refit.hip), on the poses of tests/trace_ref.py that are not gentle -- every
triangle spanning the scene, extents 2^24 apart between axes, a scene far from the centre it was created about, flipped windings, folds, a scene
collapsed onto a plane, a line and a point, degenerate triangles among live ones, a light of area 0.  A live context is created with the creation
scene and moved into the pose by mcpt_update_vertices, which refits both trees; then EVERY ray of the pose's list goes through wf_trace8_kernel and
bvh_traverse, closest hit and any hit, against the fp64 restatement's admissible answers (tests/kit.py: check_both_kernels).  No percentage and no
second GPU context decides a ray.  Further: the light records against a numpy restatement of rf_lights_kernel bit for bit, the film, no memory of the
pose after the way back, and a rebuild in the pose.  The conditions that keep this from being vacuous are asserted on the CPU (tests/test_trace_ref.py).
Measured on an MI355X: DESIGN.md, "Refit under hard deformations"."""
import numpy as np
import pytest

from tests import kit
from tests import trace_ref as R
from tests.kit import bits, check_both_kernels, render_film, trace_context

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 13
CASES = [(name, pose, tree) for name, pose in R.POSE_CASES for tree in (("host",) if name in ("one", "two") else ("host", "device"))]
ZERO_AREA_LIGHTS = {("soup", "point"), ("soup", "line"), ("room16", "point"), ("room16", "line"), ("room16", "plane"), ("soup", "third-degenerate")}


def _flags(pkg):
    return pkg.FLAG_DYNAMIC | pkg.FLAG_DETERMINISTIC | pkg.FLAG_COUNT_TRAVERSAL


def _work(r):
    """The film of 4 samples and the box + triangle tests it took."""
    r.reset_counters()
    film = render_film(r, 4, SEED)
    c = r.counters()
    return film, int(c.box_tests + c.tri_tests)


def _probes(r, rays):
    o, d, t2 = rays["origin"], rays["direction"], rays["t2"]
    return r.probe_trace4(o, d) + (r.probe_trace4(o, d, t2=t2, any_hit=True)[1],) + r.probe_trace(o, d) + (r.probe_trace(o, d, t2=t2, any_hit=True)[1],)


_identity = {}


def _after_an_identity_update(pkg, name, tree):
    """What a context of the creation scene shows after ONE update with its own vertices: the answers of both kernels to the creation scene's ray
    list, the film, wide_area_ratio.  Once per (scene, tree) and session."""
    if (name, tree) not in _identity:
        scene, rays, _ = R.case(pkg, name)
        r = trace_context(pkg, scene, tree, flags=_flags(pkg))
        try:
            r.update_vertices(scene.vertex)
            _identity[(name, tree)] = (_probes(r, rays), _work(r)[0], r.update_info().wide_area_ratio)
        finally:
            r.close()
    return _identity[(name, tree)]


def lights_restated(moved, faces, centre):
    """rf_lights_kernel (refit.hip, contraction off) for the light triangles `faces`: the area from the fp32 edges -- every product and difference
    rounded, (cx cx + cy cy) + cz cz in fp32, the root in fp64 rounded once, times 0.5 -- and the nine fp64 corner coordinates less the centre."""
    p = moved.vertex[moved.face[faces][:, :, 0]].astype(np.float64)
    e1, e2 = (p[:, 1] - p[:, 0]).astype(F32), (p[:, 2] - p[:, 0]).astype(F32)
    with np.errstate(over="raise", invalid="raise"):
        cx = e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2]; cy = e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0]; cz = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]
        s = (cx * cx + cy * cy) + cz * cz
    assert all(x.dtype == F32 for x in (cx, cy, cz, s))
    return F32(0.5) * np.sqrt(s.astype(np.float64)).astype(F32), (p - centre).reshape(-1, 9)


def _by_face(lights):
    face, rec, pos = lights
    k = np.argsort(face, kind="stable")
    return face[k], rec[k], pos[k]


@pytest.mark.parametrize("name,pose,tree", CASES)
def test_refit_in_a_hard_pose(pkg, name, pose, tree):
    scene, moved, rays, rs = R.pose_case(pkg, name, pose)
    _, rays0, _ = R.case(pkg, name)
    centre = R.centre_of(scene)
    title = "%s in pose %s, %s tree" % (name, pose, tree)
    want_probes, want_film, want_ratio = _after_an_identity_update(pkg, name, tree)
    r = trace_context(pkg, scene, tree, flags=_flags(pkg))
    try:
        assert list(r.info().centre) == centre.tolist()
        _, work0 = _work(r)
        face0, rec0, _ = r.probe_lights()
        assert face0.size > 0

        # 1. every ray admissible after the pose
        r.update_vertices(moved.vertex)
        assert list(r.info().centre) == centre.tolist()
        r.validate_trees()
        r.reset_counters()
        check_both_kernels(r, rs, rays, title)
        c = r.counters()                                                             # (of the two wf_trace8_kernel launches: probe_trace does not count)
        ratio = r.update_info().wide_area_ratio
        print("\n[hard pose] %s: wide depth %d  wide_area_ratio %.6g  stack spills %d  box tests per ray %.1f  triangle tests per ray %.1f" % (
            title, r.info().wide_depth, ratio, c.stack_spills, c.box_tests / (2.0 * rs.n), c.tri_tests / (2.0 * rs.n)))
        # 2. the overflow stack, on the pose whose boxes all overlap.  A lane holds at most two entries per level of the wide tree and eight of them in
        # LDS: room16's trees are too shallow to spill whatever their boxes do (0 spills measured); soup's are not, so the scene that reaches the
        # overflow stack on a refitted tree is soup, with both builders, and no further scene is needed for it.
        if (name, pose) == ("soup", "scramble"):
            assert c.stack_spills > 0

        # 3. the film and the ratio
        film = render_film(r, 4, SEED)
        assert np.isfinite(film).all() and (film[..., 3] == 4).all()
        assert np.isfinite(ratio) and ratio >= 0
        lp, lxi = kit.light_points(*kit.used_bounds(scene), 500, 2)
        if pose in ("point", "line"):
            # nothing can be hit, and every light has area 0: pdf = d2 / cs / 0 is an infinity (or the guard's 0), whose reciprocal the shade kernel
            # multiplies the light's radiance by -- 0 reaches the film.  A NaN direction, radiance, distance or pdf would reach it as it is.
            assert (film[..., :3] == 0).all()
            ls = r.probe_sample_light(lp, lxi)
            assert not np.isnan(ls).any()
            assert np.isin(np.abs(ls[:, 6]), (0.0, np.inf)).all()

        # 4. the light records, bit for bit
        face, rec, pos = r.probe_lights()
        area, pos9 = lights_restated(moved, face, centre)
        assert np.array_equal(face, face0) and np.array_equal(bits(rec[:, 1:]), bits(rec0[:, 1:]))     # radiance and normals: as they were
        assert np.array_equal(bits(rec[:, 0]), bits(area)), (rec[:, 0], area)
        assert np.array_equal(bits(pos), bits(pos9))
        assert ((name, pose) in ZERO_AREA_LIGHTS) == bool((area == 0).all()) and ((name, pose) in ZERO_AREA_LIGHTS or (area > 0).all())
        if pose in ("scramble", "mirror"):                                           # the centre stays: a fresh context of the posed scene holds the same records
            assert np.array_equal(R.centre_of(moved), centre)
            f = trace_context(pkg, moved, tree, flags=pkg.FLAG_DETERMINISTIC)
            try:
                for a, b in zip(_by_face((face, rec, pos)), _by_face(f.probe_lights())):
                    assert np.array_equal(bits(a), bits(b))
                lpm, _ = kit.light_points(*kit.used_bounds(moved), 500, 2)
                assert np.array_equal(bits(r.probe_sample_light(lpm, lxi)), bits(f.probe_sample_light(lpm, lxi)))
            finally:
                f.close()

        # 5. no memory of the pose
        r.update_vertices(scene.vertex)
        r.validate_trees()
        for a, b in zip(_probes(r, rays0), want_probes):
            assert np.array_equal(bits(a), bits(b))
        back, work1 = _work(r)
        assert np.array_equal(bits(back), bits(want_film))
        assert r.update_info().wide_area_ratio == want_ratio
        print("[hard pose] %s: traversal work of the film after the way back / before the pose = %.6f" % (title, work1 / max(work0, 1)))
        # not a measurement: a refitted box exceeds the built one only by padding a padded box again (~1e-6 relative per level)
        assert work1 <= 1.01 * work0

        # 6. new trees in the pose
        if pose in ("scramble", "point"):
            r.update_vertices(moved.vertex)
            r.rebuild()
            assert r.update_info().wide_area_ratio == 1.0
            r.validate_trees()
            check_both_kernels(r, rs, rays, title + ", rebuilt")
    finally:
        r.close()
