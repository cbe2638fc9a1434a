"""-m gpu: make_bsdf / bsdf_eval / bsdf_sample and sample_light of csrc/pt_device.h at their edges, through the probes of the C ABI, against the
float64 restatement and the error model of tests/shade_ref.py (BSDF) and against the oracle (light sampling).  One probe launch per scene; the
inputs, the restatement and the oracle's answers are computed once per module.

What the device is allowed: DEVICE_FACTOR (4) times the K the fp32 oracle needs on the same inputs (K_ORACLE, measured by tests/test_shade_ref.py),
per output, outside `marginal`; discrete outcomes equal, none forgiven.  Measured on an MI355X: see DESIGN.md, "Accuracy of the shading functions".
"""
import numpy as np
import pytest

from tests import shade_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def edge(pkg):
    """(cases, restatement, ~marginal, the device's out12, the allowed differences)."""
    case = R.bsdf_edge_cases()
    ref = R.bsdf_ref(*R.case_arrays(case))
    r = pkg.Renderer(pkg.scenes.open_box(8, 8))
    out = r.probe_bsdf(*R.case_arrays(case))
    r.close()
    return case, ref, ~R.marginal(case, ref), out, R.budget(case, ref, R.DEVICE_FACTOR * R.K_ORACLE)


def _worst(case, ref, ok, out):
    """Per family: the device's worst ratio to the oracle's budget (K_ORACLE), and the largest direction error with its bound."""
    k = np.where(ok, R.smallest_k(case, ref, out), 0.0) / R.K_ORACLE
    for f in np.unique(case["family"]):
        m = case["family"] == f
        print("%-16s worst ratio to the oracle's budget %6.2f (allowed %.0f)" % (f, k[m].max(), R.DEVICE_FACTOR))
    return k


def test_probe_bsdf_edges_discrete_outcomes(edge):
    """Outside `marginal`, with no share forgiven: the mirror flag, failed-or-not (pdf == 0) and the lobe taken equal the restatement's.  The lobe shows
    in the sampled direction: where the two lobes' directions are more than 0.05 apart, the device's is within 0.01 of the one the restatement took."""
    case, ref, ok, out, _ = edge
    assert np.array_equal(out[ok, 11], ref.out12[ok, 11])
    assert np.array_equal(out[ok, 10] == 0, ref.failed[ok])
    two = ok & (ref.kind != R.DIFFUSE) & ~ref.failed & np.isfinite(ref.out12[:, 4:7]).all(1)
    two &= np.linalg.norm(ref.wo_diffuse - ref.wo_specular, axis=1) > 0.05
    took_spec = np.linalg.norm(out[:, 4:7] - ref.wo_specular, axis=1) < 0.01
    took_diff = np.linalg.norm(out[:, 4:7] - ref.wo_diffuse, axis=1) < 0.01
    assert two.sum() > 1500 and set(ref.lobe[two]) == {R.DIFFUSE, R.PHONG, R.MIRROR}
    assert np.array_equal(took_spec[two], ref.lobe[two] != R.DIFFUSE) and np.array_equal(took_diff[two], ref.lobe[two] == R.DIFFUSE)
    # the exact tie w_spec == xi * total goes to the specular lobe (lower_bound: the first prefix sum that is >= r)
    tie = two & (case["family"] == "lobe_boundary") & (case["xi"][:, 0] == 0.5)
    assert tie.sum() >= 80 and took_spec[tie].all()
    # Ns = 9999 is Blinn-Phong, Ns = 10000 the mirror
    spec = ok & ref.up & (ref.lobe != R.DIFFUSE)
    assert (out[spec & (case["ns"] == 9999), 11] == 0).all() and (spec & (case["ns"] == 9999)).sum() > 10
    assert (out[spec & (case["ns"] == 10000), 11] == 1).all() and (spec & (case["ns"] == 10000)).sum() > 10


def test_probe_bsdf_edges_black_material_ends_the_path(edge):
    """Kd = Ks = 0 (SURVEY A-12): the sample's pdf and the evaluation's pdf are exactly 0, fx and f finite."""
    case, ref, ok, out, _ = edge
    b = ref.black
    assert b.sum() >= 100 and set(case["ns"][b]) >= {0.0, 10.0, 20000.0}
    assert (out[b, 10] == 0).all() and (out[b, 3] == 0).all() and (out[b, 11] == 0).all()
    assert np.isfinite(out[b]).all() and (out[b, 0:3] == 0).all() and (out[b, 7:10] == 0).all()


def test_probe_bsdf_edges_non_finite_pattern(edge):
    """The device is not a number, or infinite with the same sign, exactly where the restatement is (the mirror at m_wo.z == 0: f = 1 / 0; the half vector
    normalize(0)), and nowhere else."""
    case, ref, ok, out, _ = edge
    assert ref.nonfinite[ok].any(1).sum() >= 30 and np.isnan(ref.out12[ok]).any() and np.isinf(ref.out12[ok]).any()
    assert np.array_equal(np.isnan(out[ok]), np.isnan(ref.out12[ok]))
    inf = np.isinf(ref.out12) & ok[:, None]
    assert np.array_equal(np.isinf(out) & ok[:, None], inf) and np.array_equal(out[inf], ref.out12[inf].astype(np.float32))


def test_probe_bsdf_edges_values_within_four_times_the_oracles_budget(edge):
    """Every output of every case outside `marginal` within the error model at DEVICE_FACTOR * K_ORACLE; the worst ratio per family is printed.  The
    sampled direction of a diffuse or mirror pick has the absolute bound 4 K 2^-23 (|q| + 1) <= 1.91e-6."""
    case, ref, ok, out, allowed = edge
    k = _worst(case, ref, ok, out)
    fin = ok[:, None] & ~ref.nonfinite
    with np.errstate(invalid="ignore"):
        err = np.abs(out.astype(np.float64) - ref.out12)
    dirs = ok & (ref.lobe != R.PHONG) & ~ref.nonfinite[:, 4:7].any(1)
    ph = ok & (ref.lobe == R.PHONG)
    wide = ph & (ref.sin_t >= 0.01)
    print("direction of a diffuse / mirror pick: worst error %.3g, bound %.3g; of a Phong pick with sin theta >= 0.01: worst %.3g, bound %.3g; of any Phong "
          "pick: worst %.3g, bound %.3g" % (err[dirs, 4:7].max(), allowed[dirs, 4:7].max(), err[wide, 4:7].max(), allowed[wide, 4:7].max(),
                                           err[ph, 4:7].max(), allowed[ph, 4:7].max()))
    assert allowed[dirs, 4:7].max() <= R.DEVICE_FACTOR * R.K_ORACLE * 2.0 ** -23 * 2.0001
    bad = fin & ~(err <= allowed)
    assert not bad.any(), "%d outputs beyond the budget, worst ratio %.2f in family %s" % (bad.sum(), k.max(), case["family"][k.argmax()])


def test_probe_bsdf_edges_named_properties(edge):
    """The properties a wrong branch would break, each on the family built for it and each within the budget of the model:
    Ns = 0 gives the Blinn-Phong pdf w_spec / (2 pi) plus the diffuse term; either side of |n.x| = 0.9f takes the restatement's frame (the other frame
    turns the sampled direction by order 1); the energy rescale follows !(max < 1) at max == 1, one ulp below and above."""
    case, ref, ok, out, allowed = edge
    fam = case["family"]
    ns0 = ok & (case["ns"] == 0) & (ref.kind == R.PHONG) & ref.up & (ref.wo_z >= 0)
    want = ref.w_spec / (2 * np.float64(R.PI_F)) + ref.wo_z / np.float64(R.PI_F) * ref.w_diff
    assert ns0.sum() >= 40 and np.all(np.abs(out[ns0, 3] - want[ns0]) <= allowed[ns0, 3])
    fs = ok & (fam == "frame_switch") & ~ref.failed
    assert fs.sum() >= 200 and np.all(np.abs(out[fs, 4:7] - ref.out12[fs, 4:7]) <= allowed[fs, 4:7])
    en = ok & (fam == "energy")
    assert en.sum() >= 250 and np.all(np.abs(out[en, 0:3] - ref.out12[en, 0:3]) <= allowed[en, 0:3])
    assert np.all(np.abs(out[en, 7:10] - ref.out12[en, 7:10]) <= allowed[en, 7:10])


@pytest.fixture(scope="module")
def light_scenes(pkg):
    S = pkg.scenes
    small = S.cornell_box_small(64, 64)
    off = np.array([1000.0, -3.0, 0.25])                                         # the offset of test_fp32_traversal_envelope_vs_fp64_oracle
    c = small.camera
    moved = S.SceneData("cornell-small-moved", np.vectorize(S._q)(small.vertex + off), small.normal, small.texcoord, small.face, small.materials,
                        S._qcam(tuple(np.asarray(c.eye) + off), tuple(np.asarray(c.lookat) + off), c.up, c.fovy, c.width, c.height), dict(small.meta))
    return {"cornell-small": small, "moved": moved, "nine-lights": R.nine_light_scene(pkg)}


@pytest.mark.parametrize("name", ["cornell-small", "moved", "nine-lights"])
def test_probe_sample_light_edges_vs_oracle(pkg, orc, light_scenes, name):
    """probe_sample_light on light_edge_inputs against Oracle.sample_light: S-cornell-small, the same translated by (1000, -3, 0.25) (the add-back of
    DevScene::centre before the two fp32 roundings) and a nine-light scene (the global-memory light table).  The sampled triangle is the oracle's in
    every case -- the index clamp at xi_l = 1 and every k / n_lights boundary included --, the pdf of an in-plane point is exactly 0, and wo, radiance,
    pdf and t2 meet the tolerances of test_probe_sample_light_vs_reference; the fold at u + v == 1 and one ulp above it lands on the oracle's point."""
    scene = light_scenes[name]
    p, xi, fam = R.light_edge_inputs(scene)
    r = pkg.Renderer(scene)
    out = r.probe_sample_light(p, xi)
    r.close()
    o = orc.Oracle(scene)
    ref = np.array([o.sample_light(p[i], xi[i])[0] for i in range(len(p))])
    tri = np.array([o.sample_light_tri(p[i], xi[i]) for i in range(len(p))])
    o.close()
    lf = R.light_faces(scene)
    idx, clamped = R.light_index(xi[:, 0], len(lf))
    assert clamped.any() and np.array_equal(tri, lf[idx])                       # the oracle clamps as Render.cpp:204-205 does
    assert np.array_equal(out[:, 8], tri.astype(np.float32))
    assert set(tri) == set(lf)
    ip = fam == "in_plane"
    assert ip.sum() >= 100 and (out[ip, 6] == 0).all() and (ref[ip, 6] == 0).all()
    assert (out[~ip, 6] != 0).all()
    for f in np.unique(fam):
        m = fam == f
        assert np.allclose(out[m, 0:3], ref[m, 0:3], atol=1e-6), f               # wo
        assert np.allclose(out[m, 3:6], ref[m, 3:6]), f                          # radiance
        assert np.allclose(out[m, 6], ref[m, 6], rtol=1e-4), f                   # pdf
        assert np.allclose(out[m, 7], ref[m, 7], rtol=1e-6), f                   # t2 = float |d|
    s = xi[:, 1] + xi[:, 2]
    assert ((fam == "fold") & (s == 1)).sum() >= 40 and ((fam == "fold") & (s == np.nextafter(np.float32(1), np.float32(2)))).sum() >= 40
