"""CPU tests (no GPU) of tests/shade_ref.py: the float64 restatement of the BSDF is pinned to the REAL reference's recorded answers, the fp32
oracle is held to it on the deliberately awkward inputs, and the constant of the error model that the device test uses (K_ORACLE) is measured
here, on the reference side.  The device side of the same inputs is tests/test_shade_edges.py."""
import os

import numpy as np
import pytest

from tests import shade_ref as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def kats():
    with np.load(os.path.join(G, "ref_kats.npz")) as z:
        return {k: z[k] for k in z.files if k.startswith("bsdf_")}


@pytest.fixture(scope="module")
def edge(orc):
    """(cases, restatement, marginal mask, the oracle's out12) of the edge cases: computed once."""
    case = R.bsdf_edge_cases()
    ref = R.bsdf_ref(*R.case_arrays(case))
    got = np.zeros((len(case["ns"]), 12), np.float32)
    for i in range(len(got)):
        a = (case["n"][i], case["wi"][i], case["kd"][i], case["ks"][i], float(case["ns"][i]))
        got[i, :4] = orc.Oracle.bsdf_eval(*a, case["wo"][i])
        got[i, 4:] = orc.Oracle.bsdf_sample(*a, case["xi"][i])[0]
    return case, ref, R.marginal(case, ref), got


def test_restatement_reproduces_the_recorded_reference(kats):
    """On the real reference's recorded bsdf_eval / bsdf_sample (fp64 normal and wi, as the reference had them) the restatement, replaying the
    reference's fp32 arithmetic (dtype=float32), agrees at the tolerance test_oracle_vs_reference.py holds the oracle's path radiance to (rtol 1e-6,
    atol 1e-7), mirror flags and failed samples equal: this pins the formulas to the real reference.  In float64 the same code gives the same mirror
    flags; the K its recorded answers would need is printed, not asserted (these are random cases: a mirror at a small m_wo.z divides by a cancelling
    dot product, which the edge cases avoid on purpose).  Black materials are left out as in test_oracle_vs_reference.py: the reference reads
    uninitialised weights there (SURVEY A-12)."""
    k = kats
    sel = k["bsdf_kind"] != 3
    args = [k["bsdf_" + a][sel] for a in ("n", "wi", "kd", "ks", "ns", "wo", "xi")]
    ev, smp = k["bsdf_eval"][sel], k["bsdf_sample"][sel]
    want = np.concatenate([ev, smp], 1)
    r32 = R.bsdf_ref(*args, dtype=np.float32)
    assert np.array_equal(r32.out12[:, 11], smp[:, 7])
    assert np.array_equal(r32.out12[:, 10] == 0, smp[:, 6] == 0)
    assert np.allclose(r32.out12[:, :11], want[:, :11], rtol=1e-6, atol=1e-7)
    r64 = R.bsdf_ref(*args)
    case = dict(zip(("n", "wi", "kd", "ks", "ns", "wo", "xi"), args))
    same = (r64.out12[:, 11] == smp[:, 7]) & ((r64.out12[:, 10] == 0) == (smp[:, 6] == 0)) & ~R.marginal(case, r64)
    kk = R.smallest_k(case, r64, want)[same]
    print("recorded reference against the float64 restatement: %d of %d cases with the same discrete outcome, smallest K %.2f" % (same.sum(), len(same), kk.max()))
    assert same.mean() >= 0.99 and np.array_equal(r64.out12[:, 11], smp[:, 7])


def test_oracle_agrees_with_the_restatement_on_the_edge_cases(edge):
    """Outside `marginal`: mirror flag, failed-or-not and the non-finite pattern of the fp32 oracle equal the restatement's on every edge case, and the
    oracle stays inside the error model at K_ORACLE -- the constant the device is given DEVICE_FACTOR times of.  Prints the measured K by family."""
    case, ref, marg, got = edge
    ok = ~marg
    assert np.array_equal(got[ok, 11], ref.out12[ok, 11])
    assert np.array_equal(got[ok, 10] == 0, ref.failed[ok])
    assert np.array_equal(~np.isfinite(got[ok]), ref.nonfinite[ok])
    assert np.array_equal(np.isnan(got[ok]), np.isnan(ref.out12[ok]))
    inf = np.isinf(ref.out12) & ok[:, None]
    assert np.array_equal(got[inf], ref.out12[inf])                            # the signs of the infinities
    k = np.where(ok, R.smallest_k(case, ref, got), 0.0)
    literal = np.where(ok, R.smallest_k(case, ref, got, sin_term=False), 0.0)
    for f in np.unique(case["family"]):
        print("K %-16s %6.2f" % (f, k[case["family"] == f].max()))
    print("measured K = %.2f (K_ORACLE %.2f); without the sin-theta term of a Phong pick's direction K = %.1f (family %s)"
          % (k.max(), R.K_ORACLE, literal.max(), case["family"][literal.argmax()]))
    assert k.max() <= R.K_ORACLE
    assert k.max() > 0.5 * R.K_ORACLE                                          # the constant is the measurement, not a generous guess


def test_marginal_share_is_at_most_one_percent(edge):
    case, ref, marg, _ = edge
    print("marginal: %d of %d cases = %.2f %%" % (marg.sum(), len(marg), 100 * marg.mean()))
    assert 3500 <= len(marg) <= 4500 and marg.mean() <= 0.01
    assert not marg[(case["ns"] == 10000) | (case["ns"] == 9999)].all()        # the mirror threshold itself is not marginal
    tie = (case["family"] == "lobe_boundary") & (case["xi"][:, 0] == 0.5)
    assert tie.sum() >= 100 and not marg[tie].any()


def test_every_family_has_the_member_it_promises(edge):
    case, ref, marg, _ = edge
    fam = case["family"]
    assert set(fam) == {"grazing_axis", "grazing_generic", "highlight", "exponents", "frame_switch", "energy", "single_lobe", "lobe_boundary", "xi_edges", "random"}
    for name in ("n", "wi", "kd", "ks", "ns", "wo", "xi"):
        assert case[name].dtype == np.float32 and np.isfinite(case[name]).all()
    assert (case["xi"] >= 0).all() and (case["xi"] <= R.ONE_BELOW).all()
    # grazing: local z exactly 0 and exactly each asked value on the axis-aligned normals, for wi and for wo; all three kinds of material
    ga = fam == "grazing_axis"
    for z in R.GRAZING_Z:
        assert (ref.m_wo_z[ga] == np.float64(np.float32(z))).sum() >= 100 and (ref.wo_z[ga] == np.float64(np.float32(z))).sum() >= 100
    assert set(ref.kind[ga & (ref.m_wo_z == 0)]) == {R.DIFFUSE, R.PHONG, R.MIRROR}
    assert np.isinf(ref.out12[ga & (ref.m_wo_z == 0) & (ref.lobe == R.MIRROR), 7]).all()             # the mirror at m_wo.z == 0: f = 1 / (+-0)
    assert ref.nonfinite[ga].any(1).sum() >= 20
    for z in R.GRAZING_Z[1:]:
        assert np.isclose(ref.m_wo_z[fam == "grazing_generic"], z, rtol=0.2, atol=0).any()
    # highlight: within 1e-3 of the mirror direction
    hl = fam == "highlight"
    nn, wi, wo = (case[k][hl].astype(np.float64) for k in ("n", "wi", "wo"))
    assert np.linalg.norm(wo - (2 * (wi * nn).sum(1)[:, None] * nn - wi), axis=1).max() < 1.001e-3 and (1 - ref.hz_eval[hl]).max() < 1e-4
    # exponents: every one, on Blinn-Phong below 10000 and mirror from there on
    ex = fam == "exponents"
    assert set(case["ns"][ex]) == set(np.float32(R.NS_LIST))
    assert (ref.kind[ex & (case["ns"] == 9999)] == R.PHONG).all() and (ref.kind[ex & (case["ns"] == 10000)] == R.MIRROR).all()
    assert set(ref.lobe[ex & (case["ns"] == 0)]) == {R.DIFFUSE, R.PHONG}
    # frame switch: 0.9f and its two neighbours, both signs, the six axes
    nx = case["n"][fam == "frame_switch", 0]
    for x in (R.FRAME_SWITCH, np.nextafter(R.FRAME_SWITCH, np.float32(1)), np.nextafter(R.FRAME_SWITCH, np.float32(0))):
        assert (nx == x).sum() >= 20 and (nx == -x).sum() >= 20
    assert len(np.unique(case["n"][fam == "frame_switch"][np.abs(case["n"][fam == "frame_switch"]).max(1) == 1], axis=0)) == 6
    # energy rescale: max(kd + ks) exactly 1, one ulp below, above -- as fp32 sums, one and two lobes
    en = fam == "energy"
    mx = (case["kd"] + np.where((ref.kind == R.MIRROR)[:, None], np.float32(1), case["ks"])).max(1)
    assert mx.dtype == np.float32
    for kind in (R.DIFFUSE, R.PHONG):
        for v in (np.float32(1), R.ONE_BELOW):
            assert (en & (ref.kind == kind) & (mx == v)).sum() >= 20
        assert (en & (ref.kind == kind) & (mx > 1)).sum() >= 20
    assert (en & (ref.kind == R.MIRROR) & (mx == 1)).sum() >= 20 and (en & (ref.kind == R.MIRROR) & (mx > 1)).sum() >= 20
    # single lobes and the black material
    sl = fam == "single_lobe"
    assert (sl & ref.black).sum() >= 100 and (sl & (ref.w_diff == 0) & (ref.kind != R.DIFFUSE)).sum() >= 100 and (sl & (ref.kind == R.DIFFUSE) & ~ref.black).sum() >= 40
    # lobe boundary: w_spec == 0.5 * total exactly, in float64
    lb = fam == "lobe_boundary"
    assert (lb & (ref.margin == 0) & (case["xi"][:, 0] == 0.5) & (ref.lobe != R.DIFFUSE)).sum() >= 100
    for x in (0.5 + R.EPS24, 0.5 - R.EPS24, 0.0, 1 - R.EPS24):
        assert (lb & (case["xi"][:, 0] == np.float32(x))).sum() >= 8
    assert set(ref.lobe[lb & (case["xi"][:, 0] == R.ONE_BELOW)]) == {R.DIFFUSE}
    # ends of the random numbers, on each lobe
    xe = fam == "xi_edges"
    for lobe in (R.DIFFUSE, R.PHONG, R.MIRROR):
        for a in R.XI_EDGES:
            for b in R.XI_EDGES:
                assert (xe & (ref.lobe == lobe) & (case["xi"][:, 1] == np.float32(a)) & (case["xi"][:, 2] == np.float32(b))).sum() >= 2


def test_light_edge_inputs(pkg):
    """The light inputs hold what they promise on the scenes of the device test: a light index that needs the clamp, every k / n boundary, u + v
    exactly 1 and one ulp above, in-plane points."""
    for scene, n_lights in ((pkg.scenes.cornell_box_small(64, 64), 2), (R.nine_light_scene(pkg), 9)):
        p, xi, fam = R.light_edge_inputs(scene)
        lf = R.light_faces(scene)
        assert len(lf) == n_lights and p.dtype == np.float64 and xi.dtype == np.float32 and 100 < len(p) < 5000
        assert set(fam) == {"index", "fold", "near", "in_plane", "far"}
        idx, clamped = R.light_index(xi[:, 0], n_lights)
        assert set(idx) == set(range(n_lights))
        assert clamped.any() and np.array_equal(clamped, xi[:, 0] == 1)            # below 2^24 lights the clamp acts at xi_l = 1 alone
        for k in range(1, n_lights):
            assert (xi[:, 0] == np.float32(k) / np.float32(n_lights)).any()
        s = xi[:, 1] + xi[:, 2]
        f = fam == "fold"
        assert (s[f] == 1).any() and (s[f] == np.nextafter(np.float32(1), np.float32(2))).any() and ((xi[f, 1] == 0) & (xi[f, 2] == 0)).any()
        assert (xi[:, 0] == R.ONE_BELOW).any() and xi[:, 0].max() == 1 and xi[:, 0].min() == 0
