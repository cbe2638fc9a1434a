"""No GPU: what tests/ploc_ref.py -- the numpy restatement of the device tree builder (csrc/bvh_gpu.hip) -- says about ties, chains and tiny
scenes, and that the ray sets of the GPU suite are ones an fp32 triangle test can be held to.

The finding these tests pin.  With the tie rule the kernel had (`tie="lower"`: among equal merged areas the lower index), a run of equal boxes
merged ONE pair per round: coincident(300) 299 rounds to depth 298, coincident(5000) 4999 rounds (depth 4998 -- but the builder stops after 4096
and the context was refused), a strip of unit quads n/4 rounds, the awkward-geometry scene of tests/test_gpu_bvh_build.py 431 rounds to depth
416 -- so that test validated and traced the HOST tree its context fell back to.  With the rule it has now (`tie="pair"`: the partner i ^ 1 among
equal areas, else the lower index) the same inputs take 9 .. 45 rounds and stay at most 26 deep; inputs without ties keep their rounds and depth.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import kit, ploc_ref as P


def _figures(scene, tie, capped=False):
    r = P.predict(scene, tie) if capped else P.build(P.scene_boxes(scene), tie)
    return r["rounds"], r["depth"]


@pytest.mark.parametrize("maker,n,lower,pair", [
    ("coincident", 300, (299, 298), (9, 8)),
    ("strip", 256, (136, 8), (9, 8)),                          # 512 triangles
    ("strip", 1024, (522, 10), (11, 10)),                      # 2048 triangles
    ("grid", 64, (45, 12), (13, 12)),                          # 8192 triangles
])
def test_equal_areas_chained_under_the_old_tie_rule_and_pair_up_under_the_new(pkg, maker, n, lower, pair):
    scene = getattr(P, maker)(pkg, n)
    assert _figures(scene, "lower") == lower
    assert _figures(scene, "pair") == pair


def test_the_awkward_geometry_scene_was_too_deep_for_any_context_under_the_old_rule(pkg):
    scene = P.awkward(pkg)[0]
    assert scene.face.shape[0] == 3012
    assert _figures(scene, "lower") == (431, 416)              # > 255: discarded, the host builder's tree was what the GPU test saw
    rounds, depth = _figures(scene, "pair")
    assert rounds <= 60 and depth <= 63, (rounds, depth)       # (not an exact-arithmetic input: 45 rounds, depth 26 without contraction)


def test_many_coincident_triangles_passed_the_round_cap_under_the_old_rule(pkg):
    scene = P.coincident(pkg, 5000)
    old = P.build(P.scene_boxes(scene), "lower")                # carried to its end, past where the device stops
    assert old["gave_up"] and old["rounds"] > P.MAX_ROUNDS
    assert (old["rounds"], old["depth"], old["n_nodes"]) == (4999, 4998, 4998)
    new = P.predict(scene, "pair")
    assert (new["gave_up"], new["rounds"], new["depth"]) == (False, 13, 12)
    new = P.predict(P.strip(pkg, 9000), "pair")                 # old rule: 4516 rounds
    assert (new["gave_up"], new["rounds"], new["depth"]) == (False, 17, 14)


def test_inputs_without_ties_keep_their_rounds_and_depth(pkg):
    rng = np.random.default_rng(5)
    c = rng.uniform(0, 1, (8192, 3)); e = rng.uniform(0.001, 0.02, (8192, 3))
    boxes = np.concatenate([c - e, c + e], 1).astype(np.float32)
    a, b = P.build(boxes, "lower"), P.build(boxes, "pair")
    assert a == b and not a["gave_up"]
    assert (a["rounds"], a["depth"], a["n_nodes"]) == (34, 16, 4896)   # seeded input, fp32 without contraction: exact figures


@pytest.mark.parametrize("n", [3, 4, 5, 8, 9, 16, 17, 33, 255, 256, 257, 272, 273, 513, 4099])
def test_small_soups_build_a_sound_shape(pkg, n):
    """The sizes the GPU suite compares with the device: every one gives a tree, of n - 1 merges, whose emitted inner nodes lie between the
    fewest (every leaf full) and the most (every leaf one triangle) a tree of <= 2-triangle leaves can have."""
    scene = P.lattice_soup(pkg, n)
    b = P.scene_boxes(scene)
    assert b.shape == (n, 6) and np.array_equal(b, np.round(2 * b) / 2)                    # half-integers: exact in fp32
    ext = b[:, 3:] - b[:, :3]
    assert ext.min() >= 1 and ext.max() <= 4
    r = P.predict(scene)
    assert not r["gave_up"] and 1 <= r["max_leaf"] <= 2
    assert (n + 1) // 2 - 1 <= r["n_nodes"] <= n - 1 and 1 <= r["depth"] <= r["n_nodes"]


def test_morton_codes_and_boxes_of_a_known_case(pkg):
    """Three boxes whose centres span [0, 1] on x only: codes 0, the middle of the range and its end on the x bits alone; boxes rounded outward."""
    b = np.array([[0, 0, 0, 0, 0, 0], [0.5, 0, 0, 0.5, 0, 0], [1, 0, 0, 1, 0, 0]], np.float32)
    x = [int(c) for c in P.morton_codes(b)]
    def spread(v): return sum(((v >> k) & 1) << (3 * k + 2) for k in range(21))
    assert x == [0, spread(1 << 20), spread((1 << 21) - 1)]
    s = pkg.scenes
    v = np.array([[0.1, 0.2, 0.3], [1.1, 0.7, 0.3], [0.4, 1.3, 0.9]])
    f = np.zeros((1, 3, 4), np.int32); f[0, :, 0] = [0, 1, 2]
    box = P.scene_boxes(s.SceneData("one", v, np.array([[0, 0, 1.0]]), np.zeros((1, 2)), f, [s.Material("m")], s.Camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 4, 4)))[0]
    ctr = 0.5 * v.min(0) + 0.5 * v.max(0)
    assert (box[:3].astype(np.float64) <= v.min(0) - ctr).all() and (box[3:].astype(np.float64) >= v.max(0) - ctr).all()
    assert (np.nextafter(box[:3], np.float32(np.inf)).astype(np.float64) > v.min(0) - ctr).all()


@pytest.mark.parametrize("n,ratio,band", [(40, 1.5, (1, 63)), (150, 1.2, (64, 255)), (300, 1.15, (256, 10 ** 9))])
def test_shells_reach_the_three_depth_bands(pkg, n, ratio, band):
    """Nested shells chain under either tie rule (depth n - 2): kept by every context, kept by a wavefront context only, discarded by all."""
    scene = P.shells(pkg, n, ratio)
    for tie in ("lower", "pair"):
        r = P.predict(scene, tie)
        assert not r["gave_up"] and r["depth"] == n - 2 and band[0] <= r["depth"] <= band[1], (tie, r)


def test_enough_shells_pass_the_round_cap(pkg):
    r = P.predict(P.shells(pkg, 5000, 1.005))
    assert r["gave_up"] and r["rounds"] > P.MAX_ROUNDS, r


@pytest.mark.parametrize("name", sorted(P.HIT_SCENES))
def test_the_ray_sets_are_ones_fp32_can_answer(pkg, name):
    """The GPU suite asks a device context for the fp64 brute force's hit/miss on >= 99.9 % of these rays and its t to rtol 2e-5, atol 2e-6.  The
    same triangle test in plain fp32 numpy -- no tree, no fused multiply-add -- keeps both with margin: hit/miss on >= 99.95 %, t on every ray."""
    scene, o, d, t64, f64 = P.hit_case(pkg, name)
    assert o.shape == (P.N_RAYS_OF.get(name, P.N_RAYS), 3) and 0.2 <= (f64 >= 0).mean() <= 0.9               # hundreds of hits and of misses
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0)
    t32, f32, _, _ = kit.brute_force_trace(scene, o, d, np.float32)
    same = (f32 >= 0) == (f64 >= 0)
    both = (f32 >= 0) & (f64 >= 0)
    print("%s: hit share %.3f, fp32 agrees on hit/miss for %.4f, max |t32 - t64| / t64 = %.2e" % (
        name, (f64 >= 0).mean(), same.mean(), float(np.max(np.abs(t32[both] - t64[both]) / t64[both]))))
    assert same.mean() >= 0.9995
    assert np.allclose(t32[both], t64[both], rtol=2e-5, atol=2e-6)
    if not name.startswith("coincident"):
        assert (f32[both] == f64[both]).mean() >= 0.9995
