"""Every probed path against the oracle's event log, none forgiven (the scene, the ray families, the perturbation family and the
verdict are tests/path_ref.py's).

The state machine of wf_shade_kernel -- class sort, emitter MIS, roulette, NEE and shadow-queue hand-off, SLOT_DRAIN, item regeneration, film write --
is held to the fp64 oracle path by path: a path whose event sequence the oracle's own perturbation family does not change ("decided") must meet
max(1e-4 max(1, |L|), S_i) per channel, S_i being the largest change of L inside that family; the others must be finite and not below zero (or
the family's own lowest answer).  No share is forgiven.  MCPT_FLAG_CORRECT_SHADOW_T2 is set throughout: without it the reference's self-occlusion
verdict is fp64 noise by design (SURVEY A-9), which test_self_occlusion_rate_matches_oracle covers statistically.

CPU part (no GPU): for every depth of 1, 2, 4, 5, 6 and 0 over the whole list of 12 900 rays -- undecided paths <= 5 %, paths with S_i above the
1e-4 bound <= 2 %, every event kind the depth can reach >= 200 times among decided paths.  Measured (this list, this oracle):
    depth        1      2      4      5      6      0
    undecided  2.43   3.61   4.36   4.64   4.67   4.74  %
    S_i > 1e-4 0.16   0.74   1.36   1.52   1.66   1.88  %
One kind cannot occur on a decided path and is counted over the whole list instead: the light sample without a pdf.  Its cosine must be 0.0f
exactly, which happens where a vertex lies on the light it samples, and every shift of the vertex off that plane turns the verdict over.

GPU part: the figures measured on an MI355X are in DESIGN.md section 26.
"""
import os

import numpy as np
import pytest

from tests import path_ref as pr
from tests.kit import bits


@pytest.fixture(scope="session")
def world(pkg, orc):
    """The scene, the ray list and the oracle's judgement per depth: built once for the CPU and the GPU tests."""
    scene = pr.events_scene(pkg)
    fams = pr.ray_families()
    o = np.concatenate([f[1] for f in fams]); d = np.concatenate([f[2] for f in fams])
    fam = np.concatenate([[f[0]] * len(f[1]) for f in fams])
    flags = pkg.FLAG_CORRECT_SHADOW_T2
    oracle = orc.Oracle(scene, flags=flags)
    judged = {depth: pr.judge(oracle, scene, o, d, depth, flags, fam) for depth in pr.DEPTHS}
    emissive = np.array([np.linalg.norm(scene.materials[m].radiance) != 0 for m in scene.face[:, 0, 3]])
    for j in judged.values():
        for a in (j.L, j.ev, j.decided, j.S, j.allow, j.low):
            a.setflags(write=False)
    return dict(scene=scene, o=o, d=d, fam=fam, flags=flags, oracle=oracle, judged=judged, emissive=emissive)


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_scene_is_what_the_families_need(world, orc):
    scene = world["scene"]
    info = world["oracle"].info()
    assert info["tris"] == 170 and len(scene.materials) == 21 and info["lights"] == 26          # > WF_LDS_MATS = 16, > WF_LDS_LIGHTS = 8
    faint = [m for m in scene.materials if m.name == "faint"][0]
    assert 1e-4 < np.linalg.norm(faint.radiance) < 0.01
    # grazing: the first hit is the floor, at a cosine between 1e-3 and 1e-1
    g = world["fam"] == "grazing"
    assert np.all((-world["d"][g][:, 1] >= 1e-3 * (1 - 1e-9)) & (-world["d"][g][:, 1] <= 1e-1 * (1 + 1e-9)))
    first = world["judged"][1].ev[g][:, 2] >> 8
    assert (np.isin(first, np.arange(8))).mean() > 0.9                                           # the floor's eight faces (the sphere hides some)


def test_log_and_zero_perturbation_are_bit_equal_to_the_plain_oracle(world, orc):
    o, d = world["o"], world["d"]
    oracle = world["oracle"]
    pick = np.arange(0, len(o), 7)
    for depth in pr.DEPTHS:
        oracle.set_opts(max_depth=depth, integrator=0, flags=world["flags"])
        j = world["judged"][depth]
        plain = np.array([oracle.trace_path_counter(o[i], d[i], int(i), pr.SEED) for i in pick])
        assert np.array_equal(bits(plain), bits(j.L[pick])), depth
        unlogged, none = oracle.trace_paths_log(o, d, seed=pr.SEED, log=False)
        assert none is None and np.array_equal(bits(unlogged), bits(j.L))
        zero, ev = oracle.trace_paths_log(o, d, seed=pr.SEED, dp=0.0, dd=0.0, db=0.0, axis=3, member=9)
        assert np.array_equal(bits(zero), bits(j.L)) and np.array_equal(ev, j.ev)
        # first_item shifts the key, nothing else
        part, evp = oracle.trace_paths_log(o[100:164], d[100:164], seed=pr.SEED, first_item=100)
        assert np.array_equal(bits(part), bits(j.L[100:164])) and np.array_equal(evp, j.ev[100:164])


def test_every_member_restates_a_documented_freedom(world):
    m = pr.members(1.0)
    assert len(m) == 6 + pr.N_HASHED + 3 and sorted(k["axis"] for k in m[:6]) == list(range(6))
    assert all(k.get("dp", 0.0) in (0.0, 2.0 ** -20) and k.get("dd", 0.0) in (0.0, pr.DD) and k.get("db", 0.0) in (0.0, 2.0 ** -20) for k in m)
    assert abs(pr.DD - 1.91e-6) < 1e-8


@pytest.mark.parametrize("depth", pr.DEPTHS)
def test_conditions_on_the_list(world, depth):
    j = world["judged"][depth]
    n = len(j.L)
    undecided, sensitive = float((~j.decided).mean()), float((j.decided & j.sensitive).mean())
    counts = pr.event_counts(j.ev, world["emissive"], j.decided)
    whole = pr.event_counts(j.ev, world["emissive"], np.ones(n, bool))
    print("depth %d: %d paths, undecided %.2f %%, S above the bound %.2f %%, worst S among decided %.3g" % (depth, n, 100 * undecided, 100 * sensitive, j.S[j.decided].max()))
    print("  decided: " + ", ".join("%s %d" % kv for kv in counts.items()))
    for f, _ in pr.FAMILIES:
        sel = world["fam"] == f
        print("  %-10s %5d paths, undecided %.2f %%, S above the bound %.2f %%" % (f, sel.sum(), 100 * (~j.decided[sel]).mean(), 100 * (j.decided & j.sensitive)[sel].mean()))
    assert undecided <= pr.MAX_UNDECIDED
    assert sensitive <= pr.MAX_SENSITIVE
    counts["nee_nopdf"] = whole["nee_nopdf"]                       # cannot be decided: module docstring
    short = {k: counts[k] for k in pr.required_kinds(depth) if counts[k] < pr.MIN_EVENTS}
    assert short == {}, short
    assert np.all(np.isfinite(j.L[j.decided]))


@pytest.mark.parametrize("depth", [k for k in pr.DEPTHS if k != 0])          # (an unbounded path has no next depth)
def test_checker_fails_on_a_depth_off_by_one(world, depth):
    j = world["judged"][depth]
    oracle = world["oracle"]
    oracle.set_opts(max_depth=depth + 1, integrator=0, flags=world["flags"])
    deeper, _ = oracle.trace_paths_log(world["o"], world["d"], seed=pr.SEED, log=False)
    bad, _, _ = pr.check(j, deeper)
    assert j.decided[bad].sum() > 0; print("depth %d presented as %d: %d decided paths fail" % (depth + 1, depth, j.decided[bad].sum()))
    own, _, _ = pr.check(j, j.L)
    assert len(own) == 0                                           # ... and passes the oracle's own answers


@pytest.mark.parametrize("depth", pr.DEPTHS)
def test_checker_fails_on_a_scale_error_and_on_one_zeroed_path(world, depth):
    j = world["judged"][depth]
    bad, _, _ = pr.check(j, j.L.astype(np.float64) * (1 + 3e-4))
    assert len(bad) > 0
    # one decided path, the one with the SMALLEST radiance that is still above its allowance, set to zero
    big = np.nonzero(j.decided & np.any(np.abs(j.L64) > j.allow, axis=1))[0]
    i = big[np.argmin(np.abs(j.L64[big]).max(1))]
    got = j.L.copy(); got[i] = 0
    bad, _, _ = pr.check(j, got)
    assert bad.tolist() == [i]
    assert "path %d (%s)" % (i, world["fam"][i]) in pr.message(j, got, bad) and pr.describe(j.ev[i]) in pr.message(j, got, bad)
    # an undecided path may differ, but not be NaN or negative
    u = np.nonzero(~j.decided & (j.low.min(1) > -1e-3))[0][0]
    got = j.L.copy(); got[u] = np.nan
    assert pr.check(j, got)[0].tolist() == [u]
    got[u] = -1.0
    assert pr.check(j, got)[0].tolist() == [u]


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _context(pkg, scene, depth, flags, env=None):
    env = env or {}
    os.environ.update(env)
    try:
        return pkg.Renderer(scene, max_depth=depth, flags=flags)
    finally:
        for k in env:
            os.environ.pop(k, None)


@pytest.fixture(scope="session")
def device_answers(pkg, world):
    """probe_paths of the whole list per (pipeline, tree, depth), computed once: {(pipeline, tree, depth): L}."""
    cache = {}

    def get(pipeline, tree, depth):
        key = (pipeline, tree, depth)
        if key not in cache:
            flags = world["flags"] | (pkg.FLAG_GPU_BVH_BUILD if tree == "device" else 0)
            r = _context(pkg, world["scene"], depth, flags, {"MCPT_PIPELINE": "mega"} if pipeline == "mega" else None)
            try:
                cache[key] = r.probe_paths(world["o"], world["d"], seed=pr.SEED)
            finally:
                r.close()
            cache[key].setflags(write=False)
        return cache[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("depth", pr.DEPTHS)
@pytest.mark.parametrize("pipeline,tree", [("wave", "host"), ("mega", "host"), ("wave", "device")])
def test_every_decided_path_meets_its_allowance(world, device_answers, pipeline, tree, depth):
    j = world["judged"][depth]
    got = device_answers(pipeline, tree, depth)
    bad, ratio, rel = pr.check(j, got)
    print("%s pipeline, %s tree, depth %d: worst deviation / allowance, worst deviation / max(1, |L|) among decided paths" % (pipeline, tree, depth))
    for f, n, und, worst, worst_rel in pr.family_table(j, ratio, rel):
        print("  %-10s %5d paths, %4d undecided, %.3f of the allowance, %.3g" % (f, n, und, worst, worst_rel))
    assert len(bad) == 0, pr.message(j, got, bad)


SCHEDULES = {"pool-4096": {"MCPT_WF_POOL_SLOTS": "4096"}, "grid-1": {"MCPT_WF_GRID": "1"}}


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [5, 0])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("tree", ["host", "device"])
def test_scheduling_does_not_show(pkg, world, device_answers, tree, schedule, depth):
    """The first 6000 rays through a pool of 4096 slots (items regenerated into used slots), and through one trace block: bit for bit what the default
    context returns for the same rays."""
    n = 6000
    want = device_answers("wave", tree, depth)[:n]
    r = _context(pkg, world["scene"], depth, world["flags"] | (pkg.FLAG_GPU_BVH_BUILD if tree == "device" else 0), SCHEDULES[schedule])
    try:
        got = r.probe_paths(world["o"][:n], world["d"][:n], seed=pr.SEED)
    finally:
        r.close()
    diff = np.nonzero(np.any(bits(got) != bits(want), axis=1))[0]
    assert diff.size == 0, "%d of %d paths differ, first %d: %r vs %r, %s" % (diff.size, n, diff[0], got[diff[0]], want[diff[0]], pr.describe(world["judged"][depth].ev[diff[0]]))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [5, 0])
@pytest.mark.parametrize("tree", ["host", "device"])
def test_a_cut_list_returns_the_same_paths(pkg, world, device_answers, tree, depth):
    want = device_answers("wave", tree, depth)
    r = _context(pkg, world["scene"], depth, world["flags"] | (pkg.FLAG_GPU_BVH_BUILD if tree == "device" else 0))
    try:
        for n in (1, 255, 257, 4097):
            got = r.probe_paths(world["o"][:n], world["d"][:n], seed=pr.SEED)
            diff = np.nonzero(np.any(bits(got) != bits(want[:n]), axis=1))[0]
            assert diff.size == 0, "first %d rays: %d paths differ, first %d: %r vs %r" % (n, diff.size, diff[0], got[diff[0]], want[diff[0]])
    finally:
        r.close()
