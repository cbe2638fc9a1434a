"""Morph targets on the device: mcpt_set_vertex_morph, mcpt_update_morph (csrc/morph.hip in front of the refit, alone or in front
of the skin), mcpt_update_morph_reproject, mcpt_get_morph_info, mcpt_probe_vertices and their public surfaces.

The reference throughout is tests/morph_ref.py (numpy, the kernels' order of summation): fp64 multiply, add, divide and sqrt are correctly
rounded on both sides, so everything is compared BIT FOR BIT, without a tolerance -- directly, through mcpt_probe_vertices, and downstream
through §16's oracle: a second context of the same scene moved with mcpt_update_vertices to the restated arrays.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from tests import deform_kit as K, kit, morph_ref as M, skin_ref as S, transform_ref as T
from tests.deform_kit import CENTRE, FLAGS, H, INVALID, LAMP, M_HIGH, M_LAMP, M_LOW, N_BONES, SPHERE, UNSUPPORTED, W, clean
from tests.kit import bits, render_film

NEW_SYMBOLS = ["mcpt_set_vertex_morph", "mcpt_update_morph", "mcpt_update_morph_reproject", "mcpt_get_morph_info", "mcpt_probe_vertices"]
N_TARGETS = 5
WEIGHTS = np.array([-0.2, 0.7, 0.6, 0.0, 1.25])                              # mixed signs, one exactly 0 (on a target WITH entries), one > 1
WEIGHTS2 = np.array([-0.1, -0.5, -3.0, 0.9, 0.5])
ZERO = np.zeros(N_TARGETS)
BEND = K.mats(low=M_LOW, high=M_HIGH, lamp=M_LAMP)                           # §18's bend: 0 the walls, 1 and 2 the sphere's bones, 3 nobody, 4 the lamp


@functools.lru_cache(maxsize=None)
def _targets(pkg):
    """The five-target fixture, the same index sets for the vertices and for the normals (the sphere's corners pair vertex i with normal i):
    0 dense over the sphere (a swell about its centre), 1 sparse over the cap y > 0.45, 2 EMPTY, 3 every 7th sphere vertex, 4 the lamp's vertices.
    The normal targets carry random deltas of their own.  (vertex targets, normal targets.)"""
    s = K.scene(pkg); sphere, lamp = K.parts(pkg)
    rng = np.random.default_rng(31)
    si = np.flatnonzero(sphere); li = np.flatnonzero(lamp)
    sets = [si, si[s.vertex[si, 1] > 0.45], np.zeros(0, np.int64), si[::7], li]
    vd = [s.vertex[si] - CENTRE, rng.uniform(-0.02, 0.02, (len(sets[1]), 3)), np.zeros((0, 3)), rng.uniform(-0.01, 0.01, (len(sets[3]), 3)),
          np.tile((0.08, -0.15, 0.04), (len(li), 1))]
    nd = [rng.uniform(-0.3, 0.3, (len(i), 3)) for i in sets]
    return list(zip(sets, vd)), list(zip(sets, nd))


def _ref(pkg, weights, bones=None, rest=None, targets=None):
    """The arrays the weights (and bones) give, by the restatement."""
    s = K.scene(pkg); vt, nt = _targets(pkg) if targets is None else targets
    rv, rn = (s.vertex, s.normal) if rest is None else rest
    if bones is None:
        return M.morph_vertices(rv, vt, weights), M.morph_normals(rn, nt, weights)
    return M.morph_then_skin(rv, rn, vt, nt, weights, K.bend(pkg), bones)


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_morph_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, ("set_vertex_morph", "update_morph", "update_morph_reproject", "morph_info", "vertices"))
    assert set(pkg.MorphInfo().as_dict()) == {"struct_size", "n_targets", "updates", "vertex_entries", "normal_entries", "last_ms"}
    assert pkg.MORPH_MAX_TARGETS == M.MAX_TARGETS == 65536


def test_null_context_is_an_invalid_argument_for_the_morph_calls(pkg):
    lib = pkg.load_library()
    cam = pkg.CameraC(); info = pkg.MorphInfo()
    o = pkg.ReprojectOpts(); o.struct_size = C.sizeof(pkg.ReprojectOpts)
    t, keep = pkg.targets_struct([(np.array([0]), np.zeros((1, 3)))])
    w = np.zeros(1); wp = w.ctypes.data_as(C.c_void_p); m = T.identity(1); mp = m.ctypes.data_as(C.c_void_p)
    out = np.zeros(12); op = out.ctypes.data_as(C.c_void_p)
    assert lib.mcpt_set_vertex_morph(None, C.byref(t), 4, C.byref(t), 4) == INVALID
    assert lib.mcpt_set_vertex_morph(None, C.byref(t), 4, None, 4) == INVALID
    assert lib.mcpt_update_morph(None, wp, 1, None, 0) == INVALID and lib.mcpt_update_morph(None, wp, 1, mp, 1) == INVALID
    assert lib.mcpt_update_morph_reproject(None, wp, 1, None, 0, None, None) == INVALID
    assert lib.mcpt_update_morph_reproject(None, wp, 1, mp, 1, C.byref(cam), C.byref(o)) == INVALID
    assert lib.mcpt_get_morph_info(None, C.byref(info)) == INVALID
    assert lib.mcpt_probe_vertices(None, op, op) == INVALID


def test_morph_structs_have_the_headers_layout(pkg, tmp_path):
    """sizeof and every offsetof of mcpt_morph_targets and mcpt_morph_info as a C compiler sees include/mcpt.h, against the ctypes classes."""
    for cls, name, size in ((pkg.MorphTargets, "mcpt_morph_targets", 48), (pkg.MorphInfo, "mcpt_morph_info", 56)):
        c, py, _ = K.c_layout(cls, name, tmp_path)
        assert c == py and c[0] == size


def test_flattening_of_a_target_list(pkg):
    vt, nt = _targets(pkg)
    off, idx, dlt = pkg.flatten_targets(vt)
    assert off.dtype == idx.dtype == np.uint32 and dlt.dtype == np.float64 and dlt.shape == (idx.shape[0], 3)
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(i) for i, _ in vt])]).tolist() and off[2] == off[3]      # target 2 is empty
    for k, (i, d) in enumerate(vt):
        assert np.array_equal(idx[off[k]:off[k + 1]], i) and np.array_equal(bits(dlt[off[k]:off[k + 1]]), bits(d))
    t, keep = pkg.targets_struct(vt)
    assert (t.struct_size, t.n_targets) == (C.sizeof(pkg.MorphTargets), N_TARGETS) and [t.target_offset[k] for k in range(N_TARGETS + 1)] == off.tolist()
    assert t.index[int(off[1])] == idx[off[1]] and t.delta[3 * int(off[1]) + 2] == dlt[off[1], 2]
    # nothing is sorted or merged: what the caller gives is what the library judges
    off, idx, dlt = pkg.flatten_targets([([5, 3], np.ones((2, 3))), ([], np.zeros((0, 3)))])
    assert off.tolist() == [0, 2, 2] and idx.tolist() == [5, 3]
    t, keep = pkg.targets_struct([([], np.zeros((0, 3)))])                    # no entries at all: NULL arrays, one offset pair
    assert not t.index and not t.delta and [t.target_offset[0], t.target_offset[1]] == [0, 0]
    for bad in ([([1, 2], np.zeros((3, 3)))], [([-1], np.zeros((1, 3)))], [([2 ** 32], np.zeros((1, 3)))]):
        with pytest.raises(ValueError):
            pkg.flatten_targets(bad)


def test_the_fixture_is_what_the_suite_says(pkg):
    s = K.scene(pkg); sphere, lamp = K.parts(pkg); vt, nt = _targets(pkg)
    assert s.vertex.shape[0] == s.normal.shape[0] == 1249 and sphere.sum() == 1223 and lamp.sum() == 4
    assert np.array_equal(s.face[s.face[:, 0, 3] == SPHERE][:, :, 0], s.face[s.face[:, 0, 3] == SPHERE][:, :, 1])   # vertex i with normal i
    sizes = [len(i) for i, _ in vt]
    assert sizes[0] == 1223 and 0 < sizes[1] < 400 and sizes[2] == 0 and sizes[3] == 175 and sizes[4] == 4
    off, target, delta = M.per_record(vt, 1249)
    per = np.diff(off.astype(np.int64))
    assert per.max() == 3 and (per == 0).sum() == 1249 - 1223 - 4 and (per[~sphere & ~lamp] == 0).all()
    assert not np.signbit(s.vertex[s.vertex == 0.0]).any() and np.signbit(s.normal[s.normal == 0.0]).sum() == 48
    assert M.accepts_targets(vt, 1249) and M.accepts_targets(nt, 1249, N_TARGETS)
    for w in (WEIGHTS, WEIGHTS2):
        v, n = _ref(pkg, w)
        assert v[sphere].min() > 0.005 and v[sphere].max() < 0.995 and v[lamp].min() > 0.005 and v[lamp].max() < 0.995      # inside the room
        assert np.array_equal(bits(v[~sphere & ~lamp]), bits(s.vertex[~sphere & ~lamp]))                                 # the walls stay
    used = T.used_vertices(s)
    assert (~used).sum() == 2 and not (~used & (sphere | lamp)).any()      # two vertices that no face uses: R and D_k skip them


def test_restatement_properties(pkg):
    s = K.scene(pkg); vt, nt = _targets(pkg); sphere, lamp = K.parts(pkg)
    nv = s.vertex.shape[0]
    # no entries at all: every record is copied, normals included (not normalised)
    none = [(np.zeros(0, int), np.zeros((0, 3)))] * 3
    assert np.array_equal(bits(M.morph_vertices(s.vertex, none, [1.0, -2.0, 0.0])), bits(s.vertex))
    assert np.array_equal(bits(M.morph_normals(s.normal, none, [1.0, -2.0, 0.0])), bits(s.normal))
    assert np.array_equal(bits(M.morph_normals(s.normal, None, [1.0])), bits(s.normal))
    # one dense target with weight 1: rest + delta in one rounding
    dense = [(np.arange(nv), np.random.default_rng(1).uniform(-1, 1, (nv, 3)))]
    assert np.array_equal(bits(M.morph_vertices(s.vertex, dense, [1.0])), bits(s.vertex + dense[0][1]))
    # the per-target loop is the per-record walk in stored order, bit for bit -- vertices and normals, both weight sets
    for w in (WEIGHTS, WEIGHTS2, ZERO):
        assert np.array_equal(bits(M.morph_vertices(s.vertex, vt, w)), bits(M.morph_by_records(s.vertex, vt, w)))
        assert np.array_equal(bits(M.morph_normals(s.normal, nt, w)), bits(M.morph_by_records(s.normal, nt, w, normalise=True)))
    # two targets commute only up to rounding: the fixed order (ascending target id) is what is pinned
    rng = np.random.default_rng(2)
    a = (np.arange(nv), rng.uniform(-1, 1, (nv, 3))); b = (np.arange(nv), rng.uniform(-1, 1, (nv, 3)))
    ab = M.morph_vertices(s.vertex, [a, b], [0.3, 0.7]); ba = M.morph_vertices(s.vertex, [b, a], [0.7, 0.3])
    assert not np.array_equal(bits(ab), bits(ba)) and np.abs(ab - ba).max() <= 4 * np.finfo(np.float64).eps
    off, target, delta = M.per_record([a, b], nv)
    assert off.tolist() == (2 * np.arange(nv + 1)).tolist() and target.tolist() == [0, 1] * nv
    off, target, delta = M.per_record(vt, nv)
    for i in np.flatnonzero(np.diff(off.astype(np.int64)) > 1):
        assert (np.diff(target[off[i]:off[i + 1]].astype(np.int64)) > 0).all()          # ascending target id inside a record
    # all weights 0: the vertices (no -0.0 among them) are the rest pose bit for bit; the normals only by value -- -0 + 0 d = +0 -- and the
    # touched ones are normalised
    assert np.array_equal(bits(M.morph_vertices(s.vertex, vt, ZERO)), bits(s.vertex))
    zn = M.morph_normals(s.normal, nt, ZERO)
    assert np.array_equal(bits(zn[~sphere & ~lamp]), bits(s.normal[~sphere & ~lamp])) and not np.array_equal(bits(zn), bits(s.normal))
    assert np.abs(zn - s.normal).max() < 1e-8
    # a weight of 0 is accumulated: -0.0 in the rest pose becomes +0.0 where an entry touches it
    neg = np.array([[-0.0, 1.0, -0.0]]); one = [(np.array([0]), np.array([[3.0, 0.0, -2.0]]))]
    out = M.morph_vertices(neg, one, [0.0])
    assert not np.signbit(out[0, 0]) and np.signbit(out[0, 2]) and np.signbit(M.morph_vertices(neg, [(np.zeros(0, int), np.zeros((0, 3)))], [0.0])[0, 0])
    # normals: touched records come out unit length, a zero sum is left as it is
    n = M.morph_normals(s.normal, nt, WEIGHTS)
    touched = sphere | lamp
    assert np.abs(np.sqrt((n[touched] ** 2).sum(1)) - 1.0).max() <= 4 * np.finfo(np.float64).eps
    flat = M.morph_normals(np.array([[0.0, 1.0, 0.0]]), [(np.array([0]), np.array([[0.0, -1.0, 0.0]]))], [1.0])
    assert np.array_equal(flat, np.zeros((1, 3)))
    # the pose the ordering tests start from is a fixed point of the normalisation in the fp32 numbers the shading streams hold
    rv, rn = K.unit_rest(pkg, positive_zero=True)
    again = M.morph_normals(rn, nt, ZERO)
    assert np.array_equal(bits(again.astype(np.float32)), bits(rn.astype(np.float32))) and not np.signbit(rn[rn == 0.0]).any()
    # morph, then skin: skin_ref on morph_ref's output, and it differs from either alone
    v2, n2 = _ref(pkg, WEIGHTS, BEND)
    v1, n1 = _ref(pkg, WEIGHTS)
    vb, vw, nb, nw = K.bend(pkg)
    assert np.array_equal(bits(v2), bits(S.skin_vertices(v1, vb, vw, BEND))) and np.array_equal(bits(n2), bits(S.skin_normals(n1, nb, nw, BEND)))
    assert not np.array_equal(v2, v1) and not np.array_equal(v2, S.skin_vertices(s.vertex, vb, vw, BEND))


def test_restatement_refusals(pkg):
    s = K.scene(pkg); vt, nt = _targets(pkg); nv = s.vertex.shape[0]
    assert not M.accepts_targets([], nv) and not M.accepts_targets(vt, nv, N_TARGETS + 1)
    assert M.accepts_targets([(np.zeros(0, int), np.zeros((0, 3)))] * 65536, nv) and not M.accepts_targets([(np.zeros(0, int), np.zeros((0, 3)))] * 65537, nv)

    def with_target(k, index=None, delta=None):
        t = list(vt); t[k] = (vt[k][0] if index is None else index, vt[k][1] if delta is None else delta)
        return t

    i4 = vt[4][0]
    assert not M.accepts_targets(with_target(4, index=np.array([i4[0], i4[1], i4[3], i4[2]])), nv)         # not ascending
    assert not M.accepts_targets(with_target(4, index=np.array([i4[0], i4[1], i4[1], i4[3]])), nv)         # a duplicate
    assert not M.accepts_targets(with_target(4, index=np.array([i4[0], i4[1], i4[2], nv])), nv)            # index >= the record count
    assert M.accepts_targets(with_target(4, index=np.array([i4[0], i4[1], i4[2], nv - 1])), nv)
    for bad, ok in ((np.nan, False), (np.inf, False), (-np.inf, False), (1.0000001e18, False), (-1e18, True), (1e18, True)):
        d = vt[1][1].copy(); d[3, 1] = bad
        assert M.accepts_targets(with_target(1, delta=d), nv) == ok, bad
    # R and D_k look at the vertices a face uses only
    used = np.ones(nv, bool)
    radius = M.rest_radius(s.vertex, used); dk = M.target_delta(vt, used)
    assert radius == np.abs(s.vertex).max() and dk[2] == 0.0 and dk[4] == 0.15 and dk[0] == np.abs(vt[0][1]).max() and (dk[[0, 1, 3, 4]] > 0).all()
    few = used.copy(); few[vt[4][0]] = False
    assert M.target_delta(vt, few)[4] == 0.0 and M.rest_radius(s.vertex, few) <= radius and M.rest_radius(s.vertex, np.zeros(nv, bool)) == 0.0
    # the reach: sequential from R, with the slack factor
    e = M.reach(radius, WEIGHTS, dk)
    want = radius
    for w, d in zip(WEIGHTS, dk):
        want = want + abs(w) * d
    assert e == (1.0 + 2.0 ** -16) * want and M.accepts(WEIGHTS, radius, dk) and M.accepts(WEIGHTS2, radius, dk)
    assert not M.accepts(WEIGHTS[:-1], radius, dk)
    for bad, ok in ((np.nan, False), (np.inf, False), (-1.0000001e18, False), (1e18, True), (-1e18, True)):
        w = WEIGHTS.copy(); w[2] = bad                                       # target 2 is empty: D_2 = 0, only the weight's own rule can refuse it
        assert M.accepts(w, radius, dk) == ok, bad
    w = WEIGHTS.copy(); w[4] = 1e18 / 0.15 * 1.01                           # finite and <= 1e18 itself? no: 6.7e18 -- refused as a weight
    assert not M.accepts(w, radius, dk)
    big = np.array([1e18]); assert not M.accepts([1.0], 0.5, big) and M.accepts([0.5], 0.5, big) and not M.accepts([1.0], 0.0, big)   # the slack alone
    assert M.accepts([1.0], 0.0, big / (1.0 + 2.0 ** -15))
    # with bones: skin_ref's checks with E as every bone's radius -- a far-away bone without members, fine for the skin alone, is refused
    vb, vw, nb, nw = K.bend(pkg)
    rb = S.bone_radius(s.vertex, vb, vw, used, N_BONES)
    far = K.mats(third=np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1e18, 0.0]]))
    assert rb[3] == 0.0 and S.accepts(far, rb) and not M.accepts(WEIGHTS, radius, dk, far, N_BONES) and M.accepts(WEIGHTS, radius, dk, BEND, N_BONES)
    assert not M.accepts(WEIGHTS, radius, dk, BEND[:-1], N_BONES)
    flat = K.mats(low=T.about(np.diag([1.0, 0.0, 1.0]), CENTRE)); nan = K.mats(); nan[1, 2, 1] = np.nan
    assert not M.accepts(WEIGHTS, radius, dk, flat, N_BONES) and not M.accepts(WEIGHTS, radius, dk, nan, N_BONES)


def _host_check_cases(pkg):
    """Target sets for morph_host_check: the fixture's, random ones, and the degenerate ones (no entries, no records, one target of everything)."""
    vt, nt = _targets(pkg)
    rng = np.random.default_rng(7)
    cases = [(vt, 1249), (nt, 1249), ([(np.zeros(0, int), np.zeros((0, 3)))], 0), ([(np.zeros(0, int), np.zeros((0, 3)))] * 4, 9),
             ([(np.arange(300), rng.normal(size=(300, 3)))], 300), ([(np.array([299]), np.array([[1e18, -1e18, 0.0]]))], 300)]
    for n_records, n_targets in ((1, 3), (257, 40), (1000, 7)):
        t = []
        for _ in range(n_targets):
            idx = np.flatnonzero(rng.uniform(size=n_records) < rng.uniform(0.0, 0.6))
            t.append((idx, rng.normal(size=(len(idx), 3)) * 10.0 ** rng.integers(-6, 7)))
        cases.append((t, n_records))
    out = []
    for k, (t, n_records) in enumerate(cases):
        w = rng.normal(size=len(t)) * 10.0 ** rng.integers(-3, 4, len(t)); d = np.abs(rng.normal(size=len(t))); radius = float(rng.uniform(0, 2))
        if k == 5:
            w, d, radius = np.array([1.0]), np.array([1e18]), 0.0             # at the limit: only the slack factor puts it over
        out.append((t, n_records, radius, w, d))
    return out


@K.needs_hipcc
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_conversion_and_reach_are_the_restatement_bit_for_bit(pkg, tmp_path, sanitized):
    """The host half of the feature -- mo_per_record and mo_reach of csrc/morph.hip -- built into the stand-alone program
    tests/morph_host_check.cpp (no device is touched) against tests/morph_ref.py: the same offsets, entry order, deltas and reach, bit for
    bit.  `sanitized`: the same program under the host's address and undefined-behaviour sanitizers, which must stay silent."""
    exe = K.build_host_check("morph_host_check", ["morph.hip"], tmp_path, sanitized)
    cases = _host_check_cases(pkg)
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for t, n_records, radius, w, d in cases:
            off, idx, dlt = pkg.flatten_targets(t)
            f.write(np.array([len(t), n_records], np.uint32).tobytes()); f.write(off.tobytes()); f.write(idx.tobytes()); f.write(dlt.tobytes())
            f.write(np.concatenate([[radius], w, d]).astype(np.float64).tobytes())
    K.run_host_check(exe, tmp_path, sanitized)
    raw = open(str(tmp_path / "out.bin"), "rb").read()
    at = 0
    for t, n_records, radius, w, d in cases:
        off, target, delta = M.per_record(t, n_records)
        total = len(target)
        for want in (off, target, delta.reshape(-1), np.array([M.reach(radius, w, d)])):
            got = np.frombuffer(raw, want.dtype, want.size, at); at += want.nbytes
            assert np.array_equal(bits(got), bits(np.ascontiguousarray(want))), (n_records, len(t), total)
    assert at == len(raw)
    assert M.reach(*cases[5][2:]) > 1e18


# ------------------------------------------------------------------------------------------------------------------------ GPU helpers
def _pair(pkg, extra=0, targets="fixture"):
    """The context under test (with the five-target fixture, or `targets`, or none) and its oracle."""
    setup = None if targets is None else lambda R: R.set_vertex_morph(*(_targets(pkg) if targets == "fixture" else targets))
    return K.pair(pkg, setup, extra=extra, max_depth=6)


def _check_against_oracle(pkg, R, O, weights, bones=None, rest=None, targets=None, film=True):
    """update_morph on R, update_vertices with the restated arrays on O: the device arrays directly, then everything downstream."""
    v, n = _ref(pkg, weights, bones, rest, targets)
    R.update_morph(weights, bones); O.update_vertices(v, n)
    K.assert_arrays(R, v, n)
    a, b = K.state(pkg, R, film), K.state(pkg, O, film)
    K.assert_same(a, b)
    return a


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("gpu_tree", [False, True])
def test_five_targets_with_mixed_weights(pkg, gpu_tree):
    s = K.scene(pkg)
    R, O = _pair(pkg, extra=pkg.FLAG_GPU_BVH_BUILD if gpu_tree else 0)
    K.assert_arrays(R, s.vertex, s.normal)                                   # setting a morph moves nothing
    rest = K.state(pkg, R, film=False)
    before = R.probe_lights()
    moved = _check_against_oracle(pkg, R, O, WEIGHTS)
    assert not np.array_equal(rest["t"], moved["t"])
    assert np.array_equal(before[0], moved["light_face"]) and not np.array_equal(before[2], moved["light_pos"])           # the lamp moved
    v, _ = _ref(pkg, WEIGHTS)
    want = (v[s.face[moved["light_face"], :, 0]] - np.array(list(R.info().centre))).reshape(-1, 9)                        # the nine fp64 positions per light
    assert np.array_equal(bits(want), bits(moved["light_pos"]))
    info = R.update_info(); mi = R.morph_info()
    vt, nt = _targets(pkg)
    assert info.updates == 1 and info.last_update_ms > 0 and (mi.n_targets, mi.updates) == (N_TARGETS, 1) and 0 < mi.last_ms <= info.last_update_ms
    assert mi.vertex_entries == mi.normal_entries == sum(len(i) for i, _ in vt)
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["last_vertex", "no_entries", "vertices_only"])
def test_small_and_partial_target_sets(pkg, case):
    s = K.scene(pkg); nv = s.vertex.shape[0]
    none = (np.zeros(0, np.int64), np.zeros((0, 3)))
    if case == "last_vertex":                                                # one target, one entry on the last record: the tail lane of the last block
        targets = ([(np.array([nv - 1]), np.array([[0.01, -0.02, 0.015]]))], [(np.array([nv - 1]), np.array([[0.3, 0.1, -0.2]]))]); w = [0.75]
    elif case == "no_entries":                                               # targets without a single entry: the kernels still copy the rest pose
        targets = ([none, none], [none, none]); w = [0.5, -2.0]
    else:                                                                    # vertex targets only: the normals are the rest pose's, bit for bit
        targets = (_targets(pkg)[0], None); w = WEIGHTS
    R, O = _pair(pkg, targets=None)
    R.update_vertices(s.vertex * 0.999, None)                                # something else in the current arrays: every record must be written
    R.set_vertex_morph(*targets)
    rest = (s.vertex * 0.999, s.normal)
    v, n = _ref(pkg, w, rest=rest, targets=targets)
    if case != "last_vertex":
        assert np.array_equal(bits(n), bits(s.normal))
    if case == "no_entries":
        assert np.array_equal(bits(v), bits(rest[0]))
    else:
        assert not np.array_equal(v, rest[0])
    R.update_vertices(s.vertex, s.normal + 0.0)                              # overwritten in between: the call reads the morph's rest pose, not this
    _check_against_oracle(pkg, R, O, w, rest=rest, targets=targets)
    mi = R.morph_info()
    assert (mi.n_targets, mi.vertex_entries, mi.normal_entries) == (len(w), sum(len(i) for i, _ in targets[0]), 0 if targets[1] is None else sum(len(i) for i, _ in targets[1]))
    R.close(); O.close()


@pytest.mark.gpu
def test_morphs_are_not_cumulative_and_sequences(pkg):
    s = K.scene(pkg)
    R, O = _pair(pkg, targets=None)
    rest = K.unit_rest(pkg, positive_zero=True)
    R.update_vertices(*rest); O.update_vertices(*rest)                       # unit-length normals without -0.0: see deform_kit.unit_rest
    R.set_vertex_morph(*_targets(pkg))
    original = K.state(pkg, R)
    R.update_morph(WEIGHTS)
    moved = _check_against_oracle(pkg, R, O, WEIGHTS2, rest=rest)            # w1 then w2 = w2 alone
    assert not np.array_equal(moved["film"], original["film"])
    R.update_morph(WEIGHTS2)                                                 # the same weights twice: the same scene
    K.assert_same(K.state(pkg, R), moved)
    back = _check_against_oracle(pkg, R, O, ZERO, rest=rest)                 # w then all-zero: what the restatement says ...
    K.assert_same(original, back)                                            # ... which is the original film, traces, normals and lights, bit for bit
    assert R.morph_info().updates == 4 and R.update_info().updates == 5 and O.update_info().updates == 3
    # update_vertices, update_transforms and update_skin in between: each moves the scene from its OWN rest pose and leaves the morph's alone
    v1, n1 = _ref(pkg, WEIGHTS2, rest=rest)
    R.update_vertices(v1, n1); O.update_vertices(v1, n1)
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    _check_against_oracle(pkg, R, O, WEIGHTS, rest=rest, film=False)         # from the REST pose, not from what update_vertices wrote
    vg, ng = pkg.groups_from_faces(s, np.where(s.face[:, 0, 3] == SPHERE, 1, np.where(s.face[:, 0, 3] == LAMP, 2, 0)))
    gm = np.stack([T.identity(1)[0], clean(T.about(T.rotation((0, 1, 0), 15.0), CENTRE, (0.05, 0.0, 0.05))), M_LAMP])
    R.set_vertex_groups(vg, ng, 3)                                           # the groups' rest pose: the scene as WEIGHTS left it
    posed = _ref(pkg, WEIGHTS, rest=rest)
    R.update_transforms(gm); O.update_vertices(T.transform_vertices(posed[0], vg, gm), T.transform_normals(posed[1], ng, gm))
    K.assert_arrays(R, T.transform_vertices(posed[0], vg, gm), T.transform_normals(posed[1], ng, gm))
    _check_against_oracle(pkg, R, O, WEIGHTS2, rest=rest, film=False)
    vb, vw, nb, nw = K.bend(pkg)
    R.set_vertex_skin(vb, vw, nb, nw, N_BONES)                               # the skin's rest pose: the scene as WEIGHTS2 left it
    posed = _ref(pkg, WEIGHTS2, rest=rest)
    R.update_skin(BEND)
    K.assert_arrays(R, S.skin_vertices(posed[0], vb, vw, BEND), S.skin_normals(posed[1], nb, nw, BEND))
    _check_against_oracle(pkg, R, O, WEIGHTS, rest=rest, film=False)
    R.update_transforms(gm)                                                  # and the reverse: the groups' rest pose is as it was
    posed = _ref(pkg, WEIGHTS, rest=rest)
    K.assert_arrays(R, T.transform_vertices(posed[0], vg, gm), T.transform_normals(posed[1], ng, gm))
    # a second set_vertex_morph takes the current scene as the new rest pose -- and may change the targets
    R.update_vertices(v1, n1)
    two = ([_targets(pkg)[0][1], _targets(pkg)[0][4]], [_targets(pkg)[1][1], _targets(pkg)[1][4]])
    R.set_vertex_morph(*two)
    _check_against_oracle(pkg, R, O, [1.5, -0.25], rest=(v1, n1), targets=two)
    assert R.morph_info().n_targets == 2
    R.close(); O.close()


@pytest.mark.gpu
def test_morph_then_skin(pkg):
    s = K.scene(pkg); vb, vw, nb, nw = K.bend(pkg)
    R, O = _pair(pkg)
    R.set_vertex_skin(vb, vw, nb, nw, N_BONES)
    R.update_skin(BEND)
    skin_alone = R.vertices()
    K.assert_arrays(R, S.skin_vertices(s.vertex, vb, vw, BEND), S.skin_normals(s.normal, nb, nw, BEND))
    base = R.info().device_bytes
    R.update_morph(WEIGHTS2, BEND)
    assert R.info().device_bytes - base == 24 * (s.vertex.shape[0] + s.normal.shape[0])       # the scratch, allocated by the first such call
    both = _check_against_oracle(pkg, R, O, WEIGHTS, BEND)                   # = skin_ref of morph_ref
    base = R.info().device_bytes                                             # (the renders have allocated their pools by now)
    assert not np.array_equal(R.vertices()[0], skin_alone[0]) and not np.array_equal(R.vertices()[0], _ref(pkg, WEIGHTS)[0])
    assert (R.morph_info().updates, R.skin_info().updates, R.update_info().updates) == (2, 3, 3)
    R.update_skin(BEND)                                                      # the skin's own rest pose is untouched: what it gave before
    K.assert_arrays(R, *skin_alone)
    _check_against_oracle(pkg, R, O, WEIGHTS2, K.mats(low=M_HIGH, high=M_LOW), film=False)
    assert R.info().device_bytes == base                                     # and only by the first
    plain = _check_against_oracle(pkg, R, O, WEIGHTS, film=False)            # and without bones again: straight to the current arrays
    assert not np.array_equal(plain["t"], both["t"])
    assert (R.morph_info().updates, R.skin_info().updates) == (4, 5) and 0 < R.morph_info().last_ms <= R.update_info().last_update_ms
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["own", "side"])
def test_update_between_renders_without_a_sync(pkg, which):
    import torch
    R, O = _pair(pkg)
    O.set_vertex_morph(*_targets(pkg))
    for r in (R, O):
        r.set_vertex_skin(*K.bend(pkg), N_BONES)
    if which == "side":
        stream = torch.cuda.Stream()
        R.set_torch_stream(stream)
    R.clear()
    R.render(4, seed=9, first_sample=0); R.update_morph(WEIGHTS); R.render(4, seed=9, first_sample=4)   # nothing in between
    R.update_morph(WEIGHTS2, BEND); R.update_morph(ZERO); R.update_morph(WEIGHTS, BEND)                 # back-to-back calls through the stages keep their order
    R.render(2, seed=9, first_sample=8)
    got = R.read_accum()
    O.clear()
    O.render(4, seed=9, first_sample=0); O.sync(); O.update_morph(WEIGHTS); O.sync(); O.render(4, seed=9, first_sample=4); O.sync()
    O.update_morph(WEIGHTS2, BEND); O.sync(); O.update_morph(ZERO); O.sync(); O.update_morph(WEIGHTS, BEND); O.sync()
    O.render(2, seed=9, first_sample=8); O.sync()
    assert np.array_equal(bits(got), bits(O.read_accum())) and np.all(got[..., 3] == 10)
    K.assert_arrays(R, *_ref(pkg, WEIGHTS, BEND))
    if which == "side":
        R.set_stream(0)
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_bones", [False, True])
@pytest.mark.parametrize("with_camera", [False, True])
def test_reprojection_follows_the_morph(pkg, with_camera, with_bones):
    R, O = _pair(pkg)
    cam = pkg.scenes.Camera((0.62, 0.55, 2.25), (0.5, 0.45, 0.0), (0.0, 1.0, 0.0), 40.0, W, H) if with_camera else None
    bones = None
    if with_bones:
        R.set_vertex_skin(*K.bend(pkg), N_BONES)
        bones = K.mats(low=clean(T.about(T.rotation((0, 0, 1), 3.0), CENTRE)), high=clean(T.about(T.rotation((0, 0, 1), -10.0), CENTRE, (0.02, 0.02, 0.0))))
    w = np.array([-0.05, 0.3, 1.0, 0.4, 0.2])
    v, n = _ref(pkg, w, bones)
    opts = dict(feature_spp=4, feature_seed=3, max_history=16.0)
    for r in (R, O):
        r.clear(); r.render(8, seed=5)
    R.update_morph_reproject(w, bones, camera=cam, **opts)
    O.update_vertices_reproject(v, n, camera=cam, **opts)
    assert np.array_equal(bits(R.read_accum()), bits(O.read_accum()))
    ia, ib = R.reproject_info(), O.reproject_info()
    assert (ia.reprojections, ia.pixels_reused) == (ib.reprojections, ib.pixels_reused) == (1, ib.pixels_reused) and ia.pixels_reused > 0.5 * W * H
    assert np.array_equal(bits(R.features()), bits(O.features()))          # the context holds the new scene's features
    assert R.update_info().updates == 1 and R.morph_info().updates == 1 and R.skin_info().updates == int(with_bones)
    K.assert_arrays(R, v, n)
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    R.close(); O.close()


@pytest.mark.gpu
def test_morph_refusals(pkg):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    vt, nt = _targets(pkg)
    plain = pkg.Renderer(s, max_depth=6, flags=pkg.FLAG_DETERMINISTIC)
    for call in (lambda: plain.set_vertex_morph(vt, nt), lambda: plain.update_morph(WEIGHTS), lambda: plain.update_morph(WEIGHTS, BEND),
                 lambda: plain.update_morph_reproject(WEIGHTS), lambda: plain.vertices()):
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % UNSUPPORTED in str(e.value)
    plain.close()
    R = pkg.Renderer(s, max_depth=6, flags=FLAGS(pkg))
    o, d = K.rays(pkg)
    film = render_film(R, 4, 5); trace = R.probe_trace4(o, d); arrays = R.vertices(); bytes0 = R.info().device_bytes
    expect = {"n_targets": 0, "entries": 0}

    def unchanged():
        mi = R.morph_info()
        assert R.update_info().updates == 0 and R.skin_info().updates == 0
        assert (mi.n_targets, mi.updates, mi.vertex_entries, mi.normal_entries, mi.last_ms) == (expect["n_targets"], 0, expect["entries"], expect["entries"], 0.0)
        assert np.array_equal(bits(render_film(R, 4, 5)), bits(film))
        for x, y in zip(trace, R.probe_trace4(o, d)):
            assert np.array_equal(bits(x), bits(y))
        for x, y in zip(arrays, R.vertices()):
            assert np.array_equal(bits(x), bits(y))

    def refused(call, status=INVALID):
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % status in str(e.value)
        unchanged()
        return str(e.value)

    assert "no morph is set" in refused(lambda: R.update_morph(WEIGHTS))
    refused(lambda: R.update_morph_reproject(WEIGHTS))
    # ---- mcpt_set_vertex_morph
    def with_target(t, k, index=None, delta=None):
        t = list(t); t[k] = (t[k][0] if index is None else np.asarray(index), t[k][1] if delta is None else delta)
        return t

    def edit(a, i, k, x):
        a = a.copy(); a[i, k] = x
        return a

    i4 = vt[4][0]
    none = (np.zeros(0, np.int64), np.zeros((0, 3)))
    bad_sets = [(vt[:-1], nt), (vt, nt[:-1]),                                                               # the two sets' n_targets differ
                ([], None), ([none] * 65537, None),                                                         # n_targets outside [1, 65536]
                (with_target(vt, 4, index=[i4[0], i4[1], i4[3], i4[2]]), nt), (vt, with_target(nt, 4, index=[i4[0], i4[1], i4[3], i4[2]])),   # not ascending
                (with_target(vt, 4, index=[i4[0], i4[1], i4[1], i4[3]]), nt), (vt, with_target(nt, 0, index=np.concatenate([[nt[0][0][0]], nt[0][0][:-1]]))),   # a record twice
                (with_target(vt, 4, index=[i4[0], i4[1], i4[2], nv]), nt), (vt, with_target(nt, 4, index=[i4[0], i4[1], i4[2], nn])),       # index >= the record count
                (with_target(vt, 0, index=np.concatenate([vt[0][0][:-1], [2 ** 32 - 1]])), nt)]
    for x in (np.nan, np.inf, -np.inf, 1.0000001e18):                        # a delta component that is not finite or has |d| > 1e18
        bad_sets.append((with_target(vt, 1, delta=edit(vt[1][1], 3, 1, x)), nt))
    bad_sets.append((vt, with_target(nt, 3, delta=edit(nt[3][1], 0, 2, np.nan))))
    for args in bad_sets:
        assert not (M.accepts_targets(args[0], nv) and (args[1] is None or M.accepts_targets(args[1], nn, len(args[0]))))
        refused(lambda: R.set_vertex_morph(*args))
        assert R.info().device_bytes == bytes0
    lib = R.lib
    tv, keep_v = pkg.targets_struct(vt); tn, keep_n = pkg.targets_struct(nt)

    def raw_set(v=tv, n_vertex=nv, n=tn, n_normal=nn):
        return lib.mcpt_set_vertex_morph(R.ctx, None if v is None else C.byref(v), n_vertex, None if n is None else C.byref(n), n_normal)

    def copy_of(t, **fields):
        c = pkg.MorphTargets(); C.memmove(C.byref(c), C.byref(t), C.sizeof(c))
        for k, x in fields.items():
            setattr(c, k, x)
        return c

    u32p = C.POINTER(C.c_uint32)
    off1 = np.array(keep_v[0]); off1[0] = 1                                 # offsets that do not start at 0
    off2 = np.array(keep_v[0]); off2[2] = off2[1] - 1                       # offsets that decrease
    assert raw_set(n_vertex=nv - 1) == INVALID and raw_set(n_normal=nn + 1) == INVALID                      # counts that differ from the scene's
    assert raw_set(v=None) == INVALID                                                                       # NULL vertex targets
    assert raw_set(v=copy_of(tv, struct_size=C.sizeof(pkg.MorphTargets) - 4)) == INVALID and raw_set(n=copy_of(tn, struct_size=0)) == INVALID
    assert raw_set(v=copy_of(tv, target_offset=None)) == INVALID and raw_set(v=copy_of(tv, index=None)) == INVALID and raw_set(n=copy_of(tn, delta=None)) == INVALID
    assert raw_set(v=copy_of(tv, target_offset=off1.ctypes.data_as(u32p))) == INVALID and raw_set(n=copy_of(tn, target_offset=off2.ctypes.data_as(u32p))) == INVALID
    unchanged()
    assert R.info().device_bytes == bytes0
    R.set_vertex_morph(vt, None)                                             # accepted; then replaced
    R.set_vertex_morph(vt, nt)
    expect["n_targets"] = N_TARGETS; expect["entries"] = sum(len(i) for i, _ in vt)
    unchanged()
    bytes1 = R.info().device_bytes
    for args in bad_sets[:8]:                                                # a refused replacement leaves the morph that is set
        refused(lambda: R.set_vertex_morph(*args))
        assert R.info().device_bytes == bytes1
    # ---- mcpt_update_morph and _reproject: the weights
    used = T.used_vertices(s)
    radius = M.rest_radius(s.vertex, used); dk = M.target_delta(vt, used)
    wp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mcpt_update_morph(R.ctx, None, N_TARGETS, None, 0) == INVALID and lib.mcpt_update_morph_reproject(R.ctx, None, N_TARGETS, None, 0, None, None) == INVALID
    refused(lambda: R.update_morph(WEIGHTS[:-1])); refused(lambda: R.update_morph(np.concatenate([WEIGHTS, [0.0]])))
    for x in (np.nan, np.inf, -np.inf, -1.0000001e18):
        w = WEIGHTS.copy(); w[2] = x                                         # on the EMPTY target: only the weight's own rule refuses it
        assert not M.accepts(w, radius, dk)
        assert "weight" in refused(lambda: R.update_morph(w))
        refused(lambda: R.update_morph_reproject(w))
    far = np.array([-1e18, 1e18, 0.0, 1e18, 1e18])                          # every weight passes its own rule; the reach (about 4.8e17) passes too
    assert M.accepts(far, radius, dk) and not M.accepts(far, radius, 3.0 * dk)           # (the reach refusing is shown with deltas of 1e18, below)
    # ---- with bones: no skin yet, then the skin's own rules with E as every bone's radius
    assert "no skin is set" in refused(lambda: R.update_morph(WEIGHTS, BEND))
    nan_w = WEIGHTS.copy(); nan_w[0] = np.nan
    assert "weight" in refused(lambda: R.update_morph(nan_w, BEND))         # the weights are judged before the bones
    R.set_vertex_skin(*K.bend(pkg), N_BONES)
    bytes2 = R.info().device_bytes
    nan = K.mats(); nan[1, 2, 1] = np.nan
    flat = K.mats(low=T.about(np.diag([1.0, 0.0, 1.0]), CENTRE))              # det A = 0
    far_t = K.mats(); far_t[1, 1, :] = (0.0, 1e3, 0.0, 1e18)
    lonely = K.mats(third=np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1e18, 0.0]]))   # a bone without members: mcpt_update_skin accepts it (R_b = 0)
    for m in (nan, flat, far_t, lonely, BEND[:-1], np.concatenate([BEND, BEND[:1]])):
        assert not M.accepts(WEIGHTS, radius, dk, m, N_BONES)
        refused(lambda: R.update_morph(WEIGHTS, m))
        refused(lambda: R.update_morph_reproject(WEIGHTS, m))
        assert R.info().device_bytes == bytes2                               # no scratch was allocated by a refused call
    both = nan.copy(); both[2] = flat[1]
    assert "not finite" in refused(lambda: R.update_morph(WEIGHTS, both))
    both = flat.copy(); both[3] = lonely[3]
    assert "det A" in refused(lambda: R.update_morph(WEIGHTS, both))
    assert "n_targets" in refused(lambda: R.update_morph(WEIGHTS[:-1], nan))  # the weights' count before anything about the bones
    # ---- _reproject: weights and bones first, then the camera, then the options
    cam = s.camera
    bad_cam = pkg.scenes.Camera(cam.eye, cam.eye, cam.up, cam.fovy, W, H)
    for bones in (None, BEND):
        refused(lambda: R.update_morph_reproject(WEIGHTS, bones, camera=pkg.scenes.Camera(cam.eye, cam.lookat, cam.up, cam.fovy, W + 1, H)))
        refused(lambda: R.update_morph_reproject(WEIGHTS, bones, camera=bad_cam))
        refused(lambda: R.update_morph_reproject(WEIGHTS, bones, feature_spp=65))
        refused(lambda: R.update_morph_reproject(WEIGHTS, bones, max_history=0.5))
        assert "eye == lookat" in refused(lambda: R.update_morph_reproject(WEIGHTS, bones, camera=bad_cam, feature_spp=65))   # a bad camera before bad options
        assert R.info().device_bytes == bytes2
    assert "weight" in refused(lambda: R.update_morph_reproject(nan_w, BEND, camera=bad_cam))                # bad weights before a bad camera
    assert "not finite" in refused(lambda: R.update_morph_reproject(WEIGHTS, nan, camera=bad_cam))          # bad bones before a bad camera
    lib.mcpt_probe_vertices(R.ctx, None, None)                               # both outputs may be NULL
    unchanged()
    R.validate_trees()
    R.update_morph(WEIGHTS, BEND)                                            # and the context still works
    assert R.update_info().updates == 1 and R.morph_info().updates == 1 and R.skin_info().updates == 1
    # ---- the reach: deltas at the limit, refused by the slack factor alone; a weight that brings it back is accepted by the check
    huge = [(np.flatnonzero(used)[5:6], np.array([[1e18, 0.0, 0.0]]))]
    R.set_vertex_morph(huge)
    r5 = M.rest_radius(R.vertices()[0], used); d5 = M.target_delta(huge, used)
    for w in ([1.0], [-1.0], [1e18]):
        assert not M.accepts(w, r5, d5)
        with pytest.raises(pkg.McptError) as e:
            R.update_morph(w)
        assert "status %d" % INVALID in str(e.value) and "conservative" in str(e.value)
    assert M.accepts([0.5], r5, d5) and R.update_info().updates == 1 and R.morph_info().updates == 1
    # ... and the same delta on a vertex no face uses does not count: D_0 = 0, the call is accepted and moves nothing a ray can meet
    idle = [(np.flatnonzero(~used)[:1], np.array([[1e18, 0.0, 0.0]]))]
    R.set_vertex_morph(idle)
    before = R.vertices()[0]
    assert M.target_delta(idle, used)[0] == 0.0 and M.accepts([1.0], r5, [0.0])
    R.update_morph([1.0])
    K.assert_records(R.vertices()[0], M.morph_vertices(before, idle, [1.0]), "vertex")
    R.validate_trees()
    R.close()


@pytest.mark.gpu
def test_clone_rebuild_and_bookkeeping(pkg):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    vt, nt = _targets(pkg); entries = sum(len(i) for i, _ in vt)
    R, O = _pair(pkg, targets=None)
    base = R.info().device_bytes
    mi = R.morph_info()
    assert (mi.n_targets, mi.updates, mi.vertex_entries, mi.normal_entries) == (0, 0, 0, 0)
    fixed = 24 * (nv + nn) + 4 * (nv + 1) + 4 * (nn + 1)                     # rest pose, list offsets
    R.set_vertex_morph(vt, nt)
    assert R.info().device_bytes - base == fixed + 32 * 2 * entries + 8 * N_TARGETS
    R.set_vertex_morph(vt[:2], None)                                         # replaces: the old buffers are released
    assert R.info().device_bytes - base == fixed + 32 * (len(vt[0][0]) + len(vt[1][0])) + 8 * 2 and R.morph_info().n_targets == 2
    R.set_vertex_morph(vt, nt)
    assert R.info().device_bytes - base == fixed + 32 * 2 * entries + 8 * N_TARGETS
    R.update_morph(WEIGHTS)
    clone = R.clone()
    assert clone.info().device_bytes == R.info().device_bytes              # (neither has rendered yet: no pools)
    mi = clone.morph_info()
    assert (mi.n_targets, mi.updates, mi.vertex_entries, mi.normal_entries) == (N_TARGETS, 0, entries, entries)
    K.assert_arrays(clone, *_ref(pkg, WEIGHTS))                              # the clone is the morphed scene ...
    _check_against_oracle(pkg, clone, O, WEIGHTS2)                           # ... with the ORIGINAL rest pose and the targets
    K.assert_arrays(R, *_ref(pkg, WEIGHTS))                                  # the source did not move with its clone
    # a rebuild keeps the targets, the rest pose, R and D_k
    for builder in (pkg.REBUILD_HOST, pkg.REBUILD_DEVICE):
        R.rebuild(builder); O.rebuild(builder)
        assert R.morph_info().n_targets == N_TARGETS
        _check_against_oracle(pkg, R, O, WEIGHTS2 if builder == pkg.REBUILD_HOST else WEIGHTS)
    assert R.info().device_bytes == O.info().device_bytes + fixed + 32 * 2 * entries + 8 * N_TARGETS
    # the scratch of morph-then-skin is counted and carried
    skin_bytes = (24 + 16 + 32) * (nv + nn) + 96 * N_BONES
    R.set_vertex_skin(*K.bend(pkg), N_BONES)
    R.update_morph(WEIGHTS, BEND)
    assert R.info().device_bytes == O.info().device_bytes + fixed + 32 * 2 * entries + 8 * N_TARGETS + skin_bytes + 24 * (nv + nn)
    second = R.clone()
    bare = O.clone()                                                         # (fresh clones hold no render pools; O has the same trees)
    assert second.info().device_bytes == bare.info().device_bytes + fixed + 32 * 2 * entries + 8 * N_TARGETS + skin_bytes + 24 * (nv + nn)
    bare.close()
    K.assert_arrays(second, *_ref(pkg, WEIGHTS, BEND))
    second.update_morph(WEIGHTS2, BEND)
    K.assert_arrays(second, *_ref(pkg, WEIGHTS2, BEND))
    R.update_morph(ZERO); R.update_morph_reproject(ZERO)
    mi = R.morph_info()
    assert (mi.n_targets, mi.updates) == (N_TARGETS, 6) and mi.last_ms > 0 and R.update_info().updates == 6 and R.skin_info().updates == 1
    assert clone.morph_info().updates == 1 and clone.update_info().updates == 1 and second.morph_info().updates == 1
    assert R.update_info().last_update_ms >= mi.last_ms                      # the refit's bracket spans the weights' copy and the morph kernels
    # R and D_k travel with a clone and survive a rebuild: a weight that only a known D_0 = 4e17 can refuse (with D_0 = 0 the reach would be R)
    used = T.used_vertices(s)
    far = [(np.flatnonzero(used)[5:6], np.array([[4e17, 0.0, 0.0]]))]
    R.set_vertex_morph(far)
    third = R.clone()
    R.rebuild(pkg.REBUILD_HOST)
    assert not M.accepts([2.6], M.rest_radius(s.vertex, used), M.target_delta(far, used)) and M.accepts([2.6], M.rest_radius(s.vertex, used), [0.0])
    for r in (R, third):
        with pytest.raises(pkg.McptError) as e:
            r.update_morph([2.6])
        assert "conservative" in str(e.value)
    third.close(); second.close(); clone.close(); R.close(); O.close()


def _swell_and_lift(scene, part):
    """Two targets over the vertices of the faces in `part` (and the normals paired with them): a swell about the part's centroid, and a lift
    that grows with the height inside the part.  (vertex targets, normal targets, vertex indices.)"""
    vi = np.unique(scene.face[part][:, :, 0]); ni = np.unique(scene.face[part][:, :, 1])
    p = scene.vertex[vi]; c = p.mean(0)
    y = (p[:, 1] - p[:, 1].min()) / (p[:, 1].max() - p[:, 1].min())
    lift = np.stack([0.05 * y, 0.1 * y * y, np.zeros_like(y)], 1)
    rng = np.random.default_rng(12)
    vt = [(vi, p - c), (vi[::2], lift[::2])]
    nt = [(ni, rng.uniform(-0.05, 0.05, (len(ni), 3))), (ni[::2], rng.uniform(-0.05, 0.05, (len(ni[::2]), 3)))]
    return vt, nt, vi


@pytest.mark.gpu
def test_facade_morph(pkg, tmp_path):
    exe = kit.build_facade("facade_morph.cpp", tmp_path)
    a = pkg.scenes.cornell_box(44, 30, sphere_lon=24, sphere_lat=12)
    obj = a.write(str(tmp_path / "a"))
    # the program reads the 9-digit text of the file: the same numbers scenes.py keeps (SceneData is rounded through that text form)
    part = a.face[:, 0, 3] == SPHERE
    vt, nt, _ = _swell_and_lift(a, part)
    skin = K.height_skin(pkg, a, part)
    m = np.stack([T.identity(1)[0], M_LOW, M_HIGH]); w = np.array([-0.15, 0.8])
    names = ["voff", "vidx", "vdelta", "noff", "nidx", "ndelta"]
    for arr, name in zip(pkg.flatten_targets(vt) + pkg.flatten_targets(nt), names):
        arr.tofile(str(tmp_path / (name + ".bin")))
    w.tofile(str(tmp_path / "w.bin")); skin[0].astype(np.uint32).tofile(str(tmp_path / "b.bin")); skin[1].tofile(str(tmp_path / "bw.bin")); m.tofile(str(tmp_path / "m.bin"))
    v1, n1 = M.morph_vertices(a.vertex, vt, w), M.morph_normals(a.normal, nt, w)
    v2, n2 = M.morph_then_skin(a.vertex, a.normal, vt, nt, w, skin, m)
    for arr, name in ((v1, "v1"), (n1, "n1"), (v2, "v2"), (n2, "n2")):
        arr.tofile(str(tmp_path / (name + ".bin")))
    ins = [str(tmp_path / (n + ".bin")) for n in names + ["w", "b", "bw", "m", "v1", "n1", "v2", "n2"]]
    outs = [str(tmp_path / n) for n in ("mo.bin", "upd.bin", "ms.bin", "upd2.bin", "rp.bin")]
    k = 4
    line = kit.run_facade(exe, [obj, str(k)] + ins + outs)
    w_, h_ = int(line[0]), int(line[1])
    assert (w_, h_, int(line[2])) == (44, 30, k)
    mo, upd, ms, upd2, rp = [np.fromfile(p, np.float32).reshape(h_, w_, 4) for p in outs]
    assert np.all(mo[..., 3] == k) and mo[..., :3].sum() > 0                 # the picture started again and ends at k samples
    assert np.array_equal(bits(mo), bits(upd))                             # weights on the device = the restated arrays through update()
    assert np.array_equal(bits(ms), bits(upd2)) and not np.array_equal(ms, mo)   # and so for morph, then skin
    assert np.all(rp[..., 3] >= 1) and np.all(rp[..., 3] <= 5) and (rp[..., 3] > 1).mean() > 0.5   # history capped at 4, plus the new frame


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["alone", "bend", "reproject"])
def test_cli_swell(pkg, tmp_path, mode):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    out = str(tmp_path / "img")
    base = [obj, "--turntable", "3", "--spp", "4", "--depth", "5", "--out", out]
    swell = ["--swell", "glossy", "0.2"]
    p = kit.run_cli(base + swell + {"alone": [], "bend": ["--bend", "glossy", "25"], "reproject": ["--reproject", "8"]}[mode])
    assert p.returncode == 0, p.stderr[-2000:]
    imgs = kit.turntable_frames(out)
    assert imgs[0] != imgs[1] and imgs[1] != imgs[2]
    if mode == "alone":                                                      # clean errors
        q = kit.run_cli(base + ["--swell", "no-such-material", "0.2"])
        assert q.returncode == 1 and "no material named" in q.stderr
        for other in (["--wobble", "0.01"], ["--spin", "glossy"]):
            q = kit.run_cli(base + swell + other)
            assert q.returncode == 2 and "--swell" in q.stderr
        q = kit.run_cli([obj] + swell)
        assert q.returncode == 2 and "--turntable" in q.stderr
        for amount in ("nan", "inf"):
            q = kit.run_cli(base + ["--swell", "glossy", amount])
            assert q.returncode == 2 and "finite" in q.stderr
        q = kit.run_cli(base + swell + ["--rebuild-above", "1.0"])
        assert q.returncode == 0, q.stderr[-2000:]
    if mode == "bend":                                                       # both features with the film carried over
        q = kit.run_cli(base + swell + ["--bend", "glossy", "25", "--reproject", "8"])
        assert q.returncode == 0, q.stderr[-2000:]


@pytest.mark.gpu
def test_cli_swell_names_a_material_no_face_uses(pkg, tmp_path):
    """The one clean error of --swell that needs a scene of its own: a material that exists and that no face uses."""
    scene = pkg.scenes.cornell_box_small(40, 32)
    spare = pkg.scenes.SceneData(scene.name, scene.vertex, scene.normal, scene.texcoord, scene.face, list(scene.materials) + [pkg.scenes.Material("spare")], scene.camera, dict(scene.meta))
    obj = spare.write(str(tmp_path / "scene"))
    q = kit.run_cli([obj, "--turntable", "3", "--spp", "2", "--out", str(tmp_path / "img"), "--swell", "spare", "0.2"])
    assert q.returncode == 1 and "no face uses material" in q.stderr


@pytest.mark.gpu
def test_morph_update_is_not_slower_on_the_device_than_the_upload_it_replaces(pkg):
    """S-bath detail 160 (0.59 M triangles), the fixtures' vertices under two targets: device time (mcpt_update_info::last_update_ms, HIP events:
    everything from the first copy to the end of the refit) of mcpt_update_morph against mcpt_update_vertices fed the identical restated arrays,
    in the same process, medians of 20 after 3 warm-ups, alternating.  The one claim: the new call's device time is not larger.  The figures
    are in DESIGN.md §19 and profiles/morph_probe.json (tools/morph_probe.py)."""
    scene = pkg.scenes.bathroom_stress(64, 36, detail=160, tex_size=16)
    part = np.isin(scene.face[:, 0, 3], (5, 6))
    vt, nt, _ = _swell_and_lift(scene, part)
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    R.set_vertex_morph(vt, nt)
    mo, up = [], []
    for i in range(23):
        w = np.array([0.004 * (i + 1), 0.03 * (i + 1)])
        v, n = M.morph_vertices(scene.vertex, vt, w), M.morph_normals(scene.normal, nt, w)
        R.update_morph(w); mo.append(R.update_info().last_update_ms)
        if i == 0:
            K.assert_arrays(R, v, n)
        R.update_vertices(v, n); up.append(R.update_info().last_update_ms)
    R.validate_trees()
    R.close()
    a, b = float(np.median(mo[3:])), float(np.median(up[3:]))
    print("\n[morph] %d vertices + %d normals, %d + %d entries: update_morph %.3f ms, update_vertices %.3f ms on the device (medians of 20), ratio %.3f" % (
        scene.vertex.shape[0], scene.normal.shape[0], sum(len(i) for i, _ in vt), sum(len(i) for i, _ in nt), a, b, a / b))
    assert 0 < a <= b
