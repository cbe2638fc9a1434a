"""Each part of a live scene driven by its own deformer in one update call: mcpt_set_vertex_owners, mcpt_update_parts
(csrc/parts.hip behind the deformers' own kernels, in front of ONE normals pass and ONE refit), mcpt_update_parts_reproject, mcpt_get_parts_info
and their public surfaces.

The reference is tests/parts_ref.py: `combine` picks, per record, the output of its owner's route -- by that route's own restatement
(transform_ref, skin_ref, skin_dq_ref, morph_ref, keyframes_ref) -- when the route ran, and otherwise the bits the record held before.  Nothing
is computed on the way, so everything is compared BIT FOR BIT, without a tolerance: directly, through mcpt_probe_vertices, and downstream
through §16's oracle, a second context of the same scene moved with mcpt_update_vertices to the combined arrays.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from tests import deform_kit as K, keyframes_ref as F, kit, morph_ref as M, normals_ref as NR, parts_ref as P, skin_dq_ref as Q, skin_ref as S, transform_ref as T
from tests.deform_kit import CENTRE, FLAGS, H, INVALID, LAMP, M_HIGH, M_LAMP, M_LOW, N_BONES, SPHERE, UNSUPPORTED, W
from tests.kit import bits, render_film

NEW_SYMBOLS = ["mcpt_set_vertex_owners", "mcpt_update_parts", "mcpt_update_parts_reproject", "mcpt_get_parts_info"]
ALL = P.ROUTES
N_FRAMES = 3
START, FRAME_TIME = 0.0, 0.25                                               # x = time / 0.25 is exact: a test names u itself
T_MID, T_KEY = 0.25 * 1.25, 0.25 * 1.0                                      # u = 0.25 in segment 1; on keyframe 1 (u == 0: device-to-device copies)
BEND = K.mats(low=M_LOW, high=M_HIGH, lamp=M_LAMP)                           # §18's bend: 0 the walls, 1 and 2 the sphere's bones, 3 nobody, 4 the lamp
BEND2 = K.mats(low=M_LOW, high=K.clean(T.about(T.rotation((0, 0, 1), -15.0), (0.5, 0.1, 0.5), (0.0, 0.05, 0.02))), lamp=M_LAMP)
RIGID = K.mats(low=M_LOW, high=K.clean(T.about(T.rotation((0, 0, 1), 25.0), (0.5, 0.1, 0.5), (0.03, 0.08, -0.04))), lamp=M_LAMP)   # rotations and translations only: what §21 takes
GROUPS = np.stack([T.identity(1)[0], K.clean(T.about(T.rotation((0, 1, 0), 30.0), CENTRE, (0.02, 0.05, -0.03))), M_LAMP])        # 0 the walls, 1 the sphere, 2 the lamp
GROUPS2 = np.stack([T.identity(1)[0], K.clean(T.about(T.rotation((0, 1, 0), -50.0), CENTRE, (0.0, 0.08, 0.0))), T.identity(1)[0]])
WEIGHTS, WEIGHTS2 = np.array([0.15, 0.7]), np.array([-0.1, 0.4])


# ------------------------------------------------------------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def _groups(pkg, small):
    """(vertex groups, normal groups): the walls 0, the sphere 1, the lamp 2."""
    s = K.scene(pkg, small); mtl = s.face[:, 0, 3]
    return pkg.groups_from_faces(s, np.where(mtl == SPHERE, 1, np.where(mtl == LAMP, 2, 0)))


@functools.lru_cache(maxsize=None)
def _targets(pkg, small):
    """A small morph set, the same index sets for the vertices and for the normals: 0 dense over the sphere (a swell about its centre), 1 every
    third record of the scene (walls and lamp included).  The normal targets carry random deltas of their own."""
    s = K.scene(pkg, small); sphere, _ = K.parts(pkg, small)
    rng = np.random.default_rng(41)
    si = np.flatnonzero(sphere); every = np.arange(0, s.vertex.shape[0], 3)
    sets = [si, every]
    vd = [s.vertex[si] - CENTRE, rng.uniform(-0.01, 0.01, (len(every), 3))]
    nd = [rng.uniform(-0.3, 0.3, (len(i), 3)) for i in sets]
    return list(zip(sets, vd)), list(zip(sets, nd))


@functools.lru_cache(maxsize=None)
def _frames(pkg, small):
    """Three frames with normal frames: every vertex displaced by a different small smooth offset per frame (the room stays a room), every
    normal tilted and normalised.  Normal record 7 of frame 1 carries negative zeros.  ((3, nv, 3), (3, nn, 3).)"""
    s = K.scene(pkg, small); p, q = s.vertex, s.normal
    vf = np.repeat(p[None], N_FRAMES, 0); nf = np.repeat(q[None], N_FRAMES, 0)
    for k in range(N_FRAMES):
        vf[k] = p + 0.004 * (k + 1) * np.stack([np.sin(9.0 * p[:, 1] + k), np.sin(7.0 * p[:, 2] + 2 * k), np.sin(8.0 * p[:, 0] - k)], 1)
        n = q + 0.2 * np.stack([np.sin(5.0 * q[:, 1] + k), np.cos(6.0 * q[:, 0] - k), np.sin(4.0 * q[:, 2] + 3 * k)], 1)
        nf[k] = n / np.linalg.norm(n, axis=1, keepdims=True)
    nf[1][7] = (-0.0, 1.0, -0.0)
    return vf, nf


def _setup(pkg, R, small, mode=F.LINEAR, wrap=F.CLAMP):
    """All four deformers on one context: groups, the five-bone bend skin, the morph set, the keyframes."""
    vg, ng = _groups(pkg, small)
    R.set_vertex_groups(vg, ng, 3)
    R.set_vertex_skin(*K.bend(pkg, small), N_BONES)
    R.set_vertex_morph(*_targets(pkg, small))
    R.set_vertex_keyframes(*_frames(pkg, small), START, FRAME_TIME, mode, wrap)


def _pair(pkg, small, extra=0, **kw):
    return K.pair(pkg, lambda R: _setup(pkg, R, small, **kw), extra=extra, max_depth=6, scene=K.scene(pkg, small))


def _interleaved(n):
    """Vertex owner i % 5, normal owner (7 i + 3) % 5: every route owns records in every block and in the tail."""
    i = np.arange(n)
    return (i % 5).astype(np.uint8), ((7 * i + 3) % 5).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _split(pkg, small):
    """A realistic split, from one owner per face: the sphere MORPH, the lamp GROUPS, everything else KEYFRAMES."""
    s = K.scene(pkg, small); mtl = s.face[:, 0, 3]
    return pkg.owners_from_faces(s, np.where(mtl == SPHERE, P.MORPH, np.where(mtl == LAMP, P.GROUPS, P.KEYFRAMES)))


def _payload(routes, then_skin=False, groups=GROUPS, bones=BEND, weights=WEIGHTS, time=T_MID):
    """Renderer.update_parts' arguments for exactly `routes`."""
    return dict(groups=groups if routes & P.route(P.GROUPS) else None, bones=bones if routes & P.route(P.SKIN) or then_skin else None,
                weights=weights if routes & P.route(P.MORPH) else None, time=time if routes & P.route(P.KEYFRAMES) else None,
                morph_then_skin=then_skin, routes=routes)


def _outputs(pkg, small, routes, then_skin=False, groups=GROUPS, bones=BEND, weights=WEIGHTS, time=T_MID, dq=False, mode=F.LINEAR, wrap=F.CLAMP):
    """Per route that runs what ITS OWN call writes, by its own restatement: ({owner: vertices}, {owner: normals}).  Every rest pose is the
    scene's: the deformers were set up on the untouched scene."""
    s = K.scene(pkg, small); skin = Q if dq else S
    vb, vw, nb, nw = K.bend(pkg, small)
    v, n = {}, {}
    if routes & P.route(P.GROUPS):
        vg, ng = _groups(pkg, small)
        v[P.GROUPS] = T.transform_vertices(s.vertex, vg, groups); n[P.GROUPS] = T.transform_normals(s.normal, ng, groups)
    if routes & P.route(P.SKIN):
        v[P.SKIN] = skin.skin_vertices(s.vertex, vb, vw, bones); n[P.SKIN] = skin.skin_normals(s.normal, nb, nw, bones)
    if routes & P.route(P.MORPH):
        vt, nt = _targets(pkg, small)
        mv, mn = M.morph_vertices(s.vertex, vt, weights), M.morph_normals(s.normal, nt, weights)
        v[P.MORPH], n[P.MORPH] = (skin.skin_vertices(mv, vb, vw, bones), skin.skin_normals(mn, nb, nw, bones)) if then_skin else (mv, mn)
    if routes & P.route(P.KEYFRAMES):
        vf, nf = _frames(pkg, small)
        v[P.KEYFRAMES] = F.play_vertices(vf, time, START, FRAME_TIME, mode, wrap); n[P.KEYFRAMES] = F.play_normals(nf, time, START, FRAME_TIME, mode, wrap)
    return v, n


def _want(pkg, small, before, owners, routes, **kw):
    """The combined arrays after a parts update of `routes` on a context that held `before` = (vertices, normals)."""
    v, n = _outputs(pkg, small, routes, **kw)
    return P.combine(before[0], owners[0], v), P.combine(before[1], owners[1], n)


def _pose(pkg, small):
    """A distinctive pose that no route writes: every record moved and every normal turned."""
    s = K.scene(pkg, small)
    n = s.normal[:, [1, 2, 0]] * np.array([1.0, -1.0, 1.0])
    return s.vertex * 0.97 + np.array([0.011, 0.017, 0.013]), n


def _counts(R):
    return (R.update_info().updates, R.transform_info().updates, R.skin_info().updates, R.morph_info().updates, R.keyframe_info().updates, R.parts_info().updates)


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_parts_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, ("set_vertex_owners", "clear_vertex_owners", "update_parts", "update_parts_reproject", "parts_info"))
    assert set(pkg.PartsInfo().as_dict()) == {"struct_size", "set", "updates", "last_routes", "vertex_records", "normal_records", "last_ms", "device_bytes"}
    assert (pkg.OWNER_NONE, pkg.OWNER_GROUPS, pkg.OWNER_SKIN, pkg.OWNER_MORPH, pkg.OWNER_KEYFRAMES) == (P.NONE, P.GROUPS, P.SKIN, P.MORPH, P.KEYFRAMES) == (0, 1, 2, 3, 4)
    assert (pkg.ROUTE_GROUPS, pkg.ROUTE_SKIN, pkg.ROUTE_MORPH, pkg.ROUTE_KEYFRAMES, pkg.PARTS_MORPH_THEN_SKIN) == (2, 4, 8, 16, 1) and P.ROUTES == 30


def test_null_context_is_an_invalid_argument_for_the_parts_calls(pkg):
    lib = pkg.load_library()
    u = pkg.SceneUpdate(); u.struct_size = C.sizeof(pkg.SceneUpdate); u.routes = pkg.ROUTE_KEYFRAMES
    owner = np.zeros(4, np.uint8); op = owner.ctypes.data_as(C.c_void_p); info = pkg.PartsInfo()
    assert lib.mcpt_set_vertex_owners(None, op, 4, op, 4) == INVALID and lib.mcpt_set_vertex_owners(None, None, 0, None, 0) == INVALID
    assert lib.mcpt_update_parts(None, C.byref(u)) == INVALID and lib.mcpt_update_parts(None, None) == INVALID
    assert lib.mcpt_update_parts_reproject(None, C.byref(u), None, None) == INVALID
    assert lib.mcpt_get_parts_info(None, C.byref(info)) == INVALID


def test_parts_structs_have_the_headers_layout(pkg, tmp_path):
    """sizeof and every offsetof of mcpt_scene_update and mcpt_parts_info as a C compiler sees include/mcpt.h, against the ctypes classes, and
    the header's macros against the package's constants."""
    macros = ("MCPT_OWNER_NONE", "MCPT_OWNER_GROUPS", "MCPT_OWNER_SKIN", "MCPT_OWNER_MORPH", "MCPT_OWNER_KEYFRAMES", "MCPT_ROUTE_GROUPS", "MCPT_ROUTE_SKIN",
              "MCPT_ROUTE_MORPH", "MCPT_ROUTE_KEYFRAMES", "MCPT_PARTS_MORPH_THEN_SKIN")
    for cls, name, size in ((pkg.SceneUpdate, "mcpt_scene_update", 88), (pkg.PartsInfo, "mcpt_parts_info", 88)):
        c, py, values = K.c_layout(cls, name, tmp_path, macros)
        assert c == py and c[0] == size
        assert values == [pkg.OWNER_NONE, pkg.OWNER_GROUPS, pkg.OWNER_SKIN, pkg.OWNER_MORPH, pkg.OWNER_KEYFRAMES, pkg.ROUTE_GROUPS, pkg.ROUTE_SKIN, pkg.ROUTE_MORPH,
                          pkg.ROUTE_KEYFRAMES, pkg.PARTS_MORPH_THEN_SKIN] == [0, 1, 2, 3, 4, 2, 4, 8, 16, 1]


def test_owners_from_faces(pkg):
    for small in (True, False):
        s = K.scene(pkg, small); mtl = s.face[:, 0, 3]
        vo, no = _split(pkg, small)
        assert vo.dtype == no.dtype == np.uint8 and vo.shape == (s.vertex.shape[0],) and no.shape == (s.normal.shape[0],)
        sphere, lamp = K.parts(pkg, small); used = T.used_vertices(s)
        assert (vo[sphere] == P.MORPH).all() and (vo[lamp] == P.GROUPS).all() and (vo[used & ~sphere & ~lamp] == P.KEYFRAMES).all()
        assert (vo[~used] == P.NONE).all() and (~used).sum() == 2                # a record no face uses is NONE
        for col, o in ((0, vo), (1, no)):                                                            # every corner's record has its face's owner
            assert np.array_equal(o[s.face[:, :, col]], np.repeat(np.where(mtl == SPHERE, P.MORPH, np.where(mtl == LAMP, P.GROUPS, P.KEYFRAMES))[:, None], 3, 1))
        none = pkg.owners_from_faces(s, np.zeros(len(mtl), int))
        assert not none[0].any() and not none[1].any()
    s = K.scene(pkg, True)
    fo = np.full(s.face.shape[0], P.SKIN); fo[0] = P.GROUPS                  # face 0 shares its vertices with a neighbour of another owner
    shared = [int(i) for i in s.face[0, :, 0] if (s.face[1:, :, 0] == i).any()]
    assert shared
    with pytest.raises(ValueError, match=r"vertex (%s) is used by faces of owners 1 and 2" % "|".join(map(str, shared))):
        pkg.owners_from_faces(s, fo)
    for bad in (np.full(s.face.shape[0], 5), np.full(s.face.shape[0], -1), np.zeros(s.face.shape[0] - 1, int)):
        with pytest.raises(ValueError, match="one owner id"):
            pkg.owners_from_faces(s, bad)


def test_combine_on_hand_made_arrays():
    before = np.arange(18, dtype=np.float64).reshape(6, 3)
    before[5] = (-0.0, np.nan, np.inf)
    owners = np.array([P.NONE, P.GROUPS, P.SKIN, P.MORPH, P.KEYFRAMES, P.NONE], np.uint8)
    g, k = before + 100.0, before + 400.0
    k[4] = np.frombuffer(np.array([0x7ff8000000000123, 0x8000000000000000, 0xfff0000000000000], np.uint64).tobytes(), np.float64)   # a NaN payload, -0.0, -inf
    out = P.combine(before, owners, {P.GROUPS: g, P.KEYFRAMES: k})
    assert np.array_equal(bits(out[[0, 2, 3, 5]]), bits(before[[0, 2, 3, 5]]))                     # NONE, and owners whose route did not run
    assert np.array_equal(bits(out[1]), bits(g[1])) and np.array_equal(bits(out[4]), bits(k[4])) and bits(out[4])[0] == 0x7ff8000000000123
    assert np.array_equal(bits(P.combine(before, owners, {})), bits(before)) and P.combine(before, owners, {}) is not before
    every = P.combine(before, np.full(6, P.MORPH, np.uint8), {P.MORPH: g, P.SKIN: k})
    assert np.array_equal(bits(every), bits(g))
    with pytest.raises(AssertionError):
        P.combine(before, owners, {P.NONE: g})
    with pytest.raises(AssertionError):
        P.combine(before, owners[:-1], {P.GROUPS: g})


def _owner_cases():
    """(vertex owners, normal owners or None, n_vertex, n_normal, scene_vertex, scene_normal): every refusal, alone and two at once, and sets
    that pass."""
    rng = np.random.default_rng(7)
    cases = []
    for nv, nn in ((1, 1), (5, 3), (349, 349), (1249, 1249), (257, 0), (7, 1000)):
        vo, no = rng.integers(0, 5, nv).astype(np.uint8), rng.integers(0, 5, nn).astype(np.uint8)
        cases.append((vo, no, nv, nn, nv, nn))
        cases.append((vo, no, nv, nn, nv + 1, nn)); cases.append((vo, no, nv, nn, nv, nn + 1)); cases.append((vo, no, nv, nn, max(nv - 1, 0), nn))   # counts
        cases.append((vo, None, nv, nn, nv, nn))                                                                   # NULL normal_owner: refused iff n_normal > 0
        cases.append((vo, None, nv, nn, nv + 2, nn))                                                               # ... behind wrong counts
        for bad in (5, 6, 255):
            for at in sorted({0, nv // 2, nv - 1}):
                b = vo.copy(); b[at] = bad
                cases.append((b, no, nv, nn, nv, nn)); cases.append((b, None, nv, nn, nv, nn)); cases.append((b, no, nv, nn, nv, nn + 3))
            for at in sorted({0, nn // 2, nn - 1}) if nn else ():
                b = no.copy(); b[at] = bad
                cases.append((vo, b, nv, nn, nv, nn))
                v2 = vo.copy(); v2[nv - 1] = 9                                                                     # a bad vertex and a bad normal: the vertex is named
                cases.append((v2, b, nv, nn, nv, nn))
    cases.append((np.zeros(0, np.uint8), np.zeros(0, np.uint8), 0, 0, 0, 0))
    return cases


@K.needs_hipcc
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_owner_checks_counts_and_plans_are_the_restatement(tmp_path, sanitized):
    """The host half of the feature -- pt_check_owners and pt_plan of csrc/parts.hip -- built into the stand-alone program
    tests/parts_host_check.cpp (no device is touched) against tests/parts_ref.py: every refusal of the owner validation with the record it
    names, the per-owner counts, and the route plan for all 16 `routes` masks x the flag and for unknown bits.  `sanitized`: the same program
    under the host's address and undefined-behaviour sanitizers, which must stay silent."""
    exe = K.build_host_check("parts_host_check", ["parts.hip"], tmp_path, sanitized)
    owners = _owner_cases()
    plans = [(m << 1, f) for m in range(16) for f in (0, 1)] + [(1, 0), (1, 1), (32, 0), (30 | 32, 1), (1 << 31, 0), (30, 2), (30, 3), (8, 0x80000001), (0, 2), (1, 2), (4, 3)]
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(np.array([len(owners), len(plans)], np.uint32).tobytes())
        for vo, no, nv, nn, sv, sn in owners:
            f.write(np.array([nv, nn, sv, sn, vo.size, 0xffffffff if no is None else no.size], np.uint32).tobytes())
            f.write(vo.tobytes()); f.write(b"" if no is None else no.tobytes())
        f.write(np.array(plans, np.uint32).tobytes())
    K.run_host_check(exe, tmp_path, sanitized)
    raw = open(str(tmp_path / "out.bin"), "rb").read()
    assert len(raw) == 140 * len(owners) + 32 * len(plans)
    refused = set()
    for i, (vo, no, nv, nn, sv, sn) in enumerate(owners):
        ints = np.frombuffer(raw, np.uint32, 11, 140 * i).tolist(); msg = raw[140 * i + 44:140 * (i + 1)].split(b"\0")[0].decode()
        want = P.check_owners(vo, no, sv, sn, nv, nn)
        if want[0]:
            assert ints == [1] + want[1] + want[2] and msg == "" and sum(want[1]) == nv and sum(want[2]) == nn, (i, ints, msg)
        else:
            assert ints == [0] * 11 and msg == want[1], (i, ints, msg, want)
            refused.add(msg.split(":")[0].rstrip("0123456789 "))
    assert refused == {"n_vertex / n_normal differ from the scene's", "null normal_owner", "vertex", "normal"}
    seen = set()
    for j, (routes, flags) in enumerate(plans):
        got = np.frombuffer(raw, np.uint32, 8, 140 * len(owners) + 32 * j).tolist()
        status, steps, then_skin, bones = P.plan(routes, flags)
        assert got == [status, len(steps)] + steps + [0] * (4 - len(steps)) + [int(then_skin), int(bones)], (routes, flags, got)
        assert steps == sorted(steps) and (status == P.PLAN_OK) == (len(steps) > 0)
        seen.add(status)
    assert seen == {P.PLAN_OK, P.PLAN_NO_ROUTE, P.PLAN_UNKNOWN_ROUTE, P.PLAN_UNKNOWN_FLAG, P.PLAN_SKIN_WITHOUT_MORPH}
    assert P.plan(30, 1) == (P.PLAN_OK, [1, 2, 3, 4], True, True) and P.plan(8, 0) == (P.PLAN_OK, [3], False, False) and P.plan(8, 1)[2:] == (True, True)
    assert P.plan(0, 2)[0] == P.PLAN_NO_ROUTE and P.plan(1, 2)[0] == P.PLAN_UNKNOWN_ROUTE and P.plan(4, 3)[0] == P.PLAN_UNKNOWN_FLAG and P.plan(4, 1)[0] == P.PLAN_SKIN_WITHOUT_MORPH


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("then_skin", [False, True])
@pytest.mark.parametrize("small", [True, False])
def test_interleaved_owners_all_four_routes(pkg, small, then_skin):
    """Vertex owner i % 5, normal owner (7 i + 3) % 5, all four routes in one call, at 349 and at 1 249 records: between keyframes, on a
    keyframe (u == 0: the copies go through the scratch pair too), with Catmull-Rom, and in dual-quaternion mode with rigid bones."""
    s = K.scene(pkg, small)
    R, O = _pair(pkg, small)
    owners = _interleaved(s.vertex.shape[0])
    R.set_vertex_owners(*owners)
    K.assert_arrays(R, s.vertex, s.normal)                                   # setting owners moves nothing
    R.update_vertices(*_pose(pkg, small))                                    # what the NONE records keep
    for kw in (dict(), dict(time=T_KEY), dict(mode=F.CATMULL_ROM, wrap=F.LOOP, time=0.25 * 2.5), dict(dq=True, bones=RIGID)):
        if "mode" in kw:
            R.set_vertex_keyframes(*_frames(pkg, small), START, FRAME_TIME, kw["mode"], kw["wrap"])
        if kw.get("dq"):
            R.set_skin_mode(pkg.SKIN_DUAL_QUATERNION)
            kw = dict(kw, mode=F.CATMULL_ROM, wrap=F.LOOP)                   # (the keyframes set above stay)
        before = R.vertices()
        call = {k: kw[k] for k in ("time", "bones") if k in kw}
        R.update_parts(**_payload(ALL, then_skin, **call))
        v, n = _want(pkg, small, before, owners, ALL, then_skin=then_skin, **kw)
        K.assert_arrays(R, v, n)
        for o, a, b in ((owners[0], v, before[0]), (owners[1], n, before[1])):
            assert np.array_equal(bits(a[o == P.NONE]), bits(b[o == P.NONE])) and not np.array_equal(a[o != P.NONE], b[o != P.NONE])
    assert _counts(R) == (5, 4, 4 + 4 * then_skin, 4, 4, 4) and R.parts_info().last_routes == ALL
    R.close(); O.close()


@pytest.mark.gpu
def test_negative_zeros_of_a_keyframe_survive_the_select(pkg):
    small = True
    s = K.scene(pkg, small); _, nf = _frames(pkg, small)
    R, O = _pair(pkg, small)
    no = np.zeros(s.normal.shape[0], np.uint8); no[7] = P.KEYFRAMES
    R.set_vertex_owners(np.zeros(s.vertex.shape[0], np.uint8), no)
    R.update_parts(time=T_KEY)
    got = R.vertices()[1]
    assert np.array_equal(bits(got[7]), bits(nf[1][7])) and np.signbit(got[7]).tolist() == [True, False, True]
    K.assert_arrays(R, s.vertex, np.concatenate([s.normal[:7], nf[1][7:8], s.normal[8:]]))
    R.close(); O.close()


@pytest.mark.gpu
def test_subsets_of_routes_leave_the_other_owners_records_alone(pkg):
    small = True
    s = K.scene(pkg, small)
    R, O = _pair(pkg, small)
    owners = _interleaved(s.vertex.shape[0])
    R.set_vertex_owners(*owners)
    pose = _pose(pkg, small)
    masks = [P.route(P.SKIN) | P.route(P.KEYFRAMES)] + [P.route(o) for o in (P.GROUPS, P.SKIN, P.MORPH, P.KEYFRAMES)] + [P.route(P.MORPH)]
    for j, routes in enumerate(masks):
        then_skin = j == len(masks) - 1                                      # the last: the morph route alone, morph then skin
        R.update_vertices(*pose)
        R.update_parts(**_payload(routes, then_skin))
        v, n = _want(pkg, small, pose, owners, routes, then_skin=then_skin)
        K.assert_arrays(R, v, n)
        for o, a, b in ((owners[0], v, pose[0]), (owners[1], n, pose[1])):
            ran = np.isin(o, [k for k in range(1, 5) if routes & P.route(k)])
            assert np.array_equal(bits(a[~ran]), bits(b[~ran])) and ran.any() and not np.array_equal(a[ran], b[ran])
        assert R.parts_info().last_routes == routes
    R.close(); O.close()


@pytest.mark.gpu
def test_edges_a_route_that_owns_nothing_one_record_or_the_last(pkg):
    small = False
    s = K.scene(pkg, small); nv = s.vertex.shape[0]
    R, O = _pair(pkg, small)
    pose = _pose(pkg, small)
    # a route that runs and owns nothing: the skin, beside the keyframes that own everything
    owners = (np.full(nv, P.KEYFRAMES, np.uint8), np.full(nv, P.KEYFRAMES, np.uint8))
    R.set_vertex_owners(*owners); R.update_vertices(*pose)
    routes = P.route(P.SKIN) | P.route(P.KEYFRAMES)
    R.update_parts(**_payload(routes))
    K.assert_arrays(R, *_want(pkg, small, pose, owners, routes))
    assert R.skin_info().updates == 1 and R.keyframe_info().updates == 1
    # one route owns only record 0, another only the last record
    vo = np.zeros(nv, np.uint8); no = np.zeros(nv, np.uint8)
    vo[0] = P.GROUPS; vo[-1] = P.MORPH; no[0] = P.MORPH; no[-1] = P.GROUPS
    R.set_vertex_owners(vo, no); R.update_vertices(*pose)
    routes = P.route(P.GROUPS) | P.route(P.MORPH)
    R.update_parts(**_payload(routes))
    v, n = _want(pkg, small, pose, (vo, no), routes)
    K.assert_arrays(R, v, n)
    assert np.array_equal(bits(v[1:-1]), bits(pose[0][1:-1])) and not np.array_equal(v[0], pose[0][0]) and not np.array_equal(v[-1], pose[0][-1])
    # owners all NONE with one route run: nothing moves, and the update is still counted
    R.set_vertex_owners(np.zeros(nv, np.uint8), np.zeros(nv, np.uint8)); R.update_vertices(*pose)
    before = _counts(R)
    R.update_parts(**_payload(P.route(P.GROUPS)))
    K.assert_arrays(R, *pose)
    assert _counts(R) == (before[0] + 1, before[1] + 1, before[2], before[3], before[4], before[5] + 1)
    O.update_vertices(*pose)
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["groups", "skin", "morph", "morph_then_skin", "keyframes"])
def test_one_route_owning_everything_is_that_routes_own_call(pkg, route):
    small = True
    nv = K.scene(pkg, small).vertex.shape[0]
    R, R2 = _pair(pkg, small)
    _setup(pkg, R2, small)
    owner = {"groups": P.GROUPS, "skin": P.SKIN, "morph": P.MORPH, "morph_then_skin": P.MORPH, "keyframes": P.KEYFRAMES}[route]
    R.set_vertex_owners(np.full(nv, owner, np.uint8), np.full(nv, owner, np.uint8))
    R.update_parts(**_payload(P.route(owner), route == "morph_then_skin"))
    {"groups": lambda: R2.update_transforms(GROUPS), "skin": lambda: R2.update_skin(BEND), "morph": lambda: R2.update_morph(WEIGHTS),
     "morph_then_skin": lambda: R2.update_morph(WEIGHTS, BEND), "keyframes": lambda: R2.update_keyframes(T_MID)}[route]()
    K.assert_same(K.state(pkg, R, arrays=True), K.state(pkg, R2, arrays=True))
    assert R.update_info().updates == R2.update_info().updates == 1
    R.close(); R2.close()


@pytest.mark.gpu
def test_a_realistic_split_against_the_oracle(pkg):
    """The sphere morphed then skinned, the lamp a rigid group, everything else keyframed, in one call; the oracle context gets the combined
    arrays through update_vertices.  Every probe ray's hit, the shading records, the light records and the deterministic film, bit for bit;
    then again with the automatic normals on both contexts: one pass over the combined arrays."""
    small = False
    s = K.scene(pkg, small)
    R, O = _pair(pkg, small)
    owners = _split(pkg, small)
    R.set_vertex_owners(*owners)
    routes = P.route(P.GROUPS) | P.route(P.MORPH) | P.route(P.KEYFRAMES)
    v, n = _want(pkg, small, (s.vertex, s.normal), owners, routes, then_skin=True)
    R.update_parts(**_payload(routes, True)); O.update_vertices(v, n)
    K.assert_arrays(R, v, n)
    K.assert_same(K.state(pkg, R), K.state(pkg, O))
    assert not np.array_equal(v, s.vertex) and R.skin_info().updates == 1 and R.update_info().updates == 1
    for r in (R, O):
        r.set_auto_normals()
    before = R.normals_info().updates
    kw = dict(groups=GROUPS2, bones=BEND2, weights=WEIGHTS2, time=0.25 * 0.5)
    v2, n2 = _want(pkg, small, (v, n), owners, routes, then_skin=True, **kw)
    R.update_parts(**_payload(routes, True, **kw)); O.update_vertices(v2, n2)
    a, b = K.state(pkg, R, arrays=True), K.state(pkg, O, arrays=True)
    K.assert_same(a, b)
    auto = NR.auto_normals(s.face, v2, n2, None, v, n)
    assert np.array_equal(bits(a["vertex"]), bits(v2)) and np.array_equal(bits(a["normal"]), bits(auto)) and not np.array_equal(auto, n2)
    assert R.normals_info().updates == before + 1 and R.update_info().updates == 2
    R.close(); O.close()


@pytest.mark.gpu
def test_the_existing_calls_ignore_the_owners(pkg):
    small = True
    s = K.scene(pkg, small)
    R, O = _pair(pkg, small)
    R.set_vertex_owners(*_interleaved(s.vertex.shape[0]))
    vg, ng = _groups(pkg, small); vb, vw, nb, nw = K.bend(pkg, small); vf, nf = _frames(pkg, small)
    R.update_transforms(GROUPS)
    K.assert_arrays(R, T.transform_vertices(s.vertex, vg, GROUPS), T.transform_normals(s.normal, ng, GROUPS))   # every record
    R.update_skin(BEND)
    K.assert_arrays(R, S.skin_vertices(s.vertex, vb, vw, BEND), S.skin_normals(s.normal, nb, nw, BEND))
    R.update_morph(WEIGHTS, BEND)
    K.assert_arrays(R, *M.morph_then_skin(s.vertex, s.normal, *_targets(pkg, small), WEIGHTS, K.bend(pkg, small), BEND))
    R.update_keyframes(T_MID)
    K.assert_arrays(R, F.play_vertices(vf, T_MID, START, FRAME_TIME), F.play_normals(nf, T_MID, START, FRAME_TIME))
    R.update_vertices(*_pose(pkg, small))
    K.assert_arrays(R, *_pose(pkg, small))
    assert R.parts_info().updates == 0
    R.close(); O.close()


@pytest.mark.gpu
def test_refusals_in_their_order_change_nothing(pkg):
    """One refusal per rule, in the documented order; every call carries the NEXT rule's fault too and must report the earlier one."""
    small = True
    s = K.scene(pkg, small); nv = s.vertex.shape[0]
    lib = pkg.load_library()
    plain = pkg.Renderer(s, max_depth=6, flags=pkg.FLAG_DETERMINISTIC)       # no FLAG_DYNAMIC
    bare = pkg.Renderer(s, max_depth=6, flags=FLAGS(pkg))                    # dynamic, owners set, no route set up
    R, O = _pair(pkg, small)
    owners = _interleaved(nv)
    size = C.sizeof(pkg.SceneUpdate)
    nan = float("nan")

    def update(r, routes, flags=0, struct_size=size, null=(), n=None, **kw):
        """The status and message of mcpt_update_parts on a hand-made record; `null`: payloads left NULL; n: counts overridden."""
        u, keep = r._scene_update(kw.get("groups", GROUPS), kw.get("bones", BEND), kw.get("weights", WEIGHTS), kw.get("time", T_MID), False, routes)
        u.flags = flags; u.struct_size = struct_size
        for name in null:
            setattr(u, name, None)
        for name, value in (n or {}).items():
            setattr(u, name, value)
        st = lib.mcpt_update_parts(r.ctx, C.byref(u))
        return st, (lib.mcpt_last_error() or b"").decode()

    def snapshot(r):
        return r.vertices(), r.info().wide_tree_hash, _counts(r)

    def same(a, b):
        return np.array_equal(bits(a[0][0]), bits(b[0][0])) and np.array_equal(bits(a[0][1]), bits(b[0][1])) and a[1:] == b[1:]

    # 1. without MCPT_FLAG_DYNAMIC, before the NULL update is looked at
    assert lib.mcpt_update_parts(plain.ctx, None) == UNSUPPORTED and "MCPT_FLAG_DYNAMIC" in lib.mcpt_last_error().decode()
    assert lib.mcpt_set_vertex_owners(plain.ctx, None, 0, None, 0) == UNSUPPORTED
    # 2. a NULL update; 3. a wrong struct_size, on a context without owners; 4. no owners, with routes == 0
    before = snapshot(bare)
    assert lib.mcpt_update_parts(bare.ctx, None) == INVALID and "null update" in lib.mcpt_last_error().decode()
    assert update(bare, ALL, struct_size=size - 8) == (INVALID, "mcpt_update_parts: update->struct_size != sizeof(mcpt_scene_update)")
    st, msg = update(bare, 0)
    assert st == INVALID and "no owners are set" in msg
    bare.set_vertex_owners(*owners)
    # 5. routes == 0 (with the flag, which then has no morph route); an unknown route bit (with an unknown flag bit); an unknown flag bit (with
    # the flag without its route)
    for (routes, flags), word in (((0, 1), "names no route"), ((1, 2), "routes has an unknown bit"), ((ALL | 32, 2), "routes has an unknown bit"),
                                  ((P.route(P.GROUPS), 3), "flags has an unknown bit")):
        st, msg = update(bare, routes, flags)
        assert st == INVALID and word in msg, (routes, flags, msg)
    # 6. MCPT_PARTS_MORPH_THEN_SKIN without MCPT_ROUTE_MORPH, on a context where no route is set up
    st, msg = update(bare, P.route(P.GROUPS) | P.route(P.KEYFRAMES), 1)
    assert st == INVALID and "MCPT_PARTS_MORPH_THEN_SKIN without MCPT_ROUTE_MORPH" in msg
    # 7. per route in id order: never set up
    for routes, word in ((ALL, "no groups are set"), (ALL & ~2, "no skin is set"), (P.route(P.MORPH) | P.route(P.KEYFRAMES), "no morph is set"), (P.route(P.KEYFRAMES), "no keyframes are set")):
        st, msg = update(bare, routes)
        assert st == INVALID and word in msg, msg
    assert same(snapshot(bare), before) and bare.parts_info().updates == 0
    # ... and on the context with all four: each route's fault together with the next route's
    R.set_vertex_owners(*owners)
    R.update_parts(**_payload(ALL))
    before = snapshot(R)
    cases = [(dict(null=("group_m3x4",), n=dict(n_bones=N_BONES + 1)), "null matrices"),
             (dict(n=dict(n_groups=4, n_bones=N_BONES + 1)), "n_groups differs"),
             (dict(groups=np.stack([GROUPS[0], GROUPS[1] * 0.0, GROUPS[2]]), n=dict(n_bones=1)), "group 1: det A is zero"),
             (dict(n=dict(n_bones=N_BONES + 1, n_targets=1)), "n_bones differs"),
             (dict(null=("bone_m3x4",), weights=np.array([nan, 0.0])), "null matrices"),
             (dict(null=("morph_weight",), time=nan), "null weights"),
             (dict(n=dict(n_targets=3), time=nan), "n_targets differs"),
             (dict(weights=np.array([0.1, float("inf")]), time=nan), "target 1: the weight is not finite"),
             (dict(time=nan), "the time is not finite")]
    for kw, word in cases:
        st, msg = update(R, ALL, **kw)
        assert st == INVALID and word in msg and msg.startswith("mcpt_update_parts: "), (kw, msg)
        assert same(snapshot(R), before)
    # morph then skin: the bones are the morph route's too -- NULL ones are refused although the skin route does not run
    st, msg = update(R, P.route(P.MORPH), 1, null=("bone_m3x4",))
    assert st == INVALID and "null matrices" in msg
    st, msg = update(R, P.route(P.MORPH) | P.route(P.KEYFRAMES), 1, n=dict(n_bones=2), time=nan)
    assert st == INVALID and "n_bones differs" in msg
    # the _reproject form: the above first, then the camera, then the options
    cam = pkg.scenes.Camera((0.62, 0.55, 2.25), (0.5, 0.45, 0.0), (0.0, 1.0, 0.0), 40.0, W + 1, H)
    with pytest.raises(pkg.McptError, match="the time is not finite"):
        R.update_parts_reproject(camera=cam, **_payload(ALL, time=nan))
    with pytest.raises(pkg.McptError, match="mcpt_update_parts_reproject: width / height differ"):
        R.update_parts_reproject(camera=cam, **_payload(ALL))
    u, keep = R._scene_update(GROUPS, BEND, WEIGHTS, T_MID, False, ALL)
    o = pkg.ReprojectOpts(); o.struct_size = 4
    assert lib.mcpt_update_parts_reproject(R.ctx, C.byref(u), None, C.byref(o)) == INVALID and "struct_size" in lib.mcpt_last_error().decode()
    assert same(snapshot(R), before) and R.reproject_info().reprojections == 0
    # mcpt_set_vertex_owners: its refusals leave the owners as they are
    info = R.parts_info().as_dict()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = owners[1].copy(); bad[nv - 1] = 5
    for args, word in (((ptr(owners[0]), nv - 1, ptr(owners[1]), nv), "differ from the scene's"), ((ptr(owners[0]), nv, None, nv), "null normal_owner"),
                       ((ptr(owners[0]), nv, ptr(bad), nv), "normal %d: owner id 5 > 4" % (nv - 1))):
        assert lib.mcpt_set_vertex_owners(R.ctx, *args) == INVALID and word in lib.mcpt_last_error().decode()
    assert R.parts_info().as_dict() == info
    R.update_parts(**_payload(ALL))                                          # and the next good call is the one before, again
    assert same((snapshot(R)[0], 0, 0), (before[0], 0, 0)) and _counts(R)[0] == before[2][0] + 1
    for r in (plain, bare, R, O):
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_camera", [False, True])
def test_reprojection_follows_the_parts_update(pkg, with_camera):
    small = True
    s = K.scene(pkg, small)
    R, O = _pair(pkg, small)
    owners = _split(pkg, small)
    R.set_vertex_owners(*owners)
    cam = pkg.scenes.Camera((0.62, 0.55, 2.25), (0.5, 0.45, 0.0), (0.0, 1.0, 0.0), 40.0, W, H) if with_camera else None
    routes = P.route(P.GROUPS) | P.route(P.MORPH) | P.route(P.KEYFRAMES)
    v, n = _want(pkg, small, (s.vertex, s.normal), owners, routes, then_skin=True)
    opts = dict(feature_spp=4, feature_seed=3, max_history=16.0)
    for r in (R, O):
        r.clear(); r.render(8, seed=5)
    R.update_parts_reproject(camera=cam, **_payload(routes, True), **opts)
    O.update_vertices_reproject(v, n, camera=cam, **opts)
    assert np.array_equal(bits(R.read_accum()), bits(O.read_accum()))
    ia, ib = R.reproject_info(), O.reproject_info()
    assert (ia.reprojections, ia.pixels_reused) == (ib.reprojections, ib.pixels_reused) == (1, ib.pixels_reused) and ia.pixels_reused > 0.5 * W * H
    assert np.array_equal(bits(R.features()), bits(O.features()))            # the features are held afterwards: a denoise may follow at once
    K.assert_arrays(R, v, n)
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    assert _counts(R) == (1, 1, 1, 1, 1, 1)
    R.close(); O.close()


@pytest.mark.gpu
def test_lifetime_clone_rebuild_replace_and_clear(pkg):
    small = True
    s = K.scene(pkg, small); nv = s.vertex.shape[0]
    R, O = _pair(pkg, small)
    base = R.info().device_bytes
    pi = R.parts_info()
    assert (pi.set, pi.updates, pi.last_routes, pi.device_bytes, pi.last_ms, sum(pi.vertex_records)) == (0, 0, 0, 0, 0.0, 0)
    owners = _split(pkg, small)
    R.set_vertex_owners(*owners)
    pi = R.parts_info()
    assert R.info().device_bytes - base == pi.device_bytes == 2 * (1 + 24) * nv and pi.set == 1      # 1 B per owner, 24 B per scratch record
    assert list(pi.vertex_records) == np.bincount(owners[0], minlength=5).tolist() and list(pi.normal_records) == np.bincount(owners[1], minlength=5).tolist()
    assert pi.vertex_records[P.NONE] == 2 and pi.vertex_records[P.SKIN] == 0
    inter = _interleaved(nv)
    R.set_vertex_owners(*inter)                                              # setting again replaces: the counts follow, nothing more is held
    pi = R.parts_info()
    assert R.info().device_bytes - base == pi.device_bytes == 50 * nv and list(pi.vertex_records) == np.bincount(inter[0], minlength=5).tolist()
    R.clear_vertex_owners()
    assert R.info().device_bytes == base and R.parts_info().set == 0 and R.parts_info().device_bytes == 0
    with pytest.raises(pkg.McptError, match="no owners are set"):
        R.update_parts(**_payload(ALL))
    # a clone carries the owners: the same update gives the same arrays; the source does not move with its clone
    R.set_vertex_owners(*owners)
    routes = P.route(P.GROUPS) | P.route(P.MORPH) | P.route(P.KEYFRAMES)
    clone = R.clone()
    assert clone.parts_info().as_dict() == dict(R.parts_info().as_dict(), updates=0, last_ms=0.0) and clone.info().device_bytes == R.info().device_bytes
    v, n = _want(pkg, small, (s.vertex, s.normal), owners, routes)
    clone.update_parts(**_payload(routes))
    K.assert_arrays(clone, v, n); K.assert_arrays(R, s.vertex, s.normal)
    R.update_parts(**_payload(routes))
    K.assert_same(K.state(pkg, clone, arrays=True), K.state(pkg, R, arrays=True))
    # a rebuild keeps them (they are per record, not per leaf): the next update is the oracle's on rebuilt trees
    R.rebuild(); O.update_vertices(v, n); O.rebuild()
    kw = dict(groups=GROUPS2, weights=WEIGHTS2, time=T_KEY)
    v2, n2 = _want(pkg, small, (v, n), owners, routes, **kw)
    R.update_parts(**_payload(routes, **kw)); O.update_vertices(v2, n2)
    K.assert_arrays(R, v2, n2)
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    pi = R.parts_info(); ui = R.update_info()
    assert (pi.updates, pi.last_routes) == (2, routes) and 0 < pi.last_ms <= ui.last_update_ms
    R.close(); O.close(); clone.close()


@pytest.mark.gpu
def test_parts_updates_between_renders_without_a_sync(pkg):
    small = True
    s = K.scene(pkg, small)
    R, O = _pair(pkg, small)
    owners = _split(pkg, small)
    R.set_vertex_owners(*owners)
    routes = P.route(P.GROUPS) | P.route(P.MORPH) | P.route(P.KEYFRAMES)
    kw_b = dict(groups=GROUPS2, bones=BEND2, weights=WEIGHTS2, time=0.25 * 1.75)
    va, na = _want(pkg, small, (s.vertex, s.normal), owners, routes, then_skin=True)
    vb, nb = _want(pkg, small, (va, na), owners, routes, then_skin=True, **kw_b)
    R.clear()
    R.update_parts(**_payload(routes, True)); R.render(4, seed=9); R.update_parts(**_payload(routes, True, **kw_b))   # nothing in between
    film_a = R.read_accum()
    R.clear(); R.render(4, seed=9)
    film_b = R.read_accum()
    O.update_vertices(va, na); O.sync()
    assert np.array_equal(bits(film_a), bits(render_film(O, 4, 9)))
    O.update_vertices(vb, nb); O.sync()
    assert np.array_equal(bits(film_b), bits(render_film(O, 4, 9))) and not np.array_equal(film_a, film_b)
    K.assert_arrays(R, vb, nb)
    R.close(); O.close()


@pytest.mark.gpu
def test_cli_spin_and_bend_in_one_run(pkg, tmp_path):
    """mcpt_cli --turntable 12 --spin light --bend glossy DEG: one parts update per frame (the camera turns by 30 degrees a frame, so the first
    frames look into the room).  The lamp spins as in the --spin-only run and the sphere bends as in the --bend-only run.  The runs are
    deterministic and differ from the --spin-only run in the sphere alone, so a pixel differs only where a path met the bent sphere: frame 0
    (no bend yet) is the same picture byte for byte in all three runs; frames 1 and 2 differ from the --spin-only run in some pixels and not
    in all of them, and from the --bend-only run, in which the lamp stands still.  (Which pixels exactly is not asserted: a path that meets
    the sphere after a bounce changes a pixel that does not see it.)"""
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))

    def pixels(png):
        ppm = png + ".ppm"
        assert kit.run_cli(["--decode-image", png, ppm]).returncode == 0
        with open(ppm, "rb") as fh:
            return np.frombuffer(fh.read()[-40 * 32 * 3:], np.uint8).reshape(32, 40, 3)

    runs, seen = {}, {}
    for name, args in (("both", ["--spin", "light", "--bend", "glossy", "80"]), ("spin", ["--spin", "light"]), ("bend", ["--bend", "glossy", "80"])):
        out = str(tmp_path / name)
        p = kit.run_cli([obj, "--turntable", "12", "--spp", "4", "--depth", "5", "--deterministic", "--out", out] + args)
        assert p.returncode == 0, p.stderr[-2000:]
        runs[name] = kit.turntable_frames(out)
        seen[name] = [pixels("%s_turn%d.png" % (out, f)) for f in range(3)]
    assert runs["both"][0] == runs["spin"][0] == runs["bend"][0]
    for f in (1, 2):
        assert runs["both"][f] != runs["spin"][f] and runs["both"][f] != runs["bend"][f]
        bent = (seen["both"][f] != seen["spin"][f]).any(axis=2); lit = (seen["both"][f] != seen["bend"][f]).any(axis=2)
        print("frame %d: %d pixels differ from --spin alone, %d from --bend alone" % (f, bent.sum(), lit.sum()))
        assert 0 < bent.sum() < 40 * 32 and lit.sum() > 0
    assert len(set(runs["both"])) == 3
    # with the film carried over, with a swell in front of the bend (morph, then skin), and with the normals recomputed
    for more in (["--reproject", "8"], ["--swell", "glossy", "0.2", "--auto-normals"], ["--dual-quat", "--rebuild-above", "1.0"]):
        q = kit.run_cli([obj, "--turntable", "3", "--spp", "2", "--depth", "5", "--out", str(tmp_path / "more"), "--spin", "light", "--bend", "glossy", "40"] + more)
        assert q.returncode == 0, q.stderr[-2000:]
    # clean errors: the same material twice, and a vertex shared by two parts
    q = kit.run_cli([obj, "--turntable", "3", "--spp", "2", "--out", str(tmp_path / "no"), "--spin", "glossy", "--swell", "glossy", "0.2"])
    assert q.returncode == 2 and "name the same material" in q.stderr
