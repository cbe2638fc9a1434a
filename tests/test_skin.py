"""Deforming parts skinned on the device: mcpt_set_vertex_skin, mcpt_update_skin (csrc/skin.hip in front of the refit),
mcpt_update_skin_reproject, mcpt_get_skin_info and their public surfaces.

The oracle throughout is §16's: a second context of the same scene, moved with mcpt_update_vertices to the arrays tests/skin_ref.py computes
(numpy, the kernels' association): fp64 multiply, add, subtract, divide and sqrt are correctly rounded on both sides, so the two contexts hold
the same device arrays and everything downstream is compared BIT FOR BIT, without a tolerance.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from tests import deform_kit as K, kit, skin_ref as S, transform_ref as T
from tests.deform_kit import CENTRE, FLAGS, H, INVALID, LAMP, M_HIGH, M_LAMP, M_LOW, N_BONES, SPHERE, UNSUPPORTED, W, clean
from tests.kit import bits, render_film

NEW_SYMBOLS = ["mcpt_set_vertex_skin", "mcpt_update_skin", "mcpt_update_skin_reproject", "mcpt_get_skin_info"]
DYADIC = (0.5, 0.25, 0.125, 0.125)                                           # every partial sum and every product with 0 or 1 is exact
M_THIRD = clean(T.about(T.rotation((1, 2, 3), 30.0) @ np.diag([0.8, 0.6, 0.9]), CENTRE, (0.1, 0.2, -0.05)))
M_OTHER = clean(T.about(T.rotation((0, 1, 0), -75.0) @ np.diag([0.7, 1.1, 0.7]), CENTRE, (-0.08, 0.1, 0.1)))
M_UNUSED = clean(T.about(np.diag([1e6, 2.0, 3.0]), (5, 5, 5), (1e17, 0, 0)))     # a bone without members: validated against R_b = 0, never read


@functools.lru_cache(maxsize=None)
def _four(pkg):
    """Every sphere vertex with four random weights normalised in fp64 over bones 1 .. 3, a third of the slots exactly 0 with a random id of
    ANY bone in them; walls on bone 0, lamp on bone 4."""
    sphere, lamp = K.parts(pkg); n = int(sphere.sum())
    rng = np.random.default_rng(23)
    vb, vw = S.single(np.where(lamp, 4, 0))
    r = rng.uniform(0.05, 1.0, (n, 4)); ids = rng.integers(1, 4, (n, 4))
    zero = rng.uniform(size=(n, 4)) < 1.0 / 3.0
    zero[:, 0] &= ~zero.all(1)                                               # at least one slot carries weight
    r[zero] = 0.0; ids[zero] = rng.integers(0, N_BONES, int(zero.sum()))
    w = r / r.sum(1, keepdims=True)
    assert (w == 0.0).sum() == zero.sum() > n and np.abs(S.weight_sums(w) - 1.0).max() <= 4 * np.finfo(np.float64).eps
    vb[sphere] = ids; vw[sphere] = w
    return (vb, vw) + tuple(pkg.skin_normals_from_faces(K.scene(pkg), vb, vw))


def _mats(low=None, high=None, lamp=None, third=None):
    """deform_kit.mats with the far-away bone 3 this suite always had there."""
    return K.mats(low, high, lamp, M_UNUSED if third is None else third)


def _ref(pkg, matrices, skin=None, rest=None):
    """The arrays the bones give, by the restatement."""
    s = K.scene(pkg); vb, vw, nb, nw = K.bend(pkg) if skin is None else skin
    rv, rn = (s.vertex, s.normal) if rest is None else rest
    return S.skin_vertices(rv, vb, vw, matrices), S.skin_normals(rn, nb, nw, matrices)


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_skin_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, ("set_vertex_skin", "update_skin", "update_skin_reproject", "skin_info"))
    assert pkg.SKIN_INFLUENCES == S.INFLUENCES == 4 and callable(pkg.skin_normals_from_faces)
    assert set(pkg.SkinInfo().as_dict()) == {"struct_size", "n_bones", "updates", "last_ms"}


def test_null_context_is_an_invalid_argument_for_the_skin_calls(pkg):
    lib = pkg.load_library()
    cam = pkg.CameraC(); info = pkg.SkinInfo()
    o = pkg.ReprojectOpts(); o.struct_size = C.sizeof(pkg.ReprojectOpts)
    b, w = S.single(np.zeros(4, int)); bp, wp = b.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)
    m = T.identity(1); mp = m.ctypes.data_as(C.c_void_p)
    assert lib.mcpt_set_vertex_skin(None, bp, wp, 4, bp, wp, 4, 1) == INVALID
    assert lib.mcpt_update_skin(None, mp, 1) == INVALID
    assert lib.mcpt_update_skin_reproject(None, mp, 1, None, None) == INVALID
    assert lib.mcpt_update_skin_reproject(None, mp, 1, C.byref(cam), C.byref(o)) == INVALID
    assert lib.mcpt_get_skin_info(None, C.byref(info)) == INVALID


def test_skin_info_has_the_headers_layout(pkg, tmp_path):
    """sizeof and every offsetof of mcpt_skin_info as a C compiler sees include/mcpt.h, against the ctypes class; MCPT_SKIN_INFLUENCES."""
    c, py, macros = K.c_layout(pkg.SkinInfo, "mcpt_skin_info", tmp_path, macros=("MCPT_SKIN_INFLUENCES",))
    assert c == py
    assert macros == [pkg.SKIN_INFLUENCES]


def test_skin_normals_from_faces(pkg):
    Sc = pkg.scenes
    m = Sc._Mesh()
    m.add_quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), 0)      # vertices 0..3, faces 0, 1
    m.add_quad((2, 0, 0), (3, 0, 0), (3, 1, 0), (2, 1, 0), (0, 0, 1), 1)      # vertices 4..7, faces 2, 3
    m.add_vertex((9, 9, 9), (0, 0, 1), (0, 0))                               # vertex and normal 8: no face uses them
    cam = Sc.Camera((0.5, 0.5, 3.0), (0.5, 0.5, 0.0), (0, 1, 0), 40.0, 8, 8)
    scene = m.finish("two-quads", [Sc.Material("a"), Sc.Material("b", radiance=(1, 1, 1))], cam)
    rng = np.random.default_rng(2)
    vb = rng.integers(0, 3, (9, 4)).astype(np.uint32); vw = rng.uniform(0, 1, (9, 4)); vw /= vw.sum(1, keepdims=True)
    nb, nw = pkg.skin_normals_from_faces(scene, vb, vw)
    assert nb.dtype == np.uint32 and nw.dtype == np.float64 and nb.shape == nw.shape == (9, 4)
    pairs = {int(c[1]): int(c[0]) for f in scene.face for c in f}            # normal -> the vertex it is paired with
    assert sorted(pairs) == list(range(8))
    for n_, v_ in pairs.items():
        assert np.array_equal(nb[n_], vb[v_]) and np.array_equal(bits(nw[n_]), bits(vw[v_]))
    assert nb[8].tolist() == [0, 0, 0, 0] and nw[8].tolist() == [1.0, 0.0, 0.0, 0.0]      # unused: bone 0 with weight 1
    with pytest.raises(ValueError):
        pkg.skin_normals_from_faces(scene, vb[:-1], vw[:-1])
    # a normal shared by vertices whose records differ is refused and named; by vertices with the same record it is not
    face = scene.face.copy(); face[2:, :, 1] = 5
    shared = Sc.SceneData(scene.name, scene.vertex, scene.normal, scene.texcoord, face, scene.materials, scene.camera, {})
    with pytest.raises(ValueError) as e:
        pkg.skin_normals_from_faces(shared, vb, vw)
    assert "normal 5" in str(e.value)
    same_w = vw.copy(); same_w[4:8] = vw[4]; same_b = vb.copy(); same_b[4:8] = vb[4]
    nb, nw = pkg.skin_normals_from_faces(shared, same_b, same_w)
    assert np.array_equal(nb[5], same_b[4]) and nb[4].tolist() == [0, 0, 0, 0] and nw[4].tolist() == [1.0, 0.0, 0.0, 0.0]
    one_bit = same_w.copy(); one_bit[6, 0] = np.nextafter(one_bit[6, 0], 2.0)    # the records are compared bit for bit
    with pytest.raises(ValueError):
        pkg.skin_normals_from_faces(shared, same_b, one_bit)
    # S-cornell: every normal is paired with one vertex, so the bend's normals carry their vertices' records
    s = K.scene(pkg); vb, vw, nb, nw = K.bend(pkg)
    assert nb.shape == (s.normal.shape[0], 4)
    assert np.array_equal(nb[s.face[:, :, 1]], vb[s.face[:, :, 0]]) and np.array_equal(bits(nw[s.face[:, :, 1]]), bits(vw[s.face[:, :, 0]]))
    assert K.parts(pkg)[0].sum() > 1000 and K.parts(pkg)[1].sum() == 4 and s.vertex.shape[0] == s.normal.shape[0] == 1249


def test_restatement_identity_and_single_influence(pkg):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    rng = np.random.default_rng(4)
    # identity bones with dyadic weights: the blend is the identity exactly, whatever ids the slots name
    ids_v = rng.integers(0, 3, (nv, 4)); ids_n = rng.integers(0, 3, (nn, 4))
    dy_v = np.tile(DYADIC, (nv, 1)); dy_n = np.tile(DYADIC, (nn, 1))
    assert np.array_equal(bits(S.blend(ids_v, dy_v, T.identity(3))), bits(np.broadcast_to(T.identity(1), (nv, 3, 4))))
    assert np.array_equal(S.skin_vertices(s.vertex, ids_v, dy_v, T.identity(3)), s.vertex)
    unit = S.skin_normals(s.normal, ids_n, dy_n, T.identity(3))
    assert np.array_equal(bits(unit), bits(T.transform_normals(s.normal, np.zeros(nn, int), T.identity(1))))
    # ... and normals normalised once are a fixed point of the step in the fp32 numbers the shading streams hold (what the GPU identity test needs)
    again = S.skin_normals(unit, ids_n, dy_n, T.identity(3))
    assert np.array_equal(bits(again.astype(np.float32)), bits(unit.astype(np.float32)))
    # one influence of weight 1 (the other slots: weight 0 on bone 0) gives transform_ref's arrays bit for bit for matrices without -0.0
    sphere, lamp = K.parts(pkg)
    group = np.where(sphere, 1, np.where(lamp, 2, 0))
    m = np.stack([T.identity(1)[0], M_THIRD, M_LAMP])
    assert not np.signbit(m[m == 0.0]).any()
    vb, vw = S.single(group)
    nb, nw = pkg.skin_normals_from_faces(s, vb, vw)                          # (every normal of S-cornell is paired with the vertex of its own number)
    assert np.array_equal(nb, vb) and np.array_equal(bits(nw), bits(vw))
    assert np.array_equal(bits(S.skin_vertices(s.vertex, vb, vw, m)), bits(T.transform_vertices(s.vertex, group, m)))
    assert np.array_equal(bits(S.skin_normals(s.normal, nb, nw, m)), bits(T.transform_normals(s.normal, group, m)))
    # ... and a -0.0 entry is where a skipped slot would show: 1 * -0.0 + 0 * 1 = +0.0, all four slots are accumulated
    neg = T.identity(2); neg[1, 0, 1] = -0.0
    b, w = S.single([1])
    assert not np.signbit(S.blend(b, w, neg)[0, 0, 1]) and np.signbit(neg[1, 0, 1])
    w0 = np.array([[0.0, 1.0, 0.0, 0.0]]); b0 = np.array([[1, 0, 1, 1]])      # 0 * -0.0 = -0.0 survives only while every term is -0.0
    assert np.signbit(S.blend(b0, w0, np.stack([neg[1], neg[1]]))[0, 0, 1])


def test_restatement_blends_matrices_the_way_positions_blend(pkg):
    """Linear-blend skinning: the blended matrix applied to a point is the blend of the transformed points, to rounding."""
    s = K.scene(pkg); vb, vw, nb, nw = _four(pkg)
    m = _mats(low=M_LOW, high=M_HIGH, third=M_THIRD, lamp=M_LAMP)
    got = S.skin_vertices(s.vertex, vb, vw, m)
    each = np.stack([T.transform_vertices(s.vertex, vb[:, k], m) for k in range(4)], 1)          # (n, 4, 3)
    want = (vw[:, :, None] * each).sum(1)
    assert np.abs(got - want).max() <= 1e-15
    assert not np.array_equal(got, s.vertex) and got[K.parts(pkg)[0]].min() > 0.01 and got[K.parts(pkg)[0]].max() < 0.99
    # normals come out unit length wherever the blend is regular
    n = S.skin_normals(s.normal, nb, nw, m)
    assert np.abs(np.sqrt((n * n).sum(1)) - 1.0).max() <= 4 * np.finfo(np.float64).eps
    # two opposed rotations blended half and half are singular: cof = 0, the normal is left as it is (the zero vector)
    quarter = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0]])      # 90 degrees about y, its entries exact
    opposed = np.stack([quarter, quarter * np.array([[-1.0], [1.0], [-1.0]])]) + 0.0
    assert T.determinants(opposed).tolist() == [1.0, 1.0]
    flat = S.skin_normals(np.array([[1.0, 0.0, 0.0], [0.6, 0.0, 0.8]]), [[0, 1, 0, 0]] * 2, [[0.5, 0.5, 0.0, 0.0]] * 2, opposed)
    assert np.array_equal(flat, np.zeros((2, 3)))


def test_restatement_refusals(pkg):
    s = K.scene(pkg); vb, vw, nb, nw = K.bend(pkg)
    assert S.accepts_skin(vb, vw, N_BONES) and S.accepts_skin(nb, nw, N_BONES) and S.accepts_skin(*_four(pkg)[:2], N_BONES)
    # the weight sum: 1e-6 is the limit, fp32-normalised weights pass
    for scale, ok in ((1.0 + 0.9e-6, True), (1.0 - 0.9e-6, True), (1.0 + 1.2e-6, False), (1.0 - 1.2e-6, False)):
        w = vw.copy(); w[7] = np.array(DYADIC) * scale
        assert S.accepts_skin(vb, w, N_BONES) == ok, scale
    r32 = np.random.default_rng(1).uniform(0, 1, (1000, 4)).astype(np.float32); r32 /= r32.sum(1, keepdims=True)
    assert np.abs(S.weight_sums(r32.astype(np.float64)) - 1.0).max() < 5e-7 and S.accepts_skin(np.zeros((1000, 4), int), r32.astype(np.float64), 1)
    for bad in (np.nan, np.inf, -0.25, 1.5):
        w = vw.copy(); w[7] = (bad, 0.0, 0.0, 0.0)
        assert not S.accepts_skin(vb, w, N_BONES)
    # an id in a zero-weight slot counts
    b = vb.copy(); assert vw[7, 3] == 0.0
    b[7, 3] = N_BONES
    assert not S.accepts_skin(b, vw, N_BONES) and S.accepts_skin(b, vw, N_BONES + 1)
    # R_b: only vertices that a face uses and that give the bone a weight > 0
    used = T.used_vertices(s); sphere, lamp = K.parts(pkg)
    radius = S.bone_radius(s.vertex, vb, vw, used, N_BONES)
    far = np.abs(s.vertex).max(1)
    lower = sphere & (vw[:, 0] > 0.0); upper = sphere & (vw[:, 1] > 0.0)
    assert radius[3] == 0.0 and radius[4] == far[lamp].max() and radius[1] == far[lower].max() and radius[2] == far[upper].max()
    assert radius[0] == far[~sphere & ~lamp & used].max() and 0 < lower.sum() < sphere.sum() and 0 < upper.sum() < sphere.sum()   # (the pole rings give one of the two bones no weight)
    # the reach carries the slack factor: a row exactly at the limit passes mcpt_update_transforms' check and not this one
    assert S.accepts(_mats(low=M_LOW, high=M_HIGH, lamp=M_LAMP), radius)
    edge = T.identity(N_BONES); edge[3, 0, :] = (1.0, 0.0, 0.0, 1e18)
    assert T.accepts(edge, radius) and not S.accepts(edge, radius)
    edge[3, 0, 3] = 1e18 / (1.0 + 2.0 ** -15)
    assert S.accepts(edge, radius)
    for bad in (np.nan, np.inf):
        m = T.identity(N_BONES); m[2, 1, 2] = bad
        assert not S.accepts(m, radius)
    flat = T.identity(N_BONES); flat[1] = T.about(np.diag([1.0, 0.0, 1.0]), CENTRE)
    huge = T.identity(N_BONES); huge[1, :, :3] *= 1e160
    assert not S.accepts(flat, radius) and not S.accepts(huge, radius) and not S.accepts(T.identity(N_BONES - 1), radius)
    far_a = T.identity(N_BONES); far_a[2, 0, 0] = 2e18
    assert not S.accepts(far_a, radius) and S.accepts(far_a, np.zeros(N_BONES))


@K.needs_hipcc
def test_host_determinant_and_reach_are_the_restatement_bit_for_bit(pkg, tmp_path):
    """The host half of the feature -- sk_bone_det and sk_row_reach of csrc/skin.hip, what mcpt_update_skin validates with -- built into the
    stand-alone program tests/skin_host_check.cpp (no device is touched) against tests/skin_ref.py: the same bits, also where a last bit
    decides (a determinant that cancels to exactly 0, a reach at the limit that the slack factor puts over it)."""
    exe = K.build_host_check("skin_host_check", ["skin.hip", "transform.hip"], tmp_path)
    rng = np.random.default_rng(5)
    m = rng.normal(0.0, 1.0, (400, 3, 4)) * 10.0 ** rng.integers(-8, 9, (400, 1, 1))
    m[:40, 2, :3] = m[:40, 0, :3] * 3.0 + m[:40, 1, :3]                      # nearly singular: heavy cancellation in the determinant
    m[40:60, 2, :3] = 2.0 * m[40:60, 1, :3]                                  # singular: the cofactors of row 0 cancel exactly, det A = 0
    special = np.stack([T.identity(1)[0], M_THIRD, M_LAMP, np.zeros((3, 4)), T.identity(1)[0] * 1e160,
                        np.array([[1, 0, 0, 1e18], [0, 1, 0, 0], [0, 0, 1, 0.0]]), np.array([[1, 0, 0, 1e18 / (1.0 + 2.0 ** -15)], [0, 1, 0, 0], [0, 0, 1, 0.0]])])
    m = np.concatenate([special, m]); radius = np.concatenate([np.full(len(special), 0.8), rng.uniform(0.0, 2.0, 400)])
    np.concatenate([m.reshape(-1, 12), radius[:, None]], 1).tofile(str(tmp_path / "in.bin"))
    K.run_host_check(exe, tmp_path)
    got = np.fromfile(str(tmp_path / "out.bin")).reshape(-1, 4)
    with np.errstate(all="ignore"):
        want = np.concatenate([T.determinants(m)[:, None], S.reach(m, radius)], 1)
    assert np.array_equal(bits(got), bits(want))
    assert (want[40 + len(special):60 + len(special), 0] == 0.0).all() and want[5, 1] > 1e18 and want[6, 1] <= 1e18


# ------------------------------------------------------------------------------------------------------------------------ GPU helpers
def _pair(pkg, extra=0, skin="bend"):
    """The context under test (with the five-bone bend, or `skin`, or none) and its oracle."""
    setup = None if skin is None else lambda R: R.set_vertex_skin(*(K.bend(pkg) if skin == "bend" else skin), N_BONES)
    return K.pair(pkg, setup, extra=extra, max_depth=6)


def _check_against_oracle(pkg, R, O, matrices, skin=None, rest=None):
    v, n = _ref(pkg, matrices, skin, rest)
    R.update_skin(matrices); O.update_vertices(v, n)
    a, b = K.state(pkg, R), K.state(pkg, O)
    K.assert_same(a, b)
    return a


BEND = _mats(low=M_LOW, high=M_HIGH, lamp=M_LAMP)
BEND2 = _mats(low=M_OTHER, high=M_THIRD)


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("gpu_tree", [False, True])
def test_bend_of_the_sphere_with_a_moved_lamp(pkg, gpu_tree):
    R, O = _pair(pkg, extra=pkg.FLAG_GPU_BVH_BUILD if gpu_tree else 0)
    v, _ = _ref(pkg, BEND)
    sphere, lamp = K.parts(pkg)
    assert v[sphere].min() > 0.01 and v[sphere].max() < 0.99 and not np.array_equal(v[sphere], K.scene(pkg).vertex[sphere])   # bent, inside the room
    assert np.array_equal(v[~sphere & ~lamp], K.scene(pkg).vertex[~sphere & ~lamp])                                        # the walls stay
    rest = K.state(pkg, R, film=False)
    before = R.probe_lights()
    moved = _check_against_oracle(pkg, R, O, BEND)
    assert not np.array_equal(rest["t"], moved["t"])
    assert np.array_equal(before[0], moved["light_face"]) and not np.array_equal(before[2], moved["light_pos"])
    want = (v[K.scene(pkg).face[moved["light_face"], :, 0]] - np.array(list(R.info().centre))).reshape(-1, 9)   # the nine fp64 positions per light
    assert np.array_equal(bits(want), bits(moved["light_pos"]))
    info = R.update_info(); si = R.skin_info()
    assert info.updates == 1 and info.last_update_ms > 0 and (si.n_bones, si.updates) == (N_BONES, 1) and 0 < si.last_ms <= info.last_update_ms
    R.close(); O.close()


@pytest.mark.gpu
def test_four_influences_with_zero_weight_slots(pkg):
    skin = _four(pkg)
    R, O = _pair(pkg, skin=skin)
    m = _mats(low=M_LOW, high=M_HIGH, third=M_THIRD, lamp=M_LAMP)
    v, _ = _ref(pkg, m, skin)
    sphere = K.parts(pkg)[0]
    assert v[sphere].min() > 0.01 and v[sphere].max() < 0.99
    _check_against_oracle(pkg, R, O, m, skin)
    R.close(); O.close()


@pytest.mark.gpu
def test_identity_bones_leave_the_scene_as_it_was(pkg):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    R, O = _pair(pkg, skin=None)
    rest = K.unit_rest(pkg)
    R.update_vertices(*rest); O.update_vertices(*rest)                       # unit-length normals: see deform_kit.unit_rest
    before = K.state(pkg, R)
    rng = np.random.default_rng(8)
    vb = rng.integers(0, 3, (nv, 4)); nb = rng.integers(0, 3, (nn, 4))         # dyadic weights on any mix of identity bones: the identity exactly
    skin = (vb, np.tile(DYADIC, (nv, 1)), nb, np.tile(DYADIC, (nn, 1)))
    R.set_vertex_skin(*skin, 3)
    K.assert_same(before, K.state(pkg, R))                                   # setting a skin moves nothing
    after = _check_against_oracle(pkg, R, O, T.identity(3), skin, rest)
    K.assert_same(before, after)                                             # traces, shading normals, lights and film: as they were, bit for bit
    assert R.update_info().updates == O.update_info().updates == 2 and R.update_info().wide_area_ratio == O.update_info().wide_area_ratio
    R.close(); O.close()


@pytest.mark.gpu
def test_single_influence_is_update_transforms(pkg):
    s = K.scene(pkg); sphere, lamp = K.parts(pkg)
    R, X = _pair(pkg, skin=None)
    vg, ng = pkg.groups_from_faces(s, np.where(s.face[:, 0, 3] == SPHERE, 1, np.where(s.face[:, 0, 3] == LAMP, 2, 0)))
    X.set_vertex_groups(vg, ng, 3)
    R.set_vertex_skin(*S.single(vg), *S.single(ng), 3)
    m = np.stack([T.identity(1)[0], M_THIRD, M_LAMP])                          # (made + 0.0-clean above)
    R.update_skin(m); X.update_transforms(m)
    K.assert_same(K.state(pkg, R), K.state(pkg, X))
    R.close(); X.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one_bone", "one_bone_per_record"])
def test_extreme_bone_counts(pkg, case):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    rng = np.random.default_rng(11)
    wv = rng.uniform(0.1, 1.0, (nv, 4)); wv /= wv.sum(1, keepdims=True); wn = rng.uniform(0.1, 1.0, (nn, 4)); wn /= wn.sum(1, keepdims=True)
    if case == "one_bone":                                                   # every slot of every record names bone 0; the weights only sum to 1 within rounding
        skin = (np.zeros((nv, 4), np.uint32), wv, np.zeros((nn, 4), np.uint32), wn)
        m = clean(T.about(T.rotation((0, 1, 0), 3.0), (0.5, 0.5, 0.5), (0.01, 0.02, -0.01)))[None]
    else:                                                                    # the widest gather: a matrix of its own per vertex and per normal
        skin = (np.repeat(np.arange(nv), 4).reshape(nv, 4), wv, np.repeat(nv + np.arange(nn), 4).reshape(nn, 4), wn)
        m = T.identity(nv + nn)
        sphere = K.parts(pkg)[0]
        m[:nv][sphere, :, 3] = rng.uniform(-0.004, 0.004, (int(sphere.sum()), 3))   # pure translations for vertices, identity for normals
    R, O = _pair(pkg, skin=None)
    R.set_vertex_skin(*skin, len(m))
    _check_against_oracle(pkg, R, O, m, skin)
    assert R.skin_info().n_bones == len(m)
    R.close(); O.close()


@pytest.mark.gpu
def test_bones_are_not_cumulative_and_sequences(pkg):
    R, O = _pair(pkg, skin=None)
    rest = K.unit_rest(pkg)
    R.update_vertices(*rest); O.update_vertices(*rest)                       # unit-length normals: see deform_kit.unit_rest
    R.set_vertex_skin(*K.bend(pkg), N_BONES)
    original = K.state(pkg, R)
    R.update_skin(BEND)
    moved = _check_against_oracle(pkg, R, O, BEND2, rest=rest)               # M1 then M2 = M2 alone (the lamp is back, too)
    assert not np.array_equal(moved["film"], original["film"])
    R.update_skin(BEND2)                                                     # the same bones twice: the same scene
    K.assert_same(K.state(pkg, R), moved)
    back = _check_against_oracle(pkg, R, O, _mats(), rest=rest)              # M then identity: what the restatement says ...
    K.assert_same(original, back)                                            # ... which is the original film, traces, normals and lights, bit for bit
    assert R.skin_info().updates == 4 and R.update_info().updates == 5 and O.update_info().updates == 3
    # update_vertices in between moves the scene and leaves the skin's rest pose alone
    v1, n1 = _ref(pkg, BEND2, rest=rest)
    R.update_vertices(v1, n1); O.update_vertices(v1, n1)
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    _check_against_oracle(pkg, R, O, BEND, rest=rest)                        # from the REST pose, not from what update_vertices wrote
    # a second set_vertex_skin takes the current scene as the new rest pose -- and may change the skin
    R.update_vertices(v1, n1)
    R.set_vertex_skin(*_four(pkg), N_BONES)
    small = _mats(low=clean(T.about(T.rotation((1, 0, 0), 10.0), CENTRE, (0.0, 0.03, 0.0))), high=clean(T.about(np.eye(3), CENTRE, (0.01, 0.02, 0.0))), third=T.identity(1)[0])
    _check_against_oracle(pkg, R, O, small, _four(pkg), (v1, n1))
    R.close(); O.close()


@pytest.mark.gpu
def test_groups_and_skin_on_one_context(pkg):
    s = K.scene(pkg)
    R, O = _pair(pkg, skin=None)
    vg, ng = pkg.groups_from_faces(s, np.where(s.face[:, 0, 3] == SPHERE, 1, np.where(s.face[:, 0, 3] == LAMP, 2, 0)))
    gm = np.stack([T.identity(1)[0], clean(T.about(T.rotation((0, 1, 0), 15.0), CENTRE, (0.05, 0.0, 0.05))), M_LAMP])
    gm2 = np.stack([T.identity(1)[0], clean(T.about(np.eye(3), CENTRE, (-0.05, 0.02, 0.0))), T.identity(1)[0]])

    def groups_oracle(m):
        O.update_vertices(T.transform_vertices(s.vertex, vg, m), T.transform_normals(s.normal, ng, m))
        K.assert_same(K.state(pkg, R), K.state(pkg, O))

    R.set_vertex_groups(vg, ng, 3)                                           # the groups' rest pose: the scene as created
    R.update_transforms(gm); groups_oracle(gm)
    posed = (T.transform_vertices(s.vertex, vg, gm), T.transform_normals(s.normal, ng, gm))
    R.set_vertex_skin(*K.bend(pkg), N_BONES)                                 # the skin's OWN rest pose: the scene as the groups left it
    small = _mats(low=clean(T.about(T.rotation((0, 0, 1), 5.0), CENTRE)), high=clean(T.about(T.rotation((0, 0, 1), -12.0), CENTRE, (0.0, 0.04, 0.0))))
    _check_against_oracle(pkg, R, O, small, rest=posed)
    R.update_transforms(gm2); groups_oracle(gm2)                             # each call overwrites the other's result and reads its own rest pose
    _check_against_oracle(pkg, R, O, BEND, rest=posed)
    R.update_transforms(gm); groups_oracle(gm)
    assert R.transform_info().updates == 3 and R.skin_info().updates == 2 and R.update_info().updates == 5
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["own", "side"])
def test_update_between_renders_without_a_sync(pkg, which):
    import torch
    R, O = _pair(pkg)
    O.set_vertex_skin(*K.bend(pkg), N_BONES)
    if which == "side":
        stream = torch.cuda.Stream()
        R.set_torch_stream(stream)
    R.clear()
    R.render(4, seed=9, first_sample=0); R.update_skin(BEND); R.render(4, seed=9, first_sample=4)   # nothing in between
    R.update_skin(BEND2); R.update_skin(BEND)                                # back-to-back calls through the one stage keep their order
    R.render(2, seed=9, first_sample=8)
    got = R.read_accum()
    O.clear()
    O.render(4, seed=9, first_sample=0); O.sync(); O.update_skin(BEND); O.sync(); O.render(4, seed=9, first_sample=4); O.sync()
    O.update_skin(BEND2); O.sync(); O.update_skin(BEND); O.sync()
    O.render(2, seed=9, first_sample=8); O.sync()
    assert np.array_equal(bits(got), bits(O.read_accum())) and np.all(got[..., 3] == 10)
    if which == "side":
        R.set_stream(0)
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_camera", [False, True])
def test_reprojection_follows_the_skin(pkg, with_camera):
    R, O = _pair(pkg)
    cam = pkg.scenes.Camera((0.62, 0.55, 2.25), (0.5, 0.45, 0.0), (0.0, 1.0, 0.0), 40.0, W, H) if with_camera else None
    m = _mats(low=clean(T.about(T.rotation((0, 0, 1), 3.0), CENTRE)), high=clean(T.about(T.rotation((0, 0, 1), -10.0), CENTRE, (0.02, 0.02, 0.0))))
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
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    R.close(); O.close()


@pytest.mark.gpu
def test_skin_refusals(pkg):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    vb, vw, nb, nw = K.bend(pkg)
    plain = pkg.Renderer(s, max_depth=6, flags=pkg.FLAG_DETERMINISTIC)
    for call in (lambda: plain.set_vertex_skin(vb, vw, nb, nw, N_BONES), lambda: plain.update_skin(_mats()), lambda: plain.update_skin_reproject(_mats())):
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % UNSUPPORTED in str(e.value)
    plain.close()
    R = pkg.Renderer(s, max_depth=6, flags=FLAGS(pkg))
    o, d = K.rays(pkg)
    film = render_film(R, 4, 5); trace = R.probe_trace4(o, d); bytes0 = R.info().device_bytes
    expect = {"n_bones": 0}

    def unchanged():
        si = R.skin_info()
        assert R.update_info().updates == 0 and (si.n_bones, si.updates) == (expect["n_bones"], 0)
        assert np.array_equal(bits(render_film(R, 4, 5)), bits(film))
        for x, y in zip(trace, R.probe_trace4(o, d)):
            assert np.array_equal(bits(x), bits(y))

    def refused(call, status=INVALID):
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % status in str(e.value)
        unchanged()
        return str(e.value)

    refused(lambda: R.update_skin(_mats()))                                  # no skin is set
    # ---- mcpt_set_vertex_skin
    def edit(a, i, k, x):
        a = a.copy(); a[i, k] = x
        return a

    assert vw[5, 3] == 0.0 and nw[-1, 2] == 0.0
    bad_sets = [(vb[:-1], vw[:-1], nb, nw, N_BONES), (vb, vw, nb[:-1], nw[:-1], N_BONES),                  # counts that differ from the scene's
                (vb, vw, nb, nw, 0), (vb, vw, nb, nw, 4 * (nv + nn) + 1),                                  # n_bones outside [1, 4 (n_vertex + n_normal)]
                (edit(vb, 5, 3, N_BONES), vw, nb, nw, N_BONES), (vb, vw, edit(nb, nn - 1, 2, 7), nw, N_BONES),   # an id >= n_bones in a ZERO-weight slot
                (edit(vb, 700, 0, N_BONES), vw, nb, nw, N_BONES)]                                          # ... and in a slot that carries weight
    for x in (np.nan, np.inf, -0.25, 1.5):                                   # a weight that is not finite or is outside [0, 1]
        bad_sets.append((vb, edit(vw, 9, 1, x), nb, nw, N_BONES))
    bad_sets.append((vb, vw, nb, edit(nw, 3, 0, np.nan), N_BONES))
    for scale in (1.0 + 1.2e-6, 1.0 - 1.2e-6):                               # |S - 1| > 1e-6
        w = vw.copy(); w[7] = np.array(DYADIC) * scale
        bad_sets.append((vb, w, nb, nw, N_BONES))
        w = nw.copy(); w[nn - 2] = np.array(DYADIC) * scale
        bad_sets.append((vb, vw, nb, w, N_BONES))
    for args in bad_sets:
        assert not (len(args[0]) == nv and len(args[2]) == nn and 1 <= args[4] <= 4 * (nv + nn) and S.accepts_skin(args[0], args[1], args[4]) and S.accepts_skin(args[2], args[3], args[4]))
        refused(lambda: R.set_vertex_skin(*args))
        assert R.info().device_bytes == bytes0
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    vb32, nb32 = np.ascontiguousarray(vb, np.uint32), np.ascontiguousarray(nb, np.uint32)
    for args in ((None, P(vw), nv, P(nb32), P(nw), nn), (P(vb32), None, nv, P(nb32), P(nw), nn), (P(vb32), P(vw), nv, None, P(nw), nn), (P(vb32), P(vw), nv, P(nb32), None, nn)):
        assert R.lib.mcpt_set_vertex_skin(R.ctx, *args, N_BONES) == INVALID  # a NULL array
    unchanged()
    assert R.info().device_bytes == bytes0
    w = vw.copy(); w[7] = np.array(DYADIC) * (1.0 + 0.9e-6)                  # inside the tolerance: accepted, and used as given
    R.set_vertex_skin(vb, w, nb, nw, N_BONES)
    R.set_vertex_skin(vb, vw, nb, nw, N_BONES)
    expect["n_bones"] = N_BONES
    unchanged()
    for args in bad_sets[:6]:                                                # a refused replacement leaves the skin that is set
        refused(lambda: R.set_vertex_skin(*args))
    # ---- mcpt_update_skin and _reproject
    radius = S.bone_radius(s.vertex, vb, vw, T.used_vertices(s), N_BONES)
    nan = _mats(); nan[1, 2, 1] = np.nan
    inf = _mats(); inf[2, 0, 3] = np.inf
    flat = _mats(low=T.about(np.diag([1.0, 0.0, 1.0]), CENTRE))               # det A = 0
    zero = _mats(); zero[0] = 0.0
    huge = _mats(); huge[1, :, :3] *= 1e160                                  # det A overflows
    far_t = _mats(); far_t[1, 1, :] = (0.0, 1e3, 0.0, 1e18)                  # |t| alone is at the limit, 1e3 R_b puts the row over it
    far_a = _mats(high=np.concatenate([np.diag([2e18, 1.0, 1.0]), np.zeros((3, 1))], 1))
    edge = _mats(third=np.array([[1.0, 0, 0, 1e18], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]))   # at the limit: only the slack factor refuses it, on a bone without members
    assert radius[1] > 0 and radius[2] > 0 and radius[3] == 0 and T.accepts(edge, radius)
    for m in (nan, inf, flat, zero, huge, far_t, far_a, edge):
        assert not S.accepts(m, radius)                                      # the restatement of the validation agrees
        refused(lambda: R.update_skin(m))
        refused(lambda: R.update_skin_reproject(m))
    refused(lambda: R.update_skin(T.identity(N_BONES - 1)))                  # another n_bones
    refused(lambda: R.update_skin(T.identity(N_BONES + 1)))
    assert R.lib.mcpt_update_skin(R.ctx, None, N_BONES) == INVALID and R.lib.mcpt_update_skin_reproject(R.ctx, None, N_BONES, None, None) == INVALID
    unchanged()
    # the order: no skin / n_bones before the entries, the entries before the determinant, the determinant before the reach
    both = nan.copy(); both[2] = flat[1]
    assert "not finite" in refused(lambda: R.update_skin(both))
    both = flat.copy(); both[2] = far_a[2]
    assert "det A" in refused(lambda: R.update_skin(both))
    # _reproject: the matrices first, then the camera, then the options
    assert S.accepts(BEND, radius)
    cam = s.camera
    refused(lambda: R.update_skin_reproject(BEND, camera=pkg.scenes.Camera(cam.eye, cam.lookat, cam.up, cam.fovy, W + 1, H)))
    refused(lambda: R.update_skin_reproject(BEND, camera=pkg.scenes.Camera(cam.eye, cam.eye, cam.up, cam.fovy, W, H)))
    refused(lambda: R.update_skin_reproject(BEND, feature_spp=65))
    refused(lambda: R.update_skin_reproject(BEND, max_history=0.5))
    with pytest.raises(pkg.McptError) as e:                                  # a bad matrix is named before a bad camera
        R.update_skin_reproject(nan, camera=pkg.scenes.Camera(cam.eye, cam.eye, cam.up, cam.fovy, W, H))
    assert "matrix entry" in str(e.value)
    with pytest.raises(pkg.McptError) as e:                                  # ... and a bad camera before bad options
        R.update_skin_reproject(BEND, camera=pkg.scenes.Camera(cam.eye, cam.eye, cam.up, cam.fovy, W, H), feature_spp=65)
    assert "eye == lookat" in str(e.value)
    unchanged()
    R.validate_trees()
    R.update_skin(BEND)                                                      # and the context still works
    assert R.update_info().updates == 1 and R.skin_info().updates == 1
    R.close()


@pytest.mark.gpu
def test_clone_rebuild_and_bookkeeping(pkg):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    R, O = _pair(pkg, skin=None)
    base = R.info().device_bytes
    assert R.skin_info().n_bones == 0 and R.skin_info().updates == 0
    R.set_vertex_skin(*K.bend(pkg), N_BONES)
    per_record = 24 + 16 + 32                                                # rest pose, ids, weights
    assert R.info().device_bytes - base == per_record * (nv + nn) + 96 * N_BONES
    R.set_vertex_skin(*K.bend(pkg), N_BONES + 4)                             # replaces: the old buffers are released
    assert R.info().device_bytes - base == per_record * (nv + nn) + 96 * (N_BONES + 4) and R.skin_info().n_bones == N_BONES + 4
    R.set_vertex_skin(*K.bend(pkg), N_BONES)
    assert R.info().device_bytes - base == per_record * (nv + nn) + 96 * N_BONES
    R.update_skin(BEND)
    clone = R.clone()
    assert clone.info().device_bytes == R.info().device_bytes
    si = clone.skin_info()
    assert (si.n_bones, si.updates) == (N_BONES, 0)
    K.assert_same(K.state(pkg, clone), K.state(pkg, R))                      # the clone is the bent scene ...
    _check_against_oracle(pkg, clone, O, BEND2)                              # ... with the ORIGINAL rest pose and the skin
    v, n = _ref(pkg, BEND)
    O.update_vertices(v, n)
    K.assert_same(K.state(pkg, R), K.state(pkg, O))                          # the source did not move with its clone
    far = _mats(); far[1, 1, 1] = 2e18                                       # R_b travelled too: refused only because R_b of the lower bone is > 0
    for r in (R, clone):
        with pytest.raises(pkg.McptError):
            r.update_skin(far)
    # a rebuild keeps skin, rest pose and R_b: update_skin afterwards equals the oracle context rebuilt the same way
    for builder in (pkg.REBUILD_HOST, pkg.REBUILD_DEVICE):
        R.rebuild(builder); O.rebuild(builder)
        assert R.skin_info().n_bones == N_BONES
        K.assert_same(K.state(pkg, R), K.state(pkg, O))
        _check_against_oracle(pkg, R, O, BEND2 if builder == pkg.REBUILD_HOST else BEND)
        with pytest.raises(pkg.McptError):
            R.update_skin(far)
    assert R.info().device_bytes == O.info().device_bytes + per_record * (nv + nn) + 96 * N_BONES
    R.update_skin(_mats()); R.update_skin_reproject(_mats())
    si = R.skin_info()
    assert (si.n_bones, si.updates) == (N_BONES, 5) and si.last_ms > 0 and R.update_info().updates == 5
    assert clone.skin_info().updates == 1 and clone.update_info().updates == 1
    assert R.update_info().last_update_ms >= si.last_ms                      # the refit's bracket spans the table's copy and the skinning kernels
    clone.close(); R.close(); O.close()


@pytest.mark.gpu
def test_facade_skin(pkg, tmp_path):
    exe = kit.build_facade("facade_skin.cpp", tmp_path)
    a = pkg.scenes.cornell_box(44, 30, sphere_lon=24, sphere_lat=12)
    obj = a.write(str(tmp_path / "a"))
    # the program reads the 9-digit text of the file: the same numbers scenes.py keeps (SceneData is rounded through that text form)
    vb, vw, nb, nw = K.height_skin(pkg, a, a.face[:, 0, 3] == SPHERE)
    m = np.stack([T.identity(1)[0], M_LOW, M_HIGH])
    vb.astype(np.uint32).tofile(str(tmp_path / "b.bin")); vw.tofile(str(tmp_path / "w.bin")); m.tofile(str(tmp_path / "m.bin"))
    S.skin_vertices(a.vertex, vb, vw, m).tofile(str(tmp_path / "v.bin")); S.skin_normals(a.normal, nb, nw, m).tofile(str(tmp_path / "n.bin"))
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
def test_cli_bend(pkg, tmp_path, reproject):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    out = str(tmp_path / "img")
    base = [obj, "--turntable", "3", "--spp", "4", "--depth", "5", "--out", out]
    p = kit.run_cli(base + ["--bend", "glossy", "25"] + (["--reproject", "8"] if reproject else []))
    assert p.returncode == 0, p.stderr[-2000:]
    imgs = kit.turntable_frames(out)
    assert imgs[0] != imgs[1] and imgs[1] != imgs[2]
    if not reproject:                                                        # clean errors
        q = kit.run_cli(base + ["--bend", "no-such-material", "25"])
        assert q.returncode == 1 and "no material named" in q.stderr
        for other in (["--wobble", "0.01"], ["--spin", "glossy"]):
            q = kit.run_cli(base + ["--bend", "glossy", "25"] + other)
            assert q.returncode == 2 and "--bend" in q.stderr
        q = kit.run_cli([obj, "--bend", "glossy", "25"])
        assert q.returncode == 2 and "--turntable" in q.stderr
        q = kit.run_cli(base + ["--bend", "glossy", "25", "--rebuild-above", "1.0"])
        assert q.returncode == 0, q.stderr[-2000:]


@pytest.mark.gpu
def test_skin_update_is_not_slower_on_the_device_than_the_upload_it_replaces(pkg):
    """S-bath detail 160 (0.59 M triangles), the fixtures bent by two bones: device time (mcpt_update_info::last_update_ms, HIP events: everything
    from the first copy to the end of the refit) of mcpt_update_skin against mcpt_update_vertices fed the identical restated arrays, in the same
    process, medians of 20 after 3 warm-ups, alternating.  The one claim: the new call's device time is not larger.  The figures are in
    DESIGN.md §18 and profiles/skin_probe.json (tools/skin_probe.py)."""
    scene = pkg.scenes.bathroom_stress(64, 36, detail=160, tex_size=16)
    part = np.isin(scene.face[:, 0, 3], (5, 6))
    vb, vw, nb, nw = K.height_skin(pkg, scene, part)
    pivot = scene.vertex[np.unique(scene.face[part][:, :, 0])].mean(0)
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    R.set_vertex_skin(vb, vw, nb, nw, 3)
    sk, up = [], []
    for i in range(23):
        m = np.stack([T.identity(1)[0], T.identity(1)[0], T.about(T.rotation((0, 0, 1), 0.5 * (i + 1)), pivot)])
        v, n = S.skin_vertices(scene.vertex, vb, vw, m), S.skin_normals(scene.normal, nb, nw, m)
        R.update_skin(m); sk.append(R.update_info().last_update_ms)
        R.update_vertices(v, n); up.append(R.update_info().last_update_ms)
    R.validate_trees()
    R.close()
    a, b = float(np.median(sk[3:])), float(np.median(up[3:]))
    print("\n[skin] %d vertices + %d normals: update_skin %.3f ms, update_vertices %.3f ms on the device (medians of 20), ratio %.3f" % (
        scene.vertex.shape[0], scene.normal.shape[0], a, b, a / b))
    assert 0 < a <= b
