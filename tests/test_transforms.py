"""Rigid parts moved by per-group transforms on the device: mcpt_set_vertex_groups, mcpt_update_transforms (csrc/transform.hip in
front of the refit), mcpt_update_transforms_reproject, mcpt_get_transform_info and their public surfaces.

The oracle throughout is a second context of the same scene, moved with mcpt_update_vertices to the arrays tests/transform_ref.py computes (numpy,
the kernels' association): fp64 multiply, add, subtract, divide and sqrt are correctly rounded on both sides, so the two contexts hold the same
device arrays and everything downstream is compared BIT FOR BIT, without a tolerance.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from tests import deform_kit as K, kit, transform_ref as T
from tests.deform_kit import CENTRE, FLAGS, H, INVALID, LAMP, M_LAMP, SPHERE, UNSUPPORTED, W
from tests.kit import bits, render_film

NEW_SYMBOLS = ["mcpt_set_vertex_groups", "mcpt_update_transforms", "mcpt_update_transforms_reproject", "mcpt_get_transform_info"]


@functools.lru_cache(maxsize=None)
def _groups(pkg):
    """Group 0 the walls, 1 the sphere, 2 the lamp."""
    s = K.scene(pkg)
    m = s.face[:, 0, 3]
    return pkg.groups_from_faces(s, np.where(m == SPHERE, 1, np.where(m == LAMP, 2, 0)))


def _ref(pkg, matrices, groups=None, rest=None):
    """The arrays the matrices give, by the restatement."""
    s = K.scene(pkg); vg, ng = _groups(pkg) if groups is None else groups
    rv, rn = (s.vertex, s.normal) if rest is None else rest
    return T.transform_vertices(rv, vg, matrices), T.transform_normals(rn, ng, matrices)


def _mats(sphere=None, lamp=None):
    m = T.identity(3)
    if sphere is not None: m[1] = sphere
    if lamp is not None: m[2] = lamp
    return m


M_RIGID = T.about(T.rotation((1, 2, 3), 30.0) @ np.diag([0.8, 0.6, 0.9]), CENTRE, (0.1, 0.2, -0.05))
M_OTHER = T.about(T.rotation((0, 1, 0), -75.0) @ np.diag([0.7, 1.1, 0.7]), CENTRE, (-0.08, 0.1, 0.1))
M_MIRROR = T.about(T.rotation((0, 0, 1), 20.0) @ np.diag([-1.0, 0.9, 1.0]), CENTRE, (0.05, 0.15, 0.0))


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_transform_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, ("set_vertex_groups", "update_transforms", "update_transforms_reproject", "transform_info"))


def test_null_context_is_an_invalid_argument_for_the_transform_calls(pkg):
    lib = pkg.load_library()
    cam = pkg.CameraC(); info = pkg.TransformInfo()
    o = pkg.ReprojectOpts(); o.struct_size = C.sizeof(pkg.ReprojectOpts)
    g = np.zeros(4, np.uint32); gp = g.ctypes.data_as(C.c_void_p)
    m = T.identity(1); mp = m.ctypes.data_as(C.c_void_p)
    assert lib.mcpt_set_vertex_groups(None, gp, 4, gp, 4, 1) == INVALID
    assert lib.mcpt_update_transforms(None, mp, 1) == INVALID
    assert lib.mcpt_update_transforms_reproject(None, mp, 1, None, None) == INVALID
    assert lib.mcpt_update_transforms_reproject(None, mp, 1, C.byref(cam), C.byref(o)) == INVALID
    assert lib.mcpt_get_transform_info(None, C.byref(info)) == INVALID


def test_groups_from_faces(pkg):
    S = pkg.scenes
    m = S._Mesh()
    m.add_quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), 0)      # vertices 0..3, faces 0, 1
    m.add_quad((2, 0, 0), (3, 0, 0), (3, 1, 0), (2, 1, 0), (0, 0, 1), 1)      # vertices 4..7, faces 2, 3
    m.add_vertex((9, 9, 9), (0, 0, 1), (0, 0))                               # vertex 8: no face uses it
    cam = S.Camera((0.5, 0.5, 3.0), (0.5, 0.5, 0.0), (0, 1, 0), 40.0, 8, 8)
    scene = m.finish("two-quads", [S.Material("a"), S.Material("b", radiance=(1, 1, 1))], cam)
    vg, ng = pkg.groups_from_faces(scene, [0, 0, 2, 2])
    assert vg.dtype == np.uint32 and ng.dtype == np.uint32
    assert vg.tolist() == [0, 0, 0, 0, 2, 2, 2, 2, 0] and ng.tolist() == vg.tolist()
    with pytest.raises(ValueError) as e:
        pkg.groups_from_faces(scene, [0, 1, 2, 2])                           # the two triangles of a quad share two vertices
    assert "vertex" in str(e.value)
    with pytest.raises(ValueError):
        pkg.groups_from_faces(scene, [0, 0, 2])
    # a shared NORMAL alone is caught too
    face = scene.face.copy(); face[2:, :, 1] = 0
    shared = S.SceneData(scene.name, scene.vertex, scene.normal, scene.texcoord, face, scene.materials, scene.camera, {})
    with pytest.raises(ValueError) as e:
        pkg.groups_from_faces(shared, [0, 0, 1, 1])
    assert "normal" in str(e.value)
    # S-cornell: the sphere and the lamp have vertices of their own
    vg, ng = _groups(pkg)
    s = K.scene(pkg)
    assert (vg == 1).sum() == np.unique(s.face[s.face[:, 0, 3] == SPHERE][:, :, 0]).size > 1000 and (vg == 2).sum() == 4


def test_restatement_identity_gives_the_rest_pose(pkg):
    s = K.scene(pkg); vg, ng = _groups(pkg)
    v, n = _ref(pkg, T.identity(3))
    assert np.array_equal(v, s.vertex)                                       # (1 x + 0 y) + 0 z + 0 = x exactly
    # normals are normalised again: |n|^2 of the file's 9-digit normals is 1 within 1e-8, the quotient is rounded once more -- the same fp32
    # number the streams hold for all but ties, and a relative change of a few 1e-9 at most
    assert np.abs(n - s.normal).max() <= 1e-8
    ln = np.sqrt((n * n).sum(1))
    assert np.abs(ln - 1.0).max() <= 4 * np.finfo(np.float64).eps
    # ... and from there on the step is a fixed point of the fp32 numbers the shading streams hold, which the raw normals are not: what lets the
    # GPU identity tests ask for bit equality (see deform_kit.unit_rest)
    again = T.transform_normals(n, ng, T.identity(3))
    assert np.array_equal(again.astype(np.float32).view(np.uint32), n.astype(np.float32).view(np.uint32))
    assert np.array_equal(K.unit_rest(pkg, _groups(pkg)[1], 3)[1], n) and not np.array_equal(n.astype(np.float32), s.normal.astype(np.float32))
    # cofactors of the identity are the identity, its determinant 1, and the validation passes
    assert np.array_equal(T.cofactors(T.identity(2)), np.stack([np.eye(3)] * 2)) and T.determinants(T.identity(2)).tolist() == [1.0, 1.0]
    assert T.accepts(T.identity(3), T.group_radius(s.vertex, vg, T.used_vertices(s), 3))
    # cof(A) = det(A) A^-T on a general matrix
    A = M_RIGID[:, :3]
    np.testing.assert_allclose(T.cofactors(M_RIGID[None])[0], np.linalg.det(A) * np.linalg.inv(A).T, rtol=1e-12, atol=1e-15)
    # a rotation about a pivot: lengths from the pivot are kept
    R = T.about(T.rotation((0, 1, 0), 40.0), CENTRE)
    sv = s.vertex[vg == 1]
    out = T.transform_vertices(sv, np.zeros(len(sv), int), R[None])
    np.testing.assert_allclose(np.linalg.norm(out - CENTRE, axis=1), np.linalg.norm(sv - CENTRE, axis=1), rtol=1e-12)


def test_restatement_reflection_flips_the_normal(pkg):
    mirror = np.concatenate([np.diag([-1.0, 1.0, 1.0]), np.zeros((3, 1))], 1)[None]
    assert T.determinants(mirror)[0] == -1.0
    n = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.6, 0.8, 0.0]])
    out = T.transform_normals(n, [0, 0, 0], mirror)
    # cof = det A^-T = -diag(-1, 1, 1) = diag(1, -1, -1): as a line the mirrored normal (-x, y, z), with the sign the reversed winding of the
    # mirrored triangle asks for
    assert np.array_equal(out, n * np.array([1.0, -1.0, -1.0]))
    # the geometric normal of a mirrored triangle (its winding as stored) agrees in sign with the transformed shading normal
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]); shading = np.array([[0.0, 0.0, 1.0]])
    A = T.rotation((1, 1, 0), 35.0) @ np.diag([-1.0, 0.7, 1.2])
    M = np.concatenate([A, np.zeros((3, 1))], 1)[None]
    p = T.transform_vertices(tri, [0, 0, 0], M)
    geo = np.cross(p[1] - p[0], p[2] - p[0])
    assert float(geo @ T.transform_normals(shading, [0], M)[0]) > 0.0
    # degenerate results are left as they are
    assert np.array_equal(T.transform_normals(np.zeros((1, 3)), [0], mirror), np.zeros((1, 3)))
    # the validation: singular, non-finite, out of reach
    r = np.array([0.8])
    assert T.accepts(mirror, r) and not T.accepts(np.zeros((1, 3, 4)), r)
    bad = T.identity(1); bad[0, 1, 3] = np.inf
    assert not T.accepts(bad, r)
    far = T.identity(1); far[0, 0, :] = (1e3, 0.0, 0.0, 1e18)               # |t| alone is at the limit; 1e3 R_g on top of it is a whole ulp (128) over
    assert not T.accepts(far, r) and T.accepts(far, np.array([0.0]))


HOST_PROG = r'''
#include <cstdio>
#include <vector>
#include "transform.h"
// in: per matrix 12 doubles [A | t] and a radius; out: per matrix the 21 doubles of its record, det A and the three rows' reach
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb"); if (!f) return 3;
    std::vector<double> in; double x[13];
    while (std::fread(x, sizeof(double), 13, f) == 13) in.insert(in.end(), x, x + 13);
    std::fclose(f);
    FILE* o = std::fopen(argv[2], "wb"); if (!o) return 3;
    for (size_t i = 0; i < in.size(); i += 13) {
        double rec[XF_RECORD], out[4];
        xf_group_record(&in[i], rec);
        out[0] = xf_record_det(rec);
        for (int r = 0; r < 3; r++) out[1 + r] = xf_row_reach(&in[i] + 4 * r, in[i + 12]);
        std::fwrite(rec, sizeof(double), XF_RECORD, o); std::fwrite(out, sizeof(double), 4, o);
    }
    std::fclose(o);
    return 0; }
'''


@K.needs_hipcc
def test_host_cofactors_and_validation_are_the_restatement_bit_for_bit(pkg, tmp_path):
    """The host half of the feature -- xf_group_record, xf_record_det, xf_row_reach of csrc/transform.hip, what fills the staged table and what
    mcpt_update_transforms validates with -- built into a stand-alone program (no device is touched) against tests/transform_ref.py: the same
    bits, also where a last bit decides (a determinant that cancels to exactly 0, a reach one ulp over the limit)."""
    src = str(tmp_path / "host.cpp")
    open(src, "w").write(HOST_PROG)
    exe = K.build_host_check("host", ["transform.hip"], tmp_path, source=src)
    rng = np.random.default_rng(5)
    m = rng.normal(0.0, 1.0, (400, 3, 4)) * 10.0 ** rng.integers(-8, 9, (400, 1, 1))
    m[:40, 2, :3] = m[:40, 0, :3] * 3.0 + m[:40, 1, :3]                      # nearly singular: heavy cancellation in the determinant
    m[40:60, 2, :3] = 2.0 * m[40:60, 1, :3]                                  # singular: the cofactors of row 0 cancel exactly, det A = 0
    special = np.stack([T.identity(1)[0], M_RIGID, M_MIRROR, M_LAMP, np.zeros((3, 4)), T.identity(1)[0] * 1e160,
                        np.array([[1e3, 0, 0, 1e18], [0, 1, 0, 0], [0, 0, 1, 0.0]]), np.array([[1, 0, 0, 1e18], [0, 1, 0, 0], [0, 0, 1, 0.0]])])
    m = np.concatenate([special, m]); radius = np.concatenate([np.full(len(special), 0.8), rng.uniform(0.0, 2.0, 400)])
    np.concatenate([m.reshape(-1, 12), radius[:, None]], 1).tofile(str(tmp_path / "in.bin"))
    K.run_host_check(exe, tmp_path)
    got = np.fromfile(str(tmp_path / "out.bin")).reshape(-1, 25)
    with np.errstate(all="ignore"):
        want = np.concatenate([m.reshape(-1, 12), T.cofactors(m).reshape(-1, 9), T.determinants(m)[:, None], T.reach(m, radius)], 1)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert (want[40 + len(special):60 + len(special), 21] == 0.0).all() and want[6, 22] > 1e18 and want[7, 22] == 1e18


# ------------------------------------------------------------------------------------------------------------------------ GPU helpers
def _pair(pkg, extra=0, groups=True):
    """The context under test (with S-cornell's three groups) and its oracle."""
    return K.pair(pkg, (lambda R: R.set_vertex_groups(*_groups(pkg), 3)) if groups else None, extra=extra, max_depth=6)


def _check_against_oracle(pkg, R, O, matrices, groups=None, rest=None):
    v, n = _ref(pkg, matrices, groups, rest)
    R.update_transforms(matrices); O.update_vertices(v, n)
    a, b = K.state(pkg, R), K.state(pkg, O)
    K.assert_same(a, b)
    return a


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_identity_leaves_the_scene_as_it_was(pkg):
    R, O = _pair(pkg, extra=pkg.FLAG_COUNT_TRAVERSAL, groups=False)
    rest = K.unit_rest(pkg, _groups(pkg)[1], 3)
    R.update_vertices(*rest); O.update_vertices(*rest)                       # unit-length normals: see deform_kit.unit_rest
    R.reset_counters()
    before = K.state(pkg, R)
    c0 = R.counters(); work0 = c0.box_tests + c0.tri_tests
    ratio0 = R.update_info().wide_area_ratio
    assert work0 > 0 and abs(ratio0 - 1.0) <= 1e-3
    vg, ng = _groups(pkg)
    R.set_vertex_groups(vg, ng, 3)
    K.assert_same(before, K.state(pkg, R))                                   # setting groups moves nothing
    R.reset_counters(); O.reset_counters()
    after = _check_against_oracle(pkg, R, O, T.identity(3), rest=rest)
    K.assert_same(before, after)                                             # traces, shading normals, lights and film: as they were, bit for bit
    cr, co = R.counters(), O.counters()
    assert (cr.box_tests, cr.tri_tests, cr.shaded_hits) == (co.box_tests, co.tri_tests, co.shaded_hits)
    ir, io = R.update_info(), O.update_info()
    assert ir.wide_area_ratio == io.wide_area_ratio and ir.updates == io.updates == 2
    # and against the context before the identity, by §12's identity bounds (a refitted box pads a padded box again)
    work1 = cr.box_tests + cr.tri_tests
    print("[identity] traversal work after / before = %.6f  wide_area_ratio = %.8f" % (work1 / work0, ir.wide_area_ratio))
    assert work1 <= 1.01 * work0 and abs(ir.wide_area_ratio - 1.0) <= 1e-3
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_tree", [False, True])
def test_rigid_move_of_the_sphere(pkg, gpu_tree):
    R, O = _pair(pkg, extra=pkg.FLAG_GPU_BVH_BUILD if gpu_tree else 0)
    m = _mats(sphere=M_RIGID)
    v, _ = _ref(pkg, m)
    vg, _ = _groups(pkg)
    assert v[vg == 1].min() > 0.01 and v[vg == 1].max() < 0.99 and not np.array_equal(v, K.scene(pkg).vertex)   # moved, inside the room
    rest = K.state(pkg, R, film=False)
    moved = _check_against_oracle(pkg, R, O, m)
    assert not np.array_equal(rest["t"], moved["t"])
    info = R.update_info()
    assert info.updates == 1 and info.last_update_ms > 0
    R.close(); O.close()


@pytest.mark.gpu
def test_reflection_turns_the_normals_through_the_cofactors(pkg):
    R, O = _pair(pkg)
    assert np.linalg.det(M_MIRROR[:, :3]) < 0
    _check_against_oracle(pkg, R, O, _mats(sphere=M_MIRROR))
    # cof(A) = det(A) A^-T carries the shading normal the way it carries the triangle's own normal (the cross product of its edges in the stored
    # winding): after the reflection the two are on the same side of every sphere triangle, as they were in the rest pose -- A^-T alone would
    # leave them on opposite sides.  (Pole triangles aside, where a 9-digit normal and a sliver's cross product say little: > 99 % of the hits.)
    s = K.scene(pkg); v, _ = _ref(pkg, _mats(sphere=M_MIRROR))
    o, d = K.rays(pkg)
    t, f, u, w = R.probe_trace4(o[:W * H], d[:W * H])
    on_sphere = (f >= 0) & (s.face[np.maximum(f, 0), 0, 3] == SPHERE)
    assert on_sphere.sum() > 100
    fs = f[on_sphere]
    shade = R.probe_hit_shade(fs, u[on_sphere], w[on_sphere], d[:W * H][on_sphere])

    def geometric(vertex):
        p = vertex[s.face[fs, :, 0]]
        return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])

    side_rest = np.sign((geometric(s.vertex) * s.normal[s.face[fs, :, 1]].mean(1)).sum(1))
    side_now = np.sign((geometric(v) * shade[:, :3]).sum(1))
    assert (side_now == side_rest).mean() > 0.99
    R.close(); O.close()


@pytest.mark.gpu
def test_moved_lamp_moves_the_light_records(pkg):
    R, O = _pair(pkg)
    before = R.probe_lights()
    a = _check_against_oracle(pkg, R, O, _mats(lamp=M_LAMP))
    assert np.array_equal(before[0], a["light_face"]) and not np.array_equal(before[2], a["light_pos"])
    # light_pos64 is the moved corners relative to the creation centre
    s = K.scene(pkg); v, _ = _ref(pkg, _mats(lamp=M_LAMP))
    want = (v[s.face[a["light_face"], :, 0]] - np.array(list(R.info().centre))).reshape(-1, 9)
    assert np.array_equal(bits(want), bits(a["light_pos"]))
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one_per_vertex", "one_group", "empty_group"])
def test_group_counts(pkg, case):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    R, O = _pair(pkg, groups=False)
    rng = np.random.default_rng(11)
    if case == "one_per_vertex":                                             # the widest gather: a record of its own per vertex and per normal
        groups = (np.arange(nv, dtype=np.uint32), nv + np.arange(nn, dtype=np.uint32))
        m = T.identity(nv + nn)
        sphere = _groups(pkg)[0] == 1
        m[:nv][sphere, :, 3] = rng.uniform(-0.004, 0.004, (int(sphere.sum()), 3))   # pure translations for vertices, identity for normals
    elif case == "one_group":
        groups = (np.zeros(nv, np.uint32), np.zeros(nn, np.uint32))
        m = T.about(T.rotation((0, 1, 0), 3.0), (0.5, 0.5, 0.5), (0.01, 0.02, -0.01))[None]
    else:                                                                    # group 3 has no member: its matrix is validated (R_g = 0) and never read
        groups = _groups(pkg)
        m = np.concatenate([_mats(sphere=M_OTHER), T.about(np.diag([1e6, 2.0, 3.0]), (5, 5, 5), (1e17, 0, 0))[None]])
    R.set_vertex_groups(groups[0], groups[1], len(m))
    _check_against_oracle(pkg, R, O, m, groups)
    assert R.transform_info().n_groups == len(m)
    R.close(); O.close()


@pytest.mark.gpu
def test_transforms_are_not_cumulative(pkg):
    R, O = _pair(pkg, groups=False)
    rest = K.unit_rest(pkg, _groups(pkg)[1], 3)
    R.update_vertices(*rest); O.update_vertices(*rest)                       # unit-length normals: see deform_kit.unit_rest
    vg, ng = _groups(pkg)
    R.set_vertex_groups(vg, ng, 3)
    original = K.state(pkg, R)
    R.update_transforms(_mats(sphere=M_RIGID, lamp=M_LAMP))
    moved = _check_against_oracle(pkg, R, O, _mats(sphere=M_OTHER), rest=rest)   # M1 then M2 = M2 alone (the lamp is back, too)
    assert not np.array_equal(moved["film"], original["film"])
    R.update_transforms(_mats(sphere=M_OTHER))                               # the same matrices twice: the same scene
    K.assert_same(K.state(pkg, R), moved)
    back = _check_against_oracle(pkg, R, O, T.identity(3), rest=rest)        # M then identity: what the restatement says ...
    K.assert_same(original, back)                                            # ... which is the original film, traces, normals and lights, bit for bit
    assert R.transform_info().updates == 4 and R.update_info().updates == 5 and O.update_info().updates == 3
    R.close(); O.close()


@pytest.mark.gpu
def test_interplay_with_vertex_updates(pkg):
    R, O = _pair(pkg)
    s = K.scene(pkg); vg, ng = _groups(pkg)
    R.update_transforms(_mats(sphere=M_RIGID))
    v1, n1 = _ref(pkg, _mats(sphere=M_OTHER, lamp=M_LAMP))
    R.update_vertices(v1, n1)                                                # moves the scene, leaves the rest pose alone
    O.update_vertices(v1, n1)
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    _check_against_oracle(pkg, R, O, _mats(sphere=M_RIGID))                   # from the REST pose, not from what update_vertices wrote
    # a second set_vertex_groups takes the current scene as the new rest pose
    R.update_vertices(v1, n1)
    R.set_vertex_groups(vg, ng, 3)
    m = _mats(sphere=T.about(T.rotation((1, 0, 0), 10.0), CENTRE, (0.0, 0.05, 0.0)))
    _check_against_oracle(pkg, R, O, m, rest=(v1, n1))
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["own", "side"])
def test_update_between_renders_without_a_sync(pkg, which):
    import torch
    R, O = _pair(pkg)
    vg, ng = _groups(pkg)
    O.set_vertex_groups(vg, ng, 3)
    m = _mats(sphere=M_RIGID, lamp=M_LAMP)
    if which == "side":
        stream = torch.cuda.Stream()
        R.set_torch_stream(stream)
    R.clear()
    R.render(4, seed=9, first_sample=0); R.update_transforms(m); R.render(4, seed=9, first_sample=4)   # nothing in between
    R.update_transforms(_mats(sphere=M_OTHER)); R.update_transforms(m)       # back-to-back calls through the one stage keep their order
    R.render(2, seed=9, first_sample=8)
    got = R.read_accum()
    O.clear()
    O.render(4, seed=9, first_sample=0); O.sync(); O.update_transforms(m); O.sync(); O.render(4, seed=9, first_sample=4); O.sync()
    O.update_transforms(_mats(sphere=M_OTHER)); O.sync(); O.update_transforms(m); O.sync()
    O.render(2, seed=9, first_sample=8); O.sync()
    assert np.array_equal(bits(got), bits(O.read_accum())) and np.all(got[..., 3] == 10)
    if which == "side":
        R.set_stream(0)
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_camera", [False, True])
def test_reprojection_follows_the_transform(pkg, with_camera):
    R, O = _pair(pkg)
    s = K.scene(pkg)
    cam = pkg.scenes.Camera((0.62, 0.55, 2.25), (0.5, 0.45, 0.0), (0.0, 1.0, 0.0), 40.0, W, H) if with_camera else None
    m = _mats(sphere=T.about(T.rotation((0, 1, 0), 12.0), CENTRE, (0.03, 0.02, 0.0)))
    v, n = _ref(pkg, m)
    opts = dict(feature_spp=4, feature_seed=3, max_history=16.0)
    for r in (R, O):
        r.clear(); r.render(8, seed=5)
    R.update_transforms_reproject(m, camera=cam, **opts)
    O.update_vertices_reproject(v, n, camera=cam, **opts)
    a, b = R.read_accum(), O.read_accum()
    assert np.array_equal(bits(a), bits(b))
    ia, ib = R.reproject_info(), O.reproject_info()
    assert (ia.reprojections, ia.pixels_reused) == (ib.reprojections, ib.pixels_reused) == (1, ib.pixels_reused) and ia.pixels_reused > 0.5 * W * H
    assert np.array_equal(bits(R.features()), bits(O.features()))          # the context holds the new scene's features
    assert R.update_info().updates == 1 and R.transform_info().updates == 1
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    R.close(); O.close()


@pytest.mark.gpu
def test_transform_refusals(pkg):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    vg, ng = _groups(pkg)
    plain = pkg.Renderer(s, max_depth=6, flags=pkg.FLAG_DETERMINISTIC)
    for call in (lambda: plain.set_vertex_groups(vg, ng, 3), lambda: plain.update_transforms(T.identity(3)),
                 lambda: plain.update_transforms_reproject(T.identity(3))):
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % UNSUPPORTED in str(e.value)
    plain.close()
    R = pkg.Renderer(s, max_depth=6, flags=FLAGS(pkg))
    o, d = K.rays(pkg)
    film = render_film(R, 4, 5); trace = R.probe_trace4(o, d); bytes0 = R.info().device_bytes

    def unchanged():
        assert R.update_info().updates == 0 and R.transform_info().updates == 0
        assert np.array_equal(bits(render_film(R, 4, 5)), bits(film))
        for x, y in zip(trace, R.probe_trace4(o, d)):
            assert np.array_equal(bits(x), bits(y))

    def refused(call, status=INVALID):
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % status in str(e.value)
        unchanged()

    refused(lambda: R.update_transforms(T.identity(3)))                      # no groups are set
    bad_id = vg.copy(); bad_id[5] = 3
    bad_nid = ng.copy(); bad_nid[-1] = 7
    for args in ((vg[:-1], ng, 3), (vg, ng[:-1], 3), (vg, ng, 0), (vg, ng, nv + nn + 1), (bad_id, ng, 3), (vg, bad_nid, 3)):
        refused(lambda: R.set_vertex_groups(*args))
        assert R.info().device_bytes == bytes0 and R.transform_info().n_groups == 0
    assert R.lib.mcpt_set_vertex_groups(R.ctx, None, nv, None, nn, 3) == INVALID
    refused(lambda: R.update_transforms(T.identity(3)))                      # still none
    R.set_vertex_groups(vg, ng, 3)
    unchanged()
    radius = T.group_radius(s.vertex, vg, T.used_vertices(s), 3)
    nan = T.identity(3); nan[1, 2, 1] = np.nan
    inf = T.identity(3); inf[2, 0, 3] = np.inf
    flat = _mats(sphere=T.about(np.diag([1.0, 0.0, 1.0]), CENTRE))             # det A = 0
    zero = T.identity(3); zero[0] = 0.0
    huge = T.identity(3); huge[1, :, :3] *= 1e160                            # det A overflows
    far_t = T.identity(3); far_t[1, 1, :] = (0.0, 1e3, 0.0, 1e18)            # |t| alone is at the limit, 1e3 R_g puts the row over it
    far_a = _mats(sphere=np.concatenate([np.diag([2e18, 1.0, 1.0]), np.zeros((3, 1))], 1))
    assert radius[1] > 0
    for m in (nan, inf, flat, zero, huge, far_t, far_a):
        assert not T.accepts(m, radius)                                      # the restatement of the validation agrees
        refused(lambda: R.update_transforms(m))
        refused(lambda: R.update_transforms_reproject(m))
    refused(lambda: R.update_transforms(T.identity(2)))                      # another n_groups
    refused(lambda: R.update_transforms(T.identity(4)))
    assert R.lib.mcpt_update_transforms(R.ctx, None, 3) == INVALID and R.lib.mcpt_update_transforms_reproject(R.ctx, None, 3, None, None) == INVALID
    unchanged()
    # _reproject: the matrices first, then the camera, then the options
    ok = _mats(sphere=M_RIGID)
    assert T.accepts(ok, radius)
    cam = s.camera
    refused(lambda: R.update_transforms_reproject(ok, camera=pkg.scenes.Camera(cam.eye, cam.lookat, cam.up, cam.fovy, W + 1, H)))
    refused(lambda: R.update_transforms_reproject(ok, camera=pkg.scenes.Camera(cam.eye, cam.eye, cam.up, cam.fovy, W, H)))
    refused(lambda: R.update_transforms_reproject(ok, feature_spp=65))
    refused(lambda: R.update_transforms_reproject(ok, max_history=0.5))
    with pytest.raises(pkg.McptError) as e:                                  # a bad matrix is named before a bad camera
        R.update_transforms_reproject(nan, camera=pkg.scenes.Camera(cam.eye, cam.eye, cam.up, cam.fovy, W, H))
    assert "matrix entry" in str(e.value)
    with pytest.raises(pkg.McptError) as e:                                  # ... and a bad camera before bad options
        R.update_transforms_reproject(ok, camera=pkg.scenes.Camera(cam.eye, cam.eye, cam.up, cam.fovy, W, H), feature_spp=65)
    assert "eye == lookat" in str(e.value)
    unchanged()
    R.validate_trees()
    R.update_transforms(ok)                                                  # and the context still works
    assert R.update_info().updates == 1
    R.close()


@pytest.mark.gpu
def test_clone_and_bookkeeping(pkg):
    s = K.scene(pkg); nv, nn = s.vertex.shape[0], s.normal.shape[0]
    R, O = _pair(pkg, groups=False)
    vg, ng = _groups(pkg)
    base = R.info().device_bytes
    assert R.transform_info().n_groups == 0 and R.transform_info().updates == 0
    R.set_vertex_groups(vg, ng, 3)
    assert R.info().device_bytes - base == 24 * (nv + nn) + 4 * (nv + nn) + 168 * 3
    R.set_vertex_groups(vg, ng, 5)                                           # replaces: the old buffers are released
    assert R.info().device_bytes - base == 28 * (nv + nn) + 168 * 5 and R.transform_info().n_groups == 5
    R.set_vertex_groups(vg, ng, 3)
    assert R.info().device_bytes - base == 28 * (nv + nn) + 168 * 3
    R.update_transforms(_mats(sphere=M_RIGID))
    clone = R.clone()
    assert clone.info().device_bytes == R.info().device_bytes
    ti = clone.transform_info()
    assert (ti.n_groups, ti.updates) == (3, 0)
    K.assert_same(K.state(pkg, clone), K.state(pkg, R))                      # the clone is the moved scene ...
    _check_against_oracle(pkg, clone, O, _mats(sphere=M_OTHER, lamp=M_LAMP))  # ... with the ORIGINAL rest pose and the groups
    v, n = _ref(pkg, _mats(sphere=M_RIGID))
    O.update_vertices(v, n)
    K.assert_same(K.state(pkg, R), K.state(pkg, O))                          # the source did not move with its clone
    # R_g travelled too: the clone refuses what the source refuses
    far = T.identity(3); far[1, 1, :] = (0.0, 1e3, 0.0, 1e18)               # refused only because R_g of the sphere is > 0
    for r in (R, clone):
        with pytest.raises(pkg.McptError):
            r.update_transforms(far)
    R.update_transforms(T.identity(3)); R.update_transforms_reproject(T.identity(3))
    ti = R.transform_info()
    assert (ti.n_groups, ti.updates) == (3, 3) and ti.last_ms > 0 and R.update_info().updates == 3
    assert clone.transform_info().updates == 1 and clone.update_info().updates == 1
    assert R.update_info().last_update_ms >= ti.last_ms                      # the refit's bracket spans the transform kernels
    clone.close(); R.close(); O.close()


@pytest.mark.gpu
def test_facade_transforms(pkg, tmp_path):
    exe = kit.build_facade("facade_transforms.cpp", tmp_path)
    a = pkg.scenes.cornell_box(44, 30, sphere_lon=24, sphere_lat=12)
    obj = a.write(str(tmp_path / "a"))
    # the program reads the 9-digit text of the file: the same numbers scenes.py keeps (SceneData is rounded through that text form)
    vg, ng = pkg.groups_from_faces(a, (a.face[:, 0, 3] == SPHERE).astype(int))
    m = np.stack([T.identity(1)[0], M_RIGID])
    T.transform_vertices(a.vertex, vg, m).tofile(str(tmp_path / "v.bin")); T.transform_normals(a.normal, ng, m).tofile(str(tmp_path / "n.bin"))
    M_RIGID.tofile(str(tmp_path / "m.bin"))
    outs = [str(tmp_path / n) for n in ("xf.bin", "upd.bin", "rp.bin")]
    k = 4
    line = kit.run_facade(exe, [obj, "glossy", str(k), str(tmp_path / "m.bin"), str(tmp_path / "v.bin"), str(tmp_path / "n.bin")] + outs)
    w, h = int(line[0]), int(line[1])
    assert (w, h, int(line[2])) == (44, 30, k)
    xf, upd, rp = [np.fromfile(p, np.float32).reshape(h, w, 4) for p in outs]
    assert np.all(xf[..., 3] == k) and xf[..., :3].sum() > 0                 # the picture started again and ends at k samples
    assert np.array_equal(bits(xf), bits(upd))                             # matrices on the device = the restated arrays through update()
    assert np.all(rp[..., 3] >= 1) and np.all(rp[..., 3] <= 5) and (rp[..., 3] > 1).mean() > 0.5   # history capped at 4, plus the new frame


@pytest.mark.gpu
@pytest.mark.parametrize("reproject", [False, True])
def test_cli_spin(pkg, tmp_path, reproject):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    out = str(tmp_path / "img")
    base = [obj, "--turntable", "3", "--spp", "4", "--depth", "5", "--out", out]
    p = kit.run_cli(base + ["--spin", "glossy"] + (["--reproject", "8"] if reproject else []))
    assert p.returncode == 0, p.stderr[-2000:]
    imgs = kit.turntable_frames(out)
    assert imgs[0] != imgs[1] and imgs[1] != imgs[2]
    if not reproject:                                                        # clean errors: an unknown material, --spin without --turntable, a shared vertex
        S = pkg.scenes
        m = S._Mesh()
        m.add_quad((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1), (0, 1, 0), 0)
        m.add_quad((0.3, 0.9, 0.3), (0.7, 0.9, 0.3), (0.7, 0.9, 0.7), (0.3, 0.9, 0.7), (0, -1, 0), 1)
        i = [m.add_vertex(p_, (0, 0, 1), (0, 0)) for p_ in ((0.2, 0.1, 0.2), (0.8, 0.1, 0.2), (0.8, 0.7, 0.2), (0.2, 0.7, 0.2))]
        m.add_tri(i[0], i[1], i[2], 2); m.add_tri(i[0], i[2], i[3], 0)       # one quad, two materials: its diagonal's vertices belong to both
        shared = m.finish("shared", [S.Material("floor", kd=(0.5, 0.5, 0.5)), S.Material("lamp", kd=(0.5, 0.5, 0.5), radiance=(5, 5, 5)),
                                     S.Material("part", kd=(0.6, 0.2, 0.2))], S.Camera((0.5, 0.5, 2.5), (0.5, 0.4, 0.0), (0, 1, 0), 40.0, 24, 16))
        q = kit.run_cli([shared.write(str(tmp_path / "shared")), "--turntable", "2", "--spp", "1", "--out", out, "--spin", "part"])
        assert q.returncode == 1 and "is used by faces of groups" in q.stderr, q.stderr[-2000:]
        q = kit.run_cli(base + ["--spin", "no-such-material"])
        assert q.returncode == 1 and "no material named" in q.stderr
        q = kit.run_cli([obj, "--spin", "glossy"])
        assert q.returncode == 2 and "--turntable" in q.stderr


@pytest.mark.gpu
def test_transform_update_is_not_slower_on_the_device_than_the_upload_it_replaces(pkg):
    """S-bath detail 160 (0.59 M triangles), the fixtures as one group turned by a small angle: device time (mcpt_update_info::last_update_ms, HIP
    events: everything from the first copy to the end of the refit) of mcpt_update_transforms against mcpt_update_vertices fed the identical
    arrays, in the same process, medians of 20 after 3 warm-ups, alternating.  The one claim: the new call's device time is not larger.  The
    figures are in DESIGN.md §16 and profiles/transform_probe.json (tools/transform_probe.py)."""
    scene = pkg.scenes.bathroom_stress(64, 36, detail=160, tex_size=16)
    vg, ng = pkg.groups_from_faces(scene, np.isin(scene.face[:, 0, 3], (5, 6)).astype(int))
    pivot = scene.vertex[vg == 1].mean(0)
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    R.set_vertex_groups(vg, ng, 2)
    xf, up = [], []
    for i in range(23):
        m = np.stack([T.identity(1)[0], T.about(T.rotation((0, 1, 0), 0.5 * (i + 1)), pivot)])
        v, n = T.transform_vertices(scene.vertex, vg, m), T.transform_normals(scene.normal, ng, m)
        R.update_transforms(m); xf.append(R.update_info().last_update_ms)
        R.update_vertices(v, n); up.append(R.update_info().last_update_ms)
    R.validate_trees()
    R.close()
    a, b = float(np.median(xf[3:])), float(np.median(up[3:]))
    print("\n[transforms] %d vertices + %d normals: update_transforms %.3f ms, update_vertices %.3f ms on the device (medians of 20), ratio %.3f" % (
        scene.vertex.shape[0], scene.normal.shape[0], a, b, a / b))
    assert 0 < a <= b
