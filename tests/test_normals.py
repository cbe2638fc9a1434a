"""Smooth normals recomputed on the device after every scene update: mcpt_set_auto_normals, mcpt_update_normals,
mcpt_get_normals_info (csrc/normals.hip between every update route and the refit) and their public surfaces.

The reference throughout is tests/normals_ref.py (numpy, the kernel's order of summation): fp64 subtract, multiply, add, divide and sqrt are
correctly rounded on both sides, so everything is compared BIT FOR BIT, without a tolerance -- directly, through mcpt_probe_vertices, and
downstream through §16's oracle: a second context of the same scene, WITHOUT the feature, moved with mcpt_update_vertices to the restated
vertex and normal arrays.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from tests import deform_kit as K, kit, morph_ref as M, normals_ref as N, skin_ref as S, transform_ref as T
from tests.deform_kit import CENTRE, FLAGS, H, INVALID, LAMP, M_LAMP, M_LOW, N_BONES, SPHERE, UNSUPPORTED, W, clean
from tests.kit import bits, render_film

NEW_SYMBOLS = ["mcpt_set_auto_normals", "mcpt_update_normals", "mcpt_get_normals_info"]
FAN = 70                                                                     # triangles around the apex of the hand-made scene


M_HIGH = clean(T.about(T.rotation((0, 0, 1), 25.0) @ np.diag([0.9, 0.7, 0.9]), (0.5, 0.1, 0.5), (0.03, 0.08, -0.04)))   # (squashes more than deform_kit's)
M_SQUASH = clean(T.about(T.rotation((1, 0, 0), 20.0) @ np.diag([1.0, 0.6, 0.8]), CENTRE, (0.1, 0.2, -0.05)))
BEND = K.mats(low=M_LOW, high=M_HIGH, lamp=M_LAMP)                           # §18's bend: 0 the walls, 1 and 2 the sphere's bones, 3 nobody, 4 the lamp
GROUPS = np.stack([T.identity(1)[0], M_SQUASH, M_LAMP])                      # 0 the walls, 1 the sphere, 2 the lamp
WEIGHTS = np.array([0.35, -0.6])


# ------------------------------------------------------------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def _scene(pkg, which="big"):
    """deform_kit's S-cornell (1 249 normal records), S-cornell-small (349, two of them unused), or the hand-made fan."""
    return _fan_scene(pkg) if which == "fan" else K.scene(pkg, which == "small")


def _fan_scene(pkg):
    """The open box (walls and the lamp quad; the vertices and normals of its dropped 3 x 2 sphere stay as unused records) plus: a cone of FAN
    triangles whose apex corners all name ONE normal record, the LAST of the array (valence FAN: the sphere fixtures never exceed 6); one
    zero-area face (three collinear points whose x and z agree: every cross-product term cancels exactly) with a record of its own; and one
    face that names a single record in all three corners."""
    b = pkg.scenes.open_box(W, H)
    nv, nn = b.vertex.shape[0], b.normal.shape[0]
    ang = 2.0 * np.pi * np.arange(FAN) / FAN
    rim = np.stack([0.5 + 0.3 * np.cos(ang), np.full(FAN, 0.15), 0.5 + 0.3 * np.sin(ang)], 1)
    rim_n = np.stack([np.cos(ang), np.full(FAN, 0.6), np.sin(ang)], 1); rim_n /= np.linalg.norm(rim_n, axis=1, keepdims=True)
    extra_v = np.concatenate([rim, [[0.5, 0.45, 0.5]],                                          # rim nv .. nv + FAN - 1, apex nv + FAN
                              [[0.2, 0.1, 0.2], [0.3, 0.1, 0.3], [0.4, 0.1, 0.4]],              # the zero-area face
                              [[0.1, 0.6, 0.1], [0.3, 0.6, 0.1], [0.2, 0.7, 0.3]]])             # the single-record face
    apex_v, z_v, s_v = nv + FAN, nv + FAN + 1, nv + FAN + 4
    extra_n = np.concatenate([rim_n, [[0.0, 1.0, 0.0]], [[0.0, -0.6, 0.8]], [[0.0, 1.0, 0.0]]])   # rim, the zero-area face's, the single record, apex LAST
    z_n, s_n, apex_n = nn + FAN, nn + FAN + 1, nn + FAN + 2
    faces = []
    for i in range(FAN):
        j = (i + 1) % FAN
        faces.append([[apex_v, apex_n, 0, SPHERE], [nv + j, nn + j, 0, SPHERE], [nv + i, nn + i, 0, SPHERE]])
    faces.append([[z_v, z_n, 0, 0], [z_v + 1, z_n, 0, 0], [z_v + 2, z_n, 0, 0]])
    faces.append([[s_v, s_n, 0, 1], [s_v + 1, s_n, 0, 1], [s_v + 2, s_n, 0, 1]])
    face = np.concatenate([b.face, np.array(faces, b.face.dtype)])
    s = pkg.scenes.SceneData("fan", np.concatenate([b.vertex, extra_v]), np.concatenate([b.normal, extra_n]), b.texcoord, face, b.materials, b.camera, {"kind": "fan"})
    assert apex_n == s.normal.shape[0] - 1
    return s


def _part(scene, mtl):
    """The vertices of the faces of material `mtl`, as a boolean mask."""
    mask = np.zeros(scene.vertex.shape[0], bool); mask[np.unique(scene.face[scene.face[:, 0, 3] == mtl][:, :, 0])] = True
    return mask


def _mask(pkg, scene, which):
    """None (all records) or the records of the sphere's faces."""
    return None if which == "all" else pkg.normal_mask_from_faces(scene, scene.face[:, 0, 3] == SPHERE)


def _moved(pkg, scene, step=1):
    """(vertex, caller normals): the sphere translated and squashed (kit.moved_sphere; the normals are the analytic ones) and the lamp shifted."""
    s = kit.moved_sphere(pkg, scene, shift=(0.12 / step, 0.25 / step, -0.1 / step), squash=0.6 if step == 1 else 0.8)
    v = s.vertex.copy(); v[_part(scene, LAMP)] += np.array([0.1, -0.2, 0.05]) / step
    return v, s.normal + 0.0


@functools.lru_cache(maxsize=None)
def _targets(pkg, which="big"):
    """Two vertex targets and NO normal targets (the case glTF tells a client to recompute normals for): a lopsided swell of the sphere and a
    lift of its upper half together with the lamp."""
    s = _scene(pkg, which); si = np.flatnonzero(_part(s, SPHERE)); li = np.flatnonzero(_part(s, LAMP))
    p = s.vertex[si] - CENTRE
    up = si[s.vertex[si, 1] > 0.3]
    both = np.concatenate([li, up]); both.sort()
    return [(si, p * np.array([0.5, -0.3, 0.2])), (both, np.tile((0.05, -0.1, 0.02), (len(both), 1)))]


ROUTES = ["vertices", "vertices_with_normals", "transforms", "skin", "morph", "morph_then_skin"]


def _prepare(pkg, R, which, route):
    """The set-up a route needs on the context under test.  All of them are taken at the rest pose."""
    s = _scene(pkg, which)
    if route == "transforms":
        vg, ng = pkg.groups_from_faces(s, np.where(s.face[:, 0, 3] == SPHERE, 1, np.where(s.face[:, 0, 3] == LAMP, 2, 0)))
        R.set_vertex_groups(vg, ng, 3)
    if route in ("skin", "morph_then_skin"):
        R.set_vertex_skin(*K.bend(pkg, which == "small"), N_BONES)
    if route in ("morph", "morph_then_skin"):
        R.set_vertex_morph(_targets(pkg, which), None)


def _route(pkg, R, which, route, current_normal, reproject=None):
    """Runs the route on R (reproject: the keyword arguments of its _reproject form) and returns what the ROUTE writes by its own restatement:
    (vertex, normal) -- before the normals pass."""
    s = _scene(pkg, which)
    if route in ("vertices", "vertices_with_normals"):
        v, n = _moved(pkg, s)
        given = n if route == "vertices_with_normals" else None
        R.update_vertices(v, given) if reproject is None else R.update_vertices_reproject(v, given, **reproject)
        return v, (n if given is not None else current_normal)
    if route == "transforms":
        vg, ng = pkg.groups_from_faces(s, np.where(s.face[:, 0, 3] == SPHERE, 1, np.where(s.face[:, 0, 3] == LAMP, 2, 0)))
        R.update_transforms(GROUPS) if reproject is None else R.update_transforms_reproject(GROUPS, **reproject)
        return T.transform_vertices(s.vertex, vg, GROUPS), T.transform_normals(s.normal, ng, GROUPS)
    if route == "skin":
        vb, vw, nb, nw = K.bend(pkg, which == "small")
        R.update_skin(BEND) if reproject is None else R.update_skin_reproject(BEND, **reproject)
        return S.skin_vertices(s.vertex, vb, vw, BEND), S.skin_normals(s.normal, nb, nw, BEND)
    vt = _targets(pkg, which)
    if route == "morph":
        R.update_morph(WEIGHTS) if reproject is None else R.update_morph_reproject(WEIGHTS, **reproject)
        return M.morph_vertices(s.vertex, vt, WEIGHTS), M.morph_normals(s.normal, None, WEIGHTS)
    R.update_morph(WEIGHTS, BEND) if reproject is None else R.update_morph_reproject(WEIGHTS, BEND, **reproject)
    return M.morph_then_skin(s.vertex, s.normal, vt, None, WEIGHTS, K.bend(pkg, which == "small"), BEND)


def _brute_lists(face, n_normal, mask=None):
    """Per record the faces that name it, ascending, by the plainest loop there is."""
    lists = [[] for _ in range(n_normal)]
    for f in range(face.shape[0]):
        for r in sorted(set(int(x) for x in face[f, :, 1])):
            if mask is None or mask[r]:
                lists[r].append(f)
    return lists


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_normals_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, ("set_auto_normals", "update_normals", "normals_info"))
    assert set(pkg.NormalsInfo().as_dict()) == {"struct_size", "mode", "records", "max_valence", "entries", "updates", "last_ms"}
    assert (pkg.NORMALS_OFF, pkg.NORMALS_AREA) == (0, 1)


def test_null_context_is_an_invalid_argument_for_the_normals_calls(pkg):
    lib = pkg.load_library()
    info = pkg.NormalsInfo(); o = pkg.NormalsOpts(); o.struct_size = C.sizeof(pkg.NormalsOpts); o.mode = pkg.NORMALS_AREA
    mask = np.ones(4, np.uint8)
    assert lib.mcpt_set_auto_normals(None, None, 4, None) == INVALID
    assert lib.mcpt_set_auto_normals(None, mask.ctypes.data_as(C.c_void_p), 4, C.byref(o)) == INVALID
    assert lib.mcpt_update_normals(None) == INVALID
    assert lib.mcpt_get_normals_info(None, C.byref(info)) == INVALID


def test_normals_structs_have_the_headers_layout(pkg, tmp_path):
    """sizeof and every offsetof of mcpt_normals_opts and mcpt_normals_info as a C compiler sees include/mcpt.h, against the ctypes classes."""
    for cls, name, size in ((pkg.NormalsOpts, "mcpt_normals_opts", 24), (pkg.NormalsInfo, "mcpt_normals_info", 56)):
        c, py, modes = K.c_layout(cls, name, tmp_path, macros=("MCPT_NORMALS_OFF", "MCPT_NORMALS_AREA"))
        assert c == py and c[0] == size and modes == [0, 1]


def test_mask_from_faces(pkg):
    s = _scene(pkg, "small")
    sphere = s.face[:, 0, 3] == SPHERE
    m = pkg.normal_mask_from_faces(s, sphere)
    assert m.dtype == np.uint8 and m.shape == (349,) and m.sum() == np.unique(s.face[sphere][:, :, 1]).size == 323
    assert pkg.normal_mask_from_faces(s, np.zeros(s.face.shape[0], bool)).sum() == 0
    assert pkg.normal_mask_from_faces(s, np.ones(s.face.shape[0], bool)).sum() == 347          # two records that no face uses
    with pytest.raises(ValueError):
        pkg.normal_mask_from_faces(s, sphere[:-1])


def test_restatement_on_a_planar_grid():
    """A planar grid gives exactly (0, 0, +-1), and the sign follows the reference normals -- whichever way the faces wind."""
    xs = np.array([0.0, 0.3, 1.1, 1.7]); ys = np.array([-0.4, 0.2, 0.9])
    gx, gy = np.meshgrid(xs, ys)
    v = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.25)], 1)
    idx = np.arange(gx.size).reshape(gx.shape)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    tri = np.concatenate([np.stack([a, b, c], 1), np.stack([a, d, c], 1)])    # the two halves of a cell wind in OPPOSITE senses
    face = np.zeros((tri.shape[0], 3, 4), np.int32); face[:, :, 0] = tri; face[:, :, 1] = tri
    for sign in (1.0, -1.0):
        ref = np.tile((0.1, -0.2, sign * 0.7), (v.shape[0], 1))              # not unit, not axis-aligned: only its side matters
        out = N.auto_normals(face, v, ref)
        assert np.array_equal(bits(out), bits(np.tile((0.0, 0.0, sign), (v.shape[0], 1))))
        off, entry = N.per_record(face, v.shape[0], v, ref)
        assert 0 < entry[:, 3].sum() < entry.shape[0]                        # both windings occur, and flip tells them apart


def test_restatement_properties(pkg):
    s = _scene(pkg, "small"); nn = s.normal.shape[0]
    moved, _ = _moved(pkg, s)
    off, entry = N.per_record(s.face, nn, s.vertex, s.normal)
    count = np.diff(off.astype(np.int64))
    # the figures DESIGN.md §20 quotes for this scene: 1 620 entries, 12 of them flipped (the walls whose winding disagrees with their normals),
    # no record with both signs, two unused records, valence at most 6 (the UV sphere has one pole vertex per meridian)
    assert entry.shape[0] == 1620 and entry[:, 3].sum() == 12 and (count == 0).sum() == 2 and count.max() == 6
    for i in np.flatnonzero(count):
        assert len(set(entry[off[i]:off[i + 1], 3].tolist())) == 1
    # the lists are the faces that name the record, ascending -- whatever the order the records first appear in
    lists = _brute_lists(s.face, nn)
    fv = s.face[:, :, 0]
    for i in range(nn):
        assert np.array_equal(entry[off[i]:off[i + 1], :3], fv[lists[i]].astype(np.uint32).reshape(-1, 3)), i
    perm = np.random.default_rng(4).permutation(s.face.shape[0])            # the same faces in another order: other lists, each again ascending
    off_p, entry_p = N.per_record(s.face[perm], nn, s.vertex, s.normal)
    lists_p = _brute_lists(s.face[perm], nn)
    for i in range(nn):
        assert np.array_equal(entry_p[off_p[i]:off_p[i + 1], :3], fv[perm][lists_p[i]].astype(np.uint32).reshape(-1, 3)), i
    # swapping the second and third corner of any face changes no output bit: cross(b, a) is cross(a, b) negated exactly (every term is the
    # same two products subtracted the other way round), and flip, taken at the reference pose, follows it.  (The kernel's cross is anchored
    # at corner 0; no dot of this scene's non-degenerate faces is exactly 0.)
    swapped = s.face.copy(); swapped[:, [1, 2]] = s.face[:, [2, 1]]
    for f in (s.face, swapped):
        g = N._cross(s.vertex[f[:, 0, 0]], s.vertex[f[:, 1, 0]], s.vertex[f[:, 2, 0]])
        for c in range(3):
            d = (g * s.normal[f[:, c, 1]]).sum(1)
            assert not ((d == 0) & (np.abs(g).sum(1) > 0)).any()
    a = N.auto_normals(s.face, moved, s.normal, ref_vertex=s.vertex, ref_normal=s.normal)
    b = N.auto_normals(swapped, moved, s.normal, ref_vertex=s.vertex, ref_normal=s.normal)
    assert np.array_equal(bits(a), bits(b)) and not np.array_equal(a, s.normal)
    off_s, entry_s = N.per_record(swapped, nn, s.vertex, s.normal)
    area = np.abs(N._cross(s.vertex[entry[:, 0]], s.vertex[entry[:, 1]], s.vertex[entry[:, 2]])).sum(1) > 0
    assert np.array_equal(entry_s[area, 3], 1 - entry[area, 3])
    # written records are unit vectors on their reference normal's side; the two unused records are the input's bits
    used = count > 0
    assert np.abs(np.linalg.norm(a[used], axis=1) - 1.0).max() <= 4 * np.finfo(np.float64).eps
    assert np.array_equal(bits(a[~used]), bits(s.normal[~used]))
    rest = N.auto_normals(s.face, s.vertex, s.normal)
    assert ((rest[used] * s.normal[used]).sum(1) > 0.9).all()
    # a mask: the records it leaves out have no entries and keep the input's bits
    mask = pkg.normal_mask_from_faces(s, s.face[:, 0, 3] == SPHERE)
    off_m, entry_m = N.per_record(s.face, nn, s.vertex, s.normal, mask)
    assert (np.diff(off_m.astype(np.int64))[mask == 0] == 0).all() and entry_m.shape[0] == 1620 - 36 and entry_m[:, 3].sum() == 0
    m = N.auto_normals(s.face, moved, s.normal, mask, s.vertex, s.normal)
    assert np.array_equal(bits(m[mask == 0]), bits(s.normal[mask == 0])) and np.array_equal(bits(m[mask != 0]), bits(a[mask != 0]))


def test_restatement_on_degenerate_records(pkg):
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2.0, 2, 2], [3, 3, 3], [4, 4, 4], [0, 0, 1.0]])
    n = np.array([[0.0, 0, 1], [0.3, 0.4, 0.5], [0, 0, -2.0], [9.0, 9, 9], [0.0, np.nan, 0.0]])
    face = np.zeros((4, 3, 4), np.int32)
    face[0, :, 0] = (0, 1, 2); face[0, :, 1] = (0, 0, 2)                     # record 0 in two corners of one face: ONE entry
    face[1, :, 0] = (3, 4, 5); face[1, :, 1] = (1, 1, 1)                     # zero area (collinear): record 1 is left unwritten
    face[2, :, 0] = (0, 2, 6); face[2, :, 1] = (4, 4, 4)                     # a NaN reference normal: flip = 0
    face[3, :, 0] = (3, 3, 3); face[3, :, 1] = (1, 1, 1)                     # zero area again (one point)
    off, entry = N.per_record(face, 5, v, n)
    assert off.tolist() == [0, 1, 3, 4, 4, 5] and entry[0].tolist() == [0, 1, 2, 0] and entry[3].tolist() == [0, 1, 2, 1] and entry[4, 3] == 0
    out = N.apply(off, entry, v, n)
    assert np.array_equal(bits(out[[1, 3]]), bits(n[[1, 3]]))                # all faces of zero area / no face at all: not written
    assert np.array_equal(bits(out[0]), bits(np.array([0.0, 0.0, 1.0]))) and np.array_equal(bits(out[2]), bits(np.array([0.0, 0.0, -1.0])))
    assert np.array_equal(bits(out[4]), bits(np.array([1.0, 0.0, 0.0])))
    # coordinates at the bound: products of 1e36 and squares of 1e72 stay finite
    big = v * 1e18 / 4.0
    assert np.array_equal(bits(N.apply(off, entry, big, n)[[0, 2, 4]]), bits(out[[0, 2, 4]]))
    # an overflowing sum is not written either
    huge = v * 1e160
    assert np.array_equal(bits(N.apply(off, entry, huge, n)), bits(n))


def test_recomputed_normals_halve_the_stale_normals_error(pkg):
    """S-cornell-small under kit.moved_sphere's squash to 0.6 along y: the mean angle between the sphere's normals and the analytic normals of
    the ellipsoid (which moved_sphere computes).  Stale (rest-pose) normals: mean 8.32 deg, max 14.0 deg.  Restated area-weighted normals:
    mean 1.64 deg, max 8.5 deg (tessellation error: the rest pose shows 7.9 deg against its own stored normals).  The condition: the recomputed
    mean is below HALF the stale mean."""
    s = _scene(pkg, "small")
    moved = kit.moved_sphere(pkg, s)
    ni = np.unique(s.face[s.face[:, 0, 3] == SPHERE][:, :, 1])
    new = N.auto_normals(s.face, moved.vertex, s.normal, ref_vertex=s.vertex, ref_normal=s.normal)
    stale_mean, stale_max = N.mean_angle_deg(s.normal[ni], moved.normal[ni])
    new_mean, new_max = N.mean_angle_deg(new[ni], moved.normal[ni])
    print("\n[normals] angle to the analytic normal: stale mean %.2f max %.2f deg, recomputed mean %.2f max %.2f deg" % (stale_mean, stale_max, new_mean, new_max))
    assert new_mean < 0.5 * stale_mean


def test_the_fixtures_are_what_the_suite_says(pkg):
    big, small, fan = _scene(pkg, "big"), _scene(pkg, "small"), _scene(pkg, "fan")
    assert big.normal.shape[0] == 1249 and small.normal.shape[0] == 349
    off, entry = N.per_record(big.face, 1249, big.vertex, big.normal)
    assert np.diff(off.astype(np.int64)).max() == 6                          # the sphere fixtures never exceed valence 6: hence the fan
    nn = fan.normal.shape[0]
    off, entry = N.per_record(fan.face, nn, fan.vertex, fan.normal)
    count = np.diff(off.astype(np.int64))
    assert count[-1] == FAN == count.max() and (count[nn - 3 - FAN:nn - 3] == 2).all() and count[nn - 3] == 1 and count[nn - 2] == 1   # rim, zero-area, single
    assert (count == 0).sum() > 0                                            # the dropped sphere's records
    z = entry[off[nn - 3]]
    assert np.array_equal(N._cross(fan.vertex[z[0:1]], fan.vertex[z[1:2]], fan.vertex[z[2:3]]), np.zeros((1, 3)))
    v = _fan_moved(pkg)
    out = N.apply(off, entry, v, fan.normal)
    assert np.array_equal(bits(out[nn - 3]), bits(fan.normal[nn - 3])) and not np.array_equal(out[-1], fan.normal[-1]) and abs(np.linalg.norm(out[-1]) - 1) < 1e-15
    assert out[-1, 1] > 0.5 and np.array_equal(bits(out[count == 0]), bits(fan.normal[count == 0]))


def _fan_moved(pkg):
    """The fan scene with its apex pushed aside and its rim rippled; the zero-area face slides along its own line (and stays of zero area)."""
    s = _scene(pkg, "fan"); nv = s.vertex.shape[0]
    v = s.vertex.copy()
    first = nv - 7 - FAN
    rng = np.random.default_rng(8)
    v[first:first + FAN] += rng.uniform(-0.03, 0.03, (FAN, 3))
    v[first + FAN] += (0.12, 0.2, -0.07)
    v[first + FAN + 1:first + FAN + 4] += 0.125
    v[first + FAN + 4] += (0.0, 0.1, 0.0)
    return v


def _host_check_cases(pkg):
    """(face, n_normal, mask, vertex, normal) for normals_host_check: the fixtures, the fan, a masked and a moved reference pose, a random soup
    with repeated corners, zero and NaN normals, and the empty cases."""
    small, fan, big = _scene(pkg, "small"), _scene(pkg, "fan"), _scene(pkg, "big")
    cases = [(small.face, 349, None, small.vertex, small.normal), (fan.face, fan.normal.shape[0], None, fan.vertex, fan.normal),
             (big.face, 1249, _mask(pkg, big, "sphere"), big.vertex, big.normal),
             (small.face, 349, _mask(pkg, small, "sphere"), _moved(pkg, small)[0], _moved(pkg, small)[1]),
             (fan.face, fan.normal.shape[0], None, _fan_moved(pkg), fan.normal)]
    rng = np.random.default_rng(21)
    for nf, nv, nn in ((1, 3, 1), (300, 40, 7), (257, 500, 300)):
        face = np.zeros((nf, 3, 4), np.int32); face[:, :, 0] = rng.integers(0, nv, (nf, 3)); face[:, :, 1] = rng.integers(0, nn, (nf, 3))
        n = rng.normal(size=(nn, 3)); n[::5] = 0.0; n[1::7, 1] = np.nan
        cases.append((face, nn, (rng.uniform(size=nn) < 0.7).astype(np.uint8), rng.normal(size=(nv, 3)) * 10.0 ** rng.integers(-3, 4), n))
    cases.append((np.zeros((0, 3, 4), np.int32), 5, None, np.zeros((2, 3)), np.ones((5, 3))))                    # no faces
    cases.append((small.face, 349, np.zeros(349, np.uint8), small.vertex, small.normal))                         # everything masked out
    return cases


@K.needs_hipcc
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_lists_are_the_restatement_bit_for_bit(pkg, tmp_path, sanitized):
    """The host half of the feature -- nr_per_record of csrc/normals.hip -- built into the stand-alone program tests/normals_host_check.cpp (no
    device is touched) against tests/normals_ref.py: the same offsets, entries and flips.  `sanitized`: the same program under the host's
    address and undefined-behaviour sanitizers, which must stay silent."""
    exe = K.build_host_check("normals_host_check", ["normals.hip"], tmp_path, sanitized)
    cases = _host_check_cases(pkg)
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for face, nn, mask, v, n in cases:
            f.write(np.array([face.shape[0], nn, v.shape[0], mask is not None], np.uint32).tobytes())
            f.write(np.ascontiguousarray(face[:, :, 0], np.int32).tobytes()); f.write(np.ascontiguousarray(face[:, :, 1], np.int32).tobytes())
            if mask is not None:
                f.write(np.ascontiguousarray(mask, np.uint8).tobytes())
            f.write(np.ascontiguousarray(v, np.float64).tobytes()); f.write(np.ascontiguousarray(n, np.float64).tobytes())
    K.run_host_check(exe, tmp_path, sanitized)
    raw = open(str(tmp_path / "out.bin"), "rb").read()
    at = 0
    for k, (face, nn, mask, v, n) in enumerate(cases):
        off, entry = N.per_record(face, nn, v, n, mask)
        count = np.diff(off.astype(np.int64))
        for want in (off, entry.reshape(-1), np.array([count.max() if count.size else 0], np.uint32)):
            got = np.frombuffer(raw, want.dtype, want.size, at); at += want.nbytes
            assert np.array_equal(got, want), (k, nn)
    assert at == len(raw)


# ------------------------------------------------------------------------------------------------------------------------ GPU helpers
def _pair(pkg, which="big", extra=0):
    """The context under test and its oracle (which never has the feature)."""
    return K.pair(pkg, extra=extra, max_depth=8, scene=_scene(pkg, which))


def _lists(pkg, which, mask, ref=None):
    s = _scene(pkg, which)
    rv, rn = (s.vertex, s.normal) if ref is None else ref
    return N.per_record(s.face, s.normal.shape[0], rv, rn, mask)


def _check_route(pkg, R, O, which, route, mask, film=True, lists=None):
    """The route on R (auto normals on), update_vertices with the restated arrays on O: the device arrays directly, then everything downstream."""
    current = R.vertices()[1]
    v, n_route = _route(pkg, R, which, route, current)
    off, entry = _lists(pkg, which, mask) if lists is None else lists
    n = N.apply(off, entry, v, n_route)
    O.update_vertices(v, n)
    K.assert_arrays(R, v, n)
    keep = np.diff(off.astype(np.int64)) == 0
    assert np.array_equal(bits(n[keep]), bits(np.ascontiguousarray(n_route)[keep])) and not np.array_equal(n[~keep], np.asarray(n_route)[~keep])
    a, b = K.state(pkg, R, film), K.state(pkg, O, film)
    K.assert_same(a, b)
    return a, v, n


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("which_mask", ["all", "sphere"])
@pytest.mark.parametrize("route", ROUTES)
def test_every_route_is_followed_by_the_pass(pkg, route, which_mask):
    """S-cornell with the 48 x 24 sphere (1 249 records).  With the mask on the sphere only, the walls and the lamp keep bit for bit what their
    route wrote (asserted against the route's own restatement in _check_route)."""
    s = _scene(pkg); mask = _mask(pkg, s, which_mask)
    R, O = _pair(pkg)
    _prepare(pkg, R, "big", route)
    R.set_auto_normals(mask)
    K.assert_arrays(R, s.vertex, s.normal)                                   # setting it moves nothing
    rest = R.probe_lights()
    moved, v, n = _check_route(pkg, R, O, "big", route, mask)
    assert not np.array_equal(rest[2], moved["light_pos"])                   # the lamp moved (every route moves it)
    want = (v[s.face[moved["light_face"], :, 0]] - np.array(list(R.info().centre))).reshape(-1, 9)       # the nine fp64 positions per light
    assert np.array_equal(bits(want), bits(moved["light_pos"]))
    ni, ui = R.normals_info(), R.update_info()
    off, entry = _lists(pkg, "big", mask)
    assert (ni.mode, ni.updates, ni.entries, ni.records) == (pkg.NORMALS_AREA, 1, entry.shape[0], int((np.diff(off.astype(np.int64)) > 0).sum()))
    assert ui.updates == 1 and 0 < ni.last_ms <= ui.last_update_ms
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_tree", [False, True])
@pytest.mark.parametrize("which", ["small", "fan"])
def test_small_scene_and_fan_with_both_builders(pkg, which, gpu_tree):
    """S-cornell-small (349 records, two unused) and the hand-made scene (valence 70 on the LAST record, a zero-area face, a face with one
    record in all corners), each under the host and the device tree builder, through update_vertices(normal = None)."""
    s = _scene(pkg, which); nn = s.normal.shape[0]
    R, O = _pair(pkg, which, extra=pkg.FLAG_GPU_BVH_BUILD if gpu_tree else 0)
    R.set_auto_normals()
    off, entry = _lists(pkg, which, None)
    v = _moved(pkg, s)[0] if which == "small" else _fan_moved(pkg)
    n = N.apply(off, entry, v, s.normal)
    R.update_vertices(v, None); O.update_vertices(v, n)
    K.assert_arrays(R, v, n)
    K.assert_same(K.state(pkg, R), K.state(pkg, O))
    ni = R.normals_info()
    count = np.diff(off.astype(np.int64))
    assert (ni.records, ni.entries, ni.max_valence) == (int((count > 0).sum()), entry.shape[0], int(count.max()))
    if which == "small":
        assert (ni.records, ni.entries, ni.max_valence) == (347, 1620, 6)
    else:
        assert ni.max_valence == FAN and np.array_equal(bits(n[nn - 3]), bits(s.normal[nn - 3])) and not np.array_equal(n[-1], s.normal[-1])
    R.close(); O.close()


@pytest.mark.gpu
def test_update_normals_alone_and_sequences(pkg):
    s = _scene(pkg); nn = s.normal.shape[0]
    R, O = _pair(pkg)
    plain = K.state(pkg, R, film=False)
    base = R.info().device_bytes
    R.set_auto_normals()
    off, entry = _lists(pkg, "big", None)
    assert R.info().device_bytes - base == 4 * (nn + 1) + 16 * entry.shape[0] and entry.shape[0] <= 3 * s.face.shape[0]
    # update_normals on a context at rest: the restated normals of the rest pose, no vertex moves; twice = once
    n0 = N.apply(off, entry, s.vertex, s.normal)
    R.update_normals(); O.update_vertices(s.vertex, n0)
    K.assert_arrays(R, s.vertex, n0)
    once = K.state(pkg, R)
    K.assert_same(once, K.state(pkg, O))
    assert not np.array_equal(bits(once["shade"]), bits(plain["shade"]))     # (the stored normals are rounded to 9 digits: the pass differs in the last bits)
    R.update_normals()
    K.assert_arrays(R, s.vertex, n0)
    K.assert_same(K.state(pkg, R), once)
    assert (R.update_info().updates, R.normals_info().updates) == (2, 2)
    # M1 then M2 = M2 alone (the pass reads the current vertices only)
    v1, _ = _moved(pkg, s, step=2); v2, _ = _moved(pkg, s)
    R.update_vertices(v1, None)
    K.assert_arrays(R, v1, N.apply(off, entry, v1, n0))
    R.update_vertices(v2, None)
    n2 = N.apply(off, entry, v2, n0)
    O.update_vertices(v2, n2)
    K.assert_arrays(R, v2, n2)
    K.assert_same(K.state(pkg, R), K.state(pkg, O))
    # a second set_auto_normals takes its reference pose from the MOVED scene, and may change the mask
    mask = _mask(pkg, s, "sphere")
    R.set_auto_normals(mask)
    lists2 = _lists(pkg, "big", mask, ref=(v2, n2))
    assert R.normals_info().entries == lists2[1].shape[0] < entry.shape[0]
    _check_route(pkg, R, O, "big", "vertices_with_normals", mask, film=False, lists=lists2)
    # after OFF a route gives what a context that never had the feature gives, and device_bytes is back
    R.set_auto_normals(mode=pkg.NORMALS_OFF)
    ni = R.normals_info()
    assert (ni.mode, ni.records, ni.entries, ni.max_valence) == (pkg.NORMALS_OFF, 0, 0, 0)
    passes = ni.updates
    v, n = _moved(pkg, s, step=2)
    for r in (R, O):
        r.update_vertices(v, n); r.update_vertices(v2, None)
    K.assert_arrays(R, v2, n)
    K.assert_same(K.state(pkg, R), K.state(pkg, O))
    assert R.normals_info().updates == passes and R.info().device_bytes == O.info().device_bytes
    with pytest.raises(pkg.McptError) as e:
        R.update_normals()
    assert "status %d" % INVALID in str(e.value)
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["own", "side"])
def test_update_between_renders_without_a_sync(pkg, which):
    import torch
    s = _scene(pkg)
    R, O = _pair(pkg)
    R.set_auto_normals()
    off, entry = _lists(pkg, "big", None)
    v1, _ = _moved(pkg, s, step=2); v2, _ = _moved(pkg, s)
    n1 = N.apply(off, entry, v1, s.normal); n2 = N.apply(off, entry, v2, n1)
    if which == "side":
        stream = torch.cuda.Stream()
        R.set_torch_stream(stream)
    R.clear()
    R.render(4, seed=9, first_sample=0); R.update_vertices(v1, None); R.render(4, seed=9, first_sample=4)   # nothing in between
    R.update_vertices(v2, None); R.update_normals()                                                       # back-to-back updates keep their order
    R.render(2, seed=9, first_sample=8)
    got = R.read_accum()
    O.clear()
    O.render(4, seed=9, first_sample=0); O.sync(); O.update_vertices(v1, n1); O.sync(); O.render(4, seed=9, first_sample=4); O.sync()
    O.update_vertices(v2, n2); O.sync(); O.render(2, seed=9, first_sample=8); O.sync()
    assert np.array_equal(bits(got), bits(O.read_accum())) and np.all(got[..., 3] == 10)
    K.assert_arrays(R, v2, n2)
    if which == "side":
        R.set_stream(0)
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["vertices", "skin"])
@pytest.mark.parametrize("with_camera", [False, True])
def test_reprojection_follows_the_recomputed_normals(pkg, with_camera, route):
    s = _scene(pkg)
    R, O = _pair(pkg)
    _prepare(pkg, R, "big", route)
    R.set_auto_normals()
    cam = pkg.scenes.Camera((0.62, 0.55, 2.25), (0.5, 0.45, 0.0), (0.0, 1.0, 0.0), 40.0, W, H) if with_camera else None
    opts = dict(feature_spp=4, feature_seed=3, max_history=16.0)
    for r in (R, O):
        r.clear(); r.render(8, seed=5)
    v, n_route = _route(pkg, R, "big", route, s.normal, reproject=dict(camera=cam, **opts))
    n = N.apply(*_lists(pkg, "big", None), v, n_route)
    O.update_vertices_reproject(v, n, camera=cam, **opts)
    assert np.array_equal(bits(R.read_accum()), bits(O.read_accum()))
    ia, ib = R.reproject_info(), O.reproject_info()
    assert (ia.reprojections, ia.pixels_reused) == (ib.reprojections, ib.pixels_reused) == (1, ib.pixels_reused) and ia.pixels_reused > 0.5 * W * H
    assert np.array_equal(bits(R.features()), bits(O.features()))          # the context holds the new scene's features
    assert R.update_info().updates == 1 and R.normals_info().updates == 1
    K.assert_arrays(R, v, n)
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    R.close(); O.close()


@pytest.mark.gpu
def test_clone_rebuild_and_bookkeeping(pkg):
    s = _scene(pkg); nn = s.normal.shape[0]
    mask = _mask(pkg, s, "sphere")
    R, O = _pair(pkg)
    base = R.info().device_bytes
    ni = R.normals_info()
    assert (ni.struct_size, ni.mode, ni.records, ni.entries, ni.max_valence, ni.updates, ni.last_ms) == (56, 0, 0, 0, 0, 0, 0.0)
    off, entry = _lists(pkg, "big", mask); off_all, entry_all = _lists(pkg, "big", None)
    R.set_auto_normals(mask)
    assert R.info().device_bytes - base == 4 * (nn + 1) + 16 * entry.shape[0]
    R.set_auto_normals()                                                     # replaces: the old lists are released
    assert R.info().device_bytes - base == 4 * (nn + 1) + 16 * entry_all.shape[0] and R.normals_info().max_valence == 6
    R.set_auto_normals(mask)
    assert R.info().device_bytes - base == 4 * (nn + 1) + 16 * entry.shape[0]
    _, v1, n1 = _check_route(pkg, R, O, "big", "vertices", mask, film=False)
    clone = R.clone(); bare = O.clone()
    assert clone.info().device_bytes == bare.info().device_bytes + 4 * (nn + 1) + 16 * entry.shape[0]       # (fresh clones hold no render pools)
    bare.close()
    ci = clone.normals_info()
    assert (ci.mode, ci.records, ci.entries, ci.max_valence, ci.updates) == (pkg.NORMALS_AREA, int(mask.sum()), entry.shape[0], 6, 0)
    K.assert_arrays(clone, v1, n1)                                           # the clone is the moved scene ...
    v2, _ = _moved(pkg, s, step=2)
    n2 = N.apply(off, entry, v2, n1)
    clone.update_vertices(v2, None); O.update_vertices(v2, n2)               # ... with the lists (taken at the ORIGINAL reference pose)
    K.assert_arrays(clone, v2, n2)
    K.assert_same(K.state(pkg, clone), K.state(pkg, O))
    K.assert_arrays(R, v1, n1)                                               # the source did not move with its clone
    # a rebuild with either builder keeps the lists: they follow the description's face order, not the leaf order
    for k, builder in enumerate((pkg.REBUILD_HOST, pkg.REBUILD_DEVICE)):
        R.rebuild(builder); O.rebuild(builder)
        assert R.normals_info().entries == entry.shape[0]
        v = v2 if k == 0 else v1
        n = N.apply(off, entry, v, R.vertices()[1])
        R.update_vertices(v, None); O.update_vertices(v, n)
        K.assert_arrays(R, v, n)
        K.assert_same(K.state(pkg, R, film=k == 1), K.state(pkg, O, film=k == 1))
    assert R.info().device_bytes == O.info().device_bytes + 4 * (nn + 1) + 16 * entry.shape[0]
    assert (R.normals_info().updates, R.update_info().updates, clone.normals_info().updates) == (3, 3, 1)
    clone.close(); R.close(); O.close()


@pytest.mark.gpu
def test_normals_refusals(pkg):
    s = _scene(pkg, "small"); nn = s.normal.shape[0]
    plain = pkg.Renderer(s, max_depth=8, flags=pkg.FLAG_DETERMINISTIC)
    for call in (lambda: plain.set_auto_normals(), lambda: plain.set_auto_normals(mode=pkg.NORMALS_OFF), lambda: plain.update_normals()):
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % UNSUPPORTED in str(e.value)
    assert plain.normals_info().mode == pkg.NORMALS_OFF                      # the info call works on every context
    plain.close()
    R = pkg.Renderer(s, max_depth=8, flags=FLAGS(pkg))
    o, d = K.rays(pkg)
    film = render_film(R, 4, 5); trace = R.probe_trace4(o, d); arrays = R.vertices(); bytes0 = [R.info().device_bytes]
    expect = {"mode": 0, "records": 0, "entries": 0, "max_valence": 0}

    def unchanged():
        ni = R.normals_info()
        assert R.update_info().updates == 0 and (ni.updates, ni.last_ms) == (0, 0.0)
        assert {k: getattr(ni, k) for k in expect} == expect
        assert R.info().device_bytes == bytes0[0]
        assert np.array_equal(bits(render_film(R, 4, 5)), bits(film))
        for x, y in zip(trace, R.probe_trace4(o, d)):
            assert np.array_equal(bits(x), bits(y))
        for x, y in zip(arrays, R.vertices()):
            assert np.array_equal(bits(x), bits(y))

    lib = R.lib
    good = pkg.NormalsOpts(); good.struct_size = C.sizeof(pkg.NormalsOpts); good.mode = pkg.NORMALS_AREA
    mask = np.ones(nn, np.uint8); mp = mask.ctypes.data_as(C.c_void_p)

    def bad_opts(**fields):
        b = pkg.NormalsOpts(); b.struct_size = C.sizeof(pkg.NormalsOpts); b.mode = pkg.NORMALS_AREA
        for k, x in fields.items():
            setattr(b, k, x)
        return b

    def all_refusals():
        assert lib.mcpt_update_normals(R.ctx) == INVALID                    # (only called while auto normals are not set)
        for n_normal in (nn - 1, nn + 1, 0):                                 # a wrong n_normal, with and without a mask
            assert lib.mcpt_set_auto_normals(R.ctx, mp, n_normal, C.byref(good)) == INVALID and lib.mcpt_set_auto_normals(R.ctx, None, n_normal, None) == INVALID
        for b in (bad_opts(struct_size=0), bad_opts(struct_size=C.sizeof(pkg.NormalsOpts) - 4), bad_opts(struct_size=C.sizeof(pkg.NormalsOpts) + 4),
                  bad_opts(mode=2), bad_opts(mode=0xFFFFFFFF)):              # a wrong struct_size, an unknown mode
            assert lib.mcpt_set_auto_normals(R.ctx, mp, nn, C.byref(b)) == INVALID
        assert lib.mcpt_get_normals_info(R.ctx, None) == INVALID
        unchanged()

    with pytest.raises(pkg.McptError) as e:
        R.update_normals()                                                   # auto normals are not set
    assert "status %d" % INVALID in str(e.value) and "not set" in str(e.value)
    all_refusals()
    R.set_auto_normals(_mask(pkg, s, "sphere"))                              # accepted; a refused replacement leaves the lists that are set
    off, entry = _lists(pkg, "small", _mask(pkg, s, "sphere"))
    expect.update(mode=1, records=323, entries=entry.shape[0], max_valence=6)
    bytes0[0] += 4 * (nn + 1) + 16 * entry.shape[0]
    for n_normal in (nn - 1, nn + 1):
        assert lib.mcpt_set_auto_normals(R.ctx, mp, n_normal, C.byref(good)) == INVALID
    for b in (bad_opts(struct_size=0), bad_opts(mode=2)):
        assert lib.mcpt_set_auto_normals(R.ctx, mp, nn, C.byref(b)) == INVALID
    unchanged()
    R.validate_trees()
    assert lib.mcpt_set_auto_normals(R.ctx, None, nn, None) == 0             # NULL mask and NULL options: all records, area weighting
    assert (R.normals_info().mode, R.normals_info().records) == (1, 347)
    R.update_normals()                                                       # and the context still works
    assert R.update_info().updates == 1 and R.normals_info().updates == 1
    R.validate_trees()
    R.close()


@pytest.mark.gpu
def test_facade_normals(pkg, tmp_path):
    exe = kit.build_facade("facade_normals.cpp", tmp_path)
    a = pkg.scenes.cornell_box(44, 30, sphere_lon=24, sphere_lat=12)
    obj = a.write(str(tmp_path / "a"))
    # the program reads the 9-digit text of the file: the same numbers scenes.py keeps (SceneData is rounded through that text form)
    part = a.face[:, 0, 3] == SPHERE
    mask = pkg.normal_mask_from_faces(a, part)
    off, entry = N.per_record(a.face, a.normal.shape[0], a.vertex, a.normal, mask)
    v1, _ = _moved(pkg, a)
    n1 = N.apply(off, entry, v1, a.normal); n0 = N.apply(off, entry, a.vertex, a.normal)
    part.astype(np.uint8).tofile(str(tmp_path / "fm.bin"))
    for arr, name in ((v1, "v1"), (n1, "n1"), (n0, "n0")):
        arr.tofile(str(tmp_path / (name + ".bin")))
    ins = [str(tmp_path / (n + ".bin")) for n in ("fm", "v1", "n1", "n0")]
    outs = [str(tmp_path / n) for n in ("auto.bin", "upd.bin", "auto0.bin", "upd0.bin")]
    k = 4
    line = kit.run_facade(exe, [obj, str(k)] + ins + outs)
    w_, h_ = int(line[0]), int(line[1])
    assert (w_, h_, int(line[2]), int(line[3]), int(line[4])) == (44, 30, k, int(mask.sum()), 3)
    auto, upd, auto0, upd0 = [np.fromfile(p, np.float32).reshape(h_, w_, 4) for p in outs]
    assert np.all(auto[..., 3] == k) and auto[..., :3].sum() > 0             # the picture started again and ends at k samples
    assert np.array_equal(bits(auto), bits(upd))                           # stale normals + the pass = the restated normals through update()
    assert np.array_equal(bits(auto0), bits(upd0)) and not np.array_equal(auto0, auto)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["wobble", "swell", "reproject"])
def test_cli_auto_normals(pkg, tmp_path, mode):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    out = str(tmp_path / "img")
    base = [obj, "--turntable", "3", "--spp", "4", "--depth", "5", "--out", out]
    move = {"wobble": ["--wobble", "0.05"], "swell": ["--swell", "glossy", "0.2"], "reproject": ["--wobble", "0.05", "--reproject", "8"]}[mode]
    p = kit.run_cli(base + move + ["--deterministic"])
    assert p.returncode == 0, p.stderr[-2000:]
    without = kit.turntable_frames(out)
    p = kit.run_cli(base + move + ["--deterministic", "--auto-normals"])
    assert p.returncode == 0, p.stderr[-2000:]
    imgs = kit.turntable_frames(out)
    assert imgs[0] != imgs[1] and imgs[1] != imgs[2]
    if mode != "swell":                                                      # (--swell scales uniformly: its normals stay, up to the last bits)
        assert imgs[1] != without[1]                                         # the recomputed normals shade the wobbled frames differently
    if mode == "wobble":                                                     # clean errors, and the rebuild threshold is honoured
        q = kit.run_cli([obj, "--wobble", "0.05", "--auto-normals"])
        assert q.returncode == 2 and "--turntable" in q.stderr
        for other in ([], ["--spin", "glossy"], ["--light-pulse", "0.2"]):
            q = kit.run_cli(base + other + ["--auto-normals"])
            assert q.returncode == 2 and "--auto-normals" in q.stderr
        q = kit.run_cli(base + move + ["--auto-normals", "--rebuild-above", "1.0"])
        assert q.returncode == 0 and "rebuild: frame" in q.stdout, q.stderr[-2000:]
    if mode == "swell":
        q = kit.run_cli(base + move + ["--bend", "glossy", "25", "--auto-normals", "--reproject", "8"])
        assert q.returncode == 0, q.stderr[-2000:]


@pytest.mark.gpu
def test_auto_normals_update_is_not_slower_on_the_device_than_the_upload_it_replaces(pkg):
    """S-bath detail 160 (0.59 M triangles), the fixtures swollen and lifted, every normal record recomputed: device time
    (mcpt_update_info::last_update_ms, HIP events: everything from the first copy to the end of the refit) of mcpt_update_vertices(normal = NULL)
    with auto normals on against mcpt_update_vertices fed the identical vertices plus the restated normals with auto normals off, on the same
    context, alternating, medians of 20 after 3 warm-ups.  The one claim: the new route's device time is not larger.  The figures are in
    DESIGN.md §20 and profiles/normals_probe.json (tools/normals_probe.py): 0.549 ms against 0.650 ms."""
    scene = pkg.scenes.bathroom_stress(64, 36, detail=160, tex_size=16)
    part = np.isin(scene.face[:, 0, 3], (5, 6))
    vi = np.unique(scene.face[part][:, :, 0])
    p = scene.vertex[vi]; c = p.mean(0)
    y = (p[:, 1] - p[:, 1].min()) / (p[:, 1].max() - p[:, 1].min())
    off, entry = N.per_record(scene.face, scene.normal.shape[0], scene.vertex, scene.normal)
    vs, ns = [], []
    for swell, lift in ((0.05, 0.5), (-0.04, 1.0)):
        v = scene.vertex.copy()
        v[vi] = p + swell * (p - c) + lift * np.stack([0.05 * y, 0.1 * y * y, np.zeros_like(y)], 1)
        vs.append(v); ns.append(N.apply(off, entry, v, scene.normal))
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    auto, up = [], []
    for i in range(23):
        v, n = vs[i % 2], ns[i % 2]
        R.set_auto_normals()
        R.update_vertices(v, None); auto.append(R.update_info().last_update_ms)
        if i == 0:                                                           # (the lists were taken at the rest pose: the restatement's)
            K.assert_arrays(R, v, n)
        R.set_auto_normals(mode=pkg.NORMALS_OFF)
        R.update_vertices(v, n); up.append(R.update_info().last_update_ms)
    R.validate_trees()
    R.close()
    a, b = float(np.median(auto[3:])), float(np.median(up[3:]))
    print("\n[normals] %d vertices, %d normals, %d entries: update_vertices(normal = NULL) + pass %.3f ms, update_vertices with normals %.3f ms on the device "
          "(medians of 20), ratio %.3f" % (scene.vertex.shape[0], scene.normal.shape[0], entry.shape[0], a, b, a / b))
    assert 0 < a <= b
