"""Every route of a live-scene update on ONE context that has groups, a skin, a morph and a mask of auto normals all set (DESIGN.md §12, §14, §16,
§18 - §21): the caller's arrays, the groups' matrices, the bones in both skinning modes, the morph weights alone and in front of the bones in both
modes, and the normals pass alone -- each in its plain form and, where there is one, its _reproject form, with auto normals off and on.

The per-feature suites hold every route's numbers to a restatement; this one pins what each of them sees only a slice of: which counters a route
advances, that the plain and the _reproject form of a route write the same arrays (a clone included), and which refusal wins when several apply.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from tests import skin_ref as S, transform_ref as T
from tests.kit import bits

W, H = 8, 6                                                                  # a film of a few pixels: the routes are under test, not the picture
SPHERE = 4                                                                   # material of S-cornell's glossy sphere
CENTRE = np.array([0.5, 0.3, 0.5])                                           # of the sphere
INVALID = 1
N_GROUPS, N_BONES, N_TARGETS = 2, 3, 2
ROUTES = ["arrays", "groups", "skin/linear", "skin/dq", "morph", "morph+bones/linear", "morph+bones/dq", "normals"]
# per route the increments of (update, transform, skin, morph); normals and reprojections follow from auto normals and the form
INCREMENTS = {"arrays": (1, 0, 0, 0), "groups": (1, 1, 0, 0), "skin": (1, 0, 1, 0), "morph": (1, 0, 0, 1), "morph+bones": (1, 0, 1, 1), "normals": (1, 0, 0, 0)}
ENTRY = {"arrays": "mcpt_update_vertices_reproject", "groups": "mcpt_update_transforms_reproject", "skin": "mcpt_update_skin_reproject",
         "morph": "mcpt_update_morph_reproject", "morph+bones": "mcpt_update_morph_reproject"}
BAD_SOURCE = {"arrays": "n_vertex differs from the scene's", "groups": "n_groups differs from the groups set", "skin": "n_bones differs from the skin set",
              "morph": "n_targets differs from the morph set", "morph+bones": "n_bones differs from the skin set"}
BAD_CAMERA = "width / height differ from the context's film"
BAD_OPTS = "opts->struct_size != sizeof(mcpt_reproject_opts)"
NO_NORMALS = "mcpt_update_normals: auto normals are not set (mcpt_set_auto_normals)"


@functools.lru_cache(maxsize=None)
def _fixture(pkg):
    """The smallest dynamic fixture of the skin and morph suites (S-cornell with a 24 x 12 sphere) and what the four set calls take: the sphere
    as group 1, three bones (the sphere blended between 1 and 2 by height), two targets (a swell of the sphere, every 5th of its vertices
    nudged; the normals' targets random), the sphere's normal records as the mask."""
    s = pkg.scenes.cornell_box(W, H, sphere_lon=24, sphere_lat=12)
    part = s.face[:, 0, 3] == SPHERE
    vi = np.unique(s.face[part][:, :, 0]); ni = np.unique(s.face[part][:, :, 1])
    y = s.vertex[vi, 1]; w = (y - y.min()) / (y.max() - y.min())
    vb, vw = S.single(np.zeros(s.vertex.shape[0], int))
    vb[vi, 0] = 1; vb[vi, 1] = 2; vw[vi, 0] = 1.0 - w; vw[vi, 1] = w
    rng = np.random.default_rng(17)
    vt = [(vi, s.vertex[vi] - CENTRE), (vi[::5], rng.uniform(-0.02, 0.02, (len(vi[::5]), 3)))]
    nt = [(ni, rng.uniform(-0.3, 0.3, (len(ni), 3))), (ni[::5], rng.uniform(-0.3, 0.3, (len(ni[::5]), 3)))]
    return {"scene": s, "sphere": vi, "groups": pkg.groups_from_faces(s, part.astype(int)), "skin": (vb, vw) + tuple(pkg.skin_normals_from_faces(s, vb, vw)),
            "targets": (vt, nt), "mask": pkg.normal_mask_from_faces(s, part)}


def _context(pkg, auto):
    fx = _fixture(pkg)
    r = pkg.Renderer(fx["scene"], max_depth=4, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_DETERMINISTIC)
    r.set_vertex_groups(*fx["groups"], N_GROUPS); r.set_vertex_skin(*fx["skin"], N_BONES); r.set_vertex_morph(*fx["targets"])
    if auto:
        r.set_auto_normals(fx["mask"])
    return r


def _turn(k, lift):
    """A rigid matrix (both skinning modes take it) that differs from step to step."""
    return T.about(T.rotation((0, 1, 0), 7.0 + 4.0 * k), CENTRE, (0.0, lift, 0.0)) + 0.0


def _call(pkg, r, route, k, reproject=False):
    """One call of `route` on `r` with the values of step k, in its plain or its _reproject form."""
    fx = _fixture(pkg); s = fx["scene"]
    kind, _, mode = route.partition("/")
    form = "_reproject" if reproject else ""
    if mode:
        r.set_skin_mode(pkg.SKIN_DUAL_QUATERNION if mode == "dq" else pkg.SKIN_LINEAR)
    bones = np.stack([T.identity(1)[0], _turn(k, 0.02), _turn(k + 1, 0.03)])
    weights = np.array([0.1 + 0.05 * k, -0.4])
    if kind == "arrays":
        v = s.vertex.copy(); v[fx["sphere"]] += (0.01 * (k + 1), 0.02, -0.01)
        getattr(r, "update_vertices" + form)(v, s.normal)
    elif kind == "groups":
        getattr(r, "update_transforms" + form)(np.stack([T.identity(1)[0], _turn(k, 0.04)]))
    elif kind == "skin":
        getattr(r, "update_skin" + form)(bones)
    elif kind in ("morph", "morph+bones"):
        getattr(r, "update_morph" + form)(weights, bones if kind == "morph+bones" else None)
    else:
        assert kind == "normals" and not reproject                              # the one route without a _reproject form
        r.update_normals()


def _counters(r):
    return (r.update_info().updates, r.transform_info().updates, r.skin_info().updates, r.morph_info().updates, r.normals_info().updates,
            r.reproject_info().reprojections)


@pytest.mark.gpu
@pytest.mark.parametrize("auto", [False, True])
def test_counter_increments_per_route(pkg, auto):
    r = _context(pkg, auto)
    assert _counters(r) == (0, 0, 0, 0, 0, 0)
    k = 0
    for route in ROUTES:
        kind = route.partition("/")[0]
        for reproject in ((False,) if kind == "normals" else (False, True)):
            before = _counters(r)
            if kind == "normals" and not auto:                               # nothing to run: refused, and nothing counts
                with pytest.raises(pkg.McptError) as e:
                    _call(pkg, r, route, k)
                assert "status %d: %s" % (INVALID, NO_NORMALS) in str(e.value)
                want = (0, 0, 0, 0, 0, 0)
            else:
                _call(pkg, r, route, k, reproject)
                want = INCREMENTS[kind] + (1 if kind == "normals" else int(auto), int(reproject))
            got = tuple(a - b for a, b in zip(_counters(r), before))
            print(route, "reproject" if reproject else "plain", "auto" if auto else "off", got)
            assert got == want, (route, reproject)
            k += 1
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("auto", [False, True])
def test_plain_and_reproject_forms_write_the_same_arrays(pkg, auto):
    r = _context(pkg, auto)
    clone = r.clone(0)                                                       # taken beforehand; the same device: the machine's count is not assumed
    last = r.vertices()
    for k, route in enumerate(ROUTES):
        kind = route.partition("/")[0]
        if kind == "normals" and not auto:
            continue
        _call(pkg, r, route, k)
        plain = r.vertices()
        if kind != "normals":
            assert not np.array_equal(plain[0], last[0]), route              # the step moved the scene: an equal result below is not a stale one
            _call(pkg, r, route, k, reproject=True)
        _call(pkg, clone, route, k, reproject=kind != "normals")              # the clone sees the values of this step in this form only
        for what, other in (("reproject", r.vertices()), ("clone", clone.vertices())):
            for a, b, name in zip(plain, other, ("vertex", "normal")):
                assert np.array_equal(bits(a), bits(b)), (route, what, name)
        last = plain
    clone.close(); r.close()


def _raw_reproject(pkg, r, kind, good_source, camera, opts):
    """The _reproject entry point of `kind` through the C ABI (the wrappers cannot spoil the options' struct_size): (status, message)."""
    s = _fixture(pkg)["scene"]; p = pkg._ptr
    tail = (C.byref(pkg._camera_c(camera)), C.byref(opts))
    off = 0 if good_source else 1
    w = np.zeros(N_TARGETS + (off if kind == "morph" else 0)); m = T.identity((N_GROUPS if kind == "groups" else N_BONES) + off)
    if kind == "arrays":
        v = np.ascontiguousarray(s.vertex[:s.vertex.shape[0] - off])
        st = r.lib.mcpt_update_vertices_reproject(r.ctx, p(v), v.shape[0], None, 0, *tail)
    elif kind == "groups":
        st = r.lib.mcpt_update_transforms_reproject(r.ctx, p(m), m.shape[0], *tail)
    elif kind == "skin":
        st = r.lib.mcpt_update_skin_reproject(r.ctx, p(m), m.shape[0], *tail)
    else:
        bones = kind == "morph+bones"
        st = r.lib.mcpt_update_morph_reproject(r.ctx, p(w), w.shape[0], p(m) if bones else None, m.shape[0] if bones else 0, *tail)
    return st, (r.lib.mcpt_last_error() or b"").decode()


@pytest.mark.gpu
def test_error_precedence_of_the_reproject_forms(pkg):
    """The source's refusal comes before the camera's, the camera's before the options'; a refused call counts nothing and allocates nothing."""
    s = _fixture(pkg)["scene"]
    r = _context(pkg, auto=True)
    cam = s.camera
    bad_cam = pkg.scenes.Camera(cam.eye, cam.lookat, cam.up, cam.fovy, W + 1, H)
    good = pkg._reproject_opts()
    bad = pkg._reproject_opts(); bad.struct_size = C.sizeof(pkg.ReprojectOpts) - 4
    before = _counters(r); base = r.info().device_bytes
    for kind, fn in ENTRY.items():
        assert _raw_reproject(pkg, r, kind, False, bad_cam, good) == (INVALID, "%s: %s" % (fn, BAD_SOURCE[kind])), kind
        assert _raw_reproject(pkg, r, kind, True, bad_cam, bad) == (INVALID, "%s: %s" % (fn, BAD_CAMERA)), kind
        assert _raw_reproject(pkg, r, kind, True, cam, bad) == (INVALID, "%s: %s" % (fn, BAD_OPTS)), kind
    assert _counters(r) == before
    assert r.info().device_bytes == base                                     # morph with bones: no scratch for a call that is refused
    assert _raw_reproject(pkg, r, "morph+bones", True, cam, good)[0] == 0    # (a success leaves the last message as it was)
    # the first call that is not refused brings the scratch of "morph, then skin" (the arrays' size) and the reprojection's buffers: old and new
    # features (2 float4 per pixel each), the old film and the first hits (1 each), the arrays as they were
    nv, nn = s.vertex.shape[0], s.normal.shape[0]
    assert r.info().device_bytes - base == 2 * 24 * (nv + nn) + 6 * 16 * W * H
    assert tuple(a - b for a, b in zip(_counters(r), before)) == (1, 0, 1, 1, 1, 1)
    r.close()
