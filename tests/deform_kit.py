"""The one copy of what the live-scene deformer suites share (test_transforms, test_skin, test_skin_dq, test_morph, test_normals, and the layout
test of test_rebuild): S-cornell with its 48 x 24 sphere and the masks, skins and bone matrices built on it, the probe rays, `state` --
EVERYTHING the bit-for-bit comparisons look at, the same contract for every deformer -- and its comparisons, the pair of contexts (the one
under test and its oracle), the header-layout check and the stand-alone host-check harness.

A plain module, imported like tests/kit.py, and held to its rule: where the suites' copies differed in a default or an argument the function
here takes the argument explicitly and every call site passes the value it always used.  A fixture that only looks alike (the three suites'
morph targets, the two four-influence skins, the rigid bones of the dual-quaternion suite) stays in its suite.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import skin_ref as S, transform_ref as T
from tests.kit import CSRC, ROOT, bits, render_film

INVALID, UNSUPPORTED = 1, 6                                                  # mcpt_status
W, H = 64, 64
SPHERE, LAMP = 4, 3                                                          # materials of S-cornell: the glossy sphere, the ceiling light
CENTRE = np.array([0.5, 0.3, 0.5])                                           # of the sphere (radius 0.3: it stands on the floor)
N_BONES = 5                                                                  # 0 the walls, 1 and 2 the sphere's lower and upper bone, 3 nobody, 4 the lamp
FLAGS = lambda pkg: pkg.FLAG_DYNAMIC | pkg.FLAG_DETERMINISTIC
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")    # on the tests that build a host check


def clean(m):
    """The matrices without negative zeros (-0.0 + 0.0 = +0.0; everything else is unchanged)."""
    return np.ascontiguousarray(m, np.float64) + 0.0


M_LOW = clean(T.about(T.rotation((0, 0, 1), -6.0), CENTRE, (0.0, 0.06, 0.0)))
M_HIGH = clean(T.about(T.rotation((0, 0, 1), 25.0) @ np.diag([0.9, 0.95, 0.9]), (0.5, 0.1, 0.5), (0.03, 0.08, -0.04)))
M_LAMP = clean(T.about(T.rotation((0, 1, 0), 25.0), (0.5, 0.999, 0.5), (0.1, -0.2, 0.05)))


# ------------------------------------------------------------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def scene(pkg, small=False):
    """S-cornell with the 48 x 24 sphere (1 249 vertices and normals: five 256-blocks with a tail) or S-cornell-small (349 records: two blocks
    with a tail, two of the records unused)."""
    return pkg.scenes.cornell_box_small(W, H) if small else pkg.scenes.cornell_box(W, H, sphere_lon=48, sphere_lat=24)


_cornell = scene                                                             # (for pair, whose `scene` argument hides the function)


@functools.lru_cache(maxsize=None)
def parts(pkg, small=False):
    """(sphere, lamp) as boolean masks over the vertices."""
    s = scene(pkg, small)
    out = []
    for mtl in (SPHERE, LAMP):
        mask = np.zeros(s.vertex.shape[0], bool); mask[np.unique(s.face[s.face[:, 0, 3] == mtl][:, :, 0])] = True
        out.append(mask)
    return out


@functools.lru_cache(maxsize=None)
def bend(pkg, small=False):
    """The five-bone skin: walls on bone 0, lamp on bone 4, every sphere vertex blended between bones 1 and 2 by its height;
    bone 3 has no member.  (vertex ids, vertex weights, normal ids, normal weights.)"""
    s = scene(pkg, small); sphere, lamp = parts(pkg, small)
    vb, vw = S.single(np.where(lamp, 4, 0))
    y = s.vertex[sphere, 1]; w = (y - y.min()) / (y.max() - y.min())
    assert w.min() == 0.0 and w.max() == 1.0
    vb[sphere, 0] = 1; vb[sphere, 1] = 2; vw[sphere, 0] = 1.0 - w; vw[sphere, 1] = w
    return (vb, vw) + tuple(pkg.skin_normals_from_faces(s, vb, vw))


def height_skin(pkg, scene, part):
    """Three bones: the vertices of the faces in `part` blended between bones 1 and 2 by their height inside the part's y-extent, the rest bone 0."""
    vi = np.unique(scene.face[part][:, :, 0])
    y = scene.vertex[vi, 1]; w = (y - y.min()) / (y.max() - y.min())
    vb, vw = S.single(np.zeros(scene.vertex.shape[0], int))
    vb[vi, 0] = 1; vb[vi, 1] = 2; vw[vi, 0] = 1.0 - w; vw[vi, 1] = w
    nb, nw = pkg.skin_normals_from_faces(scene, vb, vw)
    return vb, vw, nb, nw


def mats(low=None, high=None, lamp=None, third=None, n=N_BONES):
    """`n` bone matrices: the identity but for the sphere's lower and upper bone, the lamp's, and bone 3 (which has no member)."""
    m = T.identity(n)
    if third is not None: m[3] = third
    if low is not None: m[1] = low
    if high is not None: m[2] = high
    if lamp is not None: m[4] = lamp
    return m


def unit_rest(pkg, group=None, n_groups=1, positive_zero=False):
    """S-cornell's vertices and its normals NORMALISED by the restatement (as members of `group` under `n_groups` identity matrices; None: all of
    group 0).  The file's normals are 9-digit decimals, unit length within ~1e-9 only: the kernels' c / |c| moves 16 of the 1 249 to another
    fp32 number, so an identity on the raw scene cannot leave the shading streams bit for bit as they were.  Normalised once they are a fixed
    point of that step in fp32 (each suite asserts it in a restatement test): a context put on this pose first (update_vertices) must come back
    to it bit for bit under an identity.  `positive_zero`: without negative zeros, for a deformer that turns -0.0 into +0.0."""
    s = scene(pkg)
    n = T.transform_normals(s.normal, np.zeros(s.normal.shape[0], int) if group is None else group, T.identity(n_groups))
    return s.vertex, n + 0.0 if positive_zero else n


@functools.lru_cache(maxsize=None)
def rays(pkg):
    """Rays from S-cornell's eye towards fixed points of the back wall's plane (one per pixel) and random rays through its box: computed once,
    never changed.  (origins, directions.)"""
    ex = np.array(scene(pkg).camera.eye); rng = np.random.default_rng(3)
    t = rng.uniform(0.0, 1.0, (W * H, 3)); t[:, 2] = 0.0                     # towards points of the back wall's plane: all through the room
    d = t - ex; d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = rng.uniform(0.01, 0.99, (3000, 3)); q = rng.uniform(0.01, 0.99, (3000, 3))
    e = q - o; e /= np.linalg.norm(e, axis=1, keepdims=True)
    return np.concatenate([np.broadcast_to(ex, d.shape), o]), np.concatenate([d, e])


def pair(pkg, setup=None, extra=0, max_depth=6, scene=None):
    """The context under test -- `setup(R)` puts the deformer on it -- and its oracle, which never has the feature: (R, O)."""
    s = _cornell(pkg) if scene is None else scene
    R = pkg.Renderer(s, max_depth=max_depth, flags=FLAGS(pkg) | extra); O = pkg.Renderer(s, max_depth=max_depth, flags=FLAGS(pkg) | extra)
    if setup is not None:
        setup(R)
    return R, O


# ------------------------------------------------------------------------------------------------------------------------ comparisons
def state(pkg, r, film=True, arrays=False):
    """Everything the comparisons look at, of one context.  `arrays`: the device's vertex and normal arrays too."""
    o, d = rays(pkg)
    r.validate_trees()
    t, f, u, v = r.probe_trace4(o, d)
    hit = f >= 0
    assert hit.mean() > 0.9
    shade = r.probe_hit_shade(f[hit], u[hit], v[hit], d[hit])
    lf, lrec, lpos = r.probe_lights()
    out = dict(zip(("vertex", "normal"), r.vertices())) if arrays else {}
    out.update({"t": t, "face": f, "u": u, "v": v, "shade": shade, "light_face": lf, "light_rec": lrec, "light_pos": lpos})
    if film:
        out["film"] = render_film(r, 4, 5)
    return out


def assert_same(a, b, skip=()):
    """Two states (or any two dicts of arrays) with the same keys, bit for bit but for the keys in `skip`; a failure names the key."""
    assert a.keys() == b.keys()
    for k in a:
        if k not in skip:
            assert np.array_equal(bits(a[k]), bits(b[k])), k


def assert_records(got, want, what):
    """The device's array against the restatement's, bit for bit; a failure names the first record."""
    bad = np.flatnonzero((bits(got) != bits(np.ascontiguousarray(want, np.float64))).any(axis=1))
    assert bad.size == 0, "%s %d of %d differing: device %r, restatement %r" % (what, bad[0], bad.size, got[bad[0]].tolist(), np.asarray(want)[bad[0]].tolist())


def assert_arrays(r, v, n):
    gv, gn = r.vertices()
    assert_records(gv, v, "vertex"); assert_records(gn, n, "normal")


def _any_hits(pkg, r):
    """Any-hit verdicts of both trace kernels for the suite's rays, each cut off at a fixed random distance."""
    o, d = rays(pkg)
    t2 = np.random.default_rng(9).uniform(0.05, 1.6, o.shape[0])
    return r.probe_trace4(o, d, t2=t2, any_hit=True)[1], r.probe_trace(o, d, t2=t2, any_hit=True)[1]


def _full_state(pkg, r):
    s = state(pkg, r)
    s["any4"], s["any2"] = _any_hits(pkg, r)
    return s


def _assert_same_rays(a, b, new_of_old, hidden=None):
    """State `a` of a context over the whole face list against state `b` of a context whose faces are numbered new_of_old[face of a] (-1: a face
    b does not have).  No ray of `a` names a face without a number; the hit masks are equal; t is bit for bit on hits; the faces are equal
    except where both report the same t bits -- an exact tie between two triangles, which two different trees may break differently --; u, v
    and the shade records are bit for bit where the faces agree; the any-hit verdicts are equal; the light lists are equal bit for bit, faces
    mapped; the films have equal sample counts and differ in rgb on at most 1 % of the pixels (the bound tests/test_gpu_bvh_build.py uses for
    two trees over one geometry)."""
    fa, fb = a["face"], b["face"]
    hit = fa >= 0
    assert np.array_equal(hit, fb >= 0)
    mapped = np.where(hit, new_of_old[np.maximum(fa, 0)], -1)
    assert np.all(mapped[hit] >= 0), "a ray names a hidden face"
    if hidden is not None:
        assert not hidden[fa[hit]].any()
    assert np.array_equal(bits(a["t"])[hit], bits(b["t"])[hit])
    agree = hit & (mapped == fb)
    tie = hit & ~agree
    assert np.array_equal(bits(a["t"])[tie], bits(b["t"])[tie])              # (implied by the line above: a differing face is an exact tie)
    print("faces agree on %.5f of the hits" % (agree.sum() / max(1, hit.sum())))
    assert agree.sum() >= 0.99 * hit.sum()
    for k in ("u", "v"):
        assert np.array_equal(bits(a[k])[agree], bits(b[k])[agree]), k
    assert np.array_equal(bits(a["shade"])[agree[hit]], bits(b["shade"])[agree[hit]])
    assert np.array_equal(a["any4"], b["any4"]) and np.array_equal(a["any2"], b["any2"])
    assert np.array_equal(new_of_old[a["light_face"]], b["light_face"])
    assert np.array_equal(bits(a["light_rec"]), bits(b["light_rec"])) and np.array_equal(bits(a["light_pos"]), bits(b["light_pos"]))
    if "film" in a:
        assert np.array_equal(a["film"][..., 3], b["film"][..., 3])
        share = float(np.mean(np.any(bits(a["film"][..., :3]) != bits(b["film"][..., :3]), axis=-1)))
        print("share of pixels whose rgb differs: %.5f" % share)
        assert share <= 0.01


def c_layout(cls, c_name, tmp_path, macros=()):
    """[sizeof, offsetof ...] of the struct `c_name` as a C compiler sees include/mcpt.h, the same of the ctypes class, and the integer values of
    the header's `macros`.  The header's ABI version is 4."""
    fields = [f[0] for f in cls._fields_]
    line = '  printf("%%zu%s\\n", sizeof(%s)%s);' % (" %zu" * len(fields), c_name, "".join(", offsetof(%s, %s)" % (c_name, f) for f in fields))
    consts = '  printf("%%u%s\\n", MCPT_ABI_VERSION%s);' % (" %lld" * len(macros), "".join(", (long long)(%s)" % m for m in macros))
    src = tmp_path / (c_name + ".c"); exe = str(tmp_path / c_name)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcpt.h"\nint main(void) {\n%s\n%s\n  return 0; }\n' % (line, consts))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [[int(x) for x in l.split()] for l in subprocess.check_output([exe]).decode().splitlines()]
    assert out[1][0] == 4
    return out[0], [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields], out[1][1:]


# ------------------------------------------------------------------------------------------------------------------------ host checks
def build_host_check(name, csrc_sources, tmp_path, sanitized=False, source=None):
    """Compile the host half of a feature -- `csrc_sources` of csrc/ -- with tests/<name>.cpp (or `source`) into a stand-alone program with a main
    of its own: no device is touched and nothing is loaded into Python.  `sanitized`: under the host's address and undefined-behaviour
    sanitizers.  Returns the executable."""
    exe = str(tmp_path / name)
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitized else []
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC] + extra +
                          [os.path.join(CSRC, s) for s in csrc_sources] + [source or os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe])
    return exe


def run_host_check(exe, tmp_path, sanitized=False):
    """Run the program on <tmp_path>/in.bin to write <tmp_path>/out.bin: it must end with 0, and the sanitizers must stay silent."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")                   # (the HIP runtime's start-up allocations are not this program's)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, ("sanitized: " if sanitized else "") + p.stderr[-3000:]
