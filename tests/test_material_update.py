"""Material, light and texture edits of a live context: mcpt_update_materials (csrc/materials.hip: the lobe class of every triangle
rewritten, the light list rebuilt by a stream compaction in face order), mcpt_update_texture, mcpt_get_material_info, the two probes and their
public surfaces.

The oracle throughout is this library's own fresh mcpt_create of the edited scene.  Geometry and builder are the same, so the trees are the same
(wide_tree_hash is asserted equal) and everything compared below is bit-equal: no tolerance anywhere.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import time

import numpy as np
import pytest

from tests import kit, visibility_ref as V
from tests.kit import bits, render_film

NEW_SYMBOLS = ["mcpt_update_materials", "mcpt_update_texture", "mcpt_get_material_info", "mcpt_probe_lights", "mcpt_probe_face_classes"]
INVALID, NO_LIGHTS = 1, 4


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_material_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS)


def test_null_context_is_an_invalid_argument_for_the_material_calls(pkg):
    lib = pkg.load_library()
    mats = (pkg.MaterialC * 2)(); tex = pkg.Texture(); info = pkg.MaterialInfo(); n = C.c_uint32(0)
    buf = np.zeros(64, np.float64); p = buf.ctypes.data_as(C.c_void_p)
    assert lib.mcpt_update_materials(None, mats, 2) == INVALID
    assert lib.mcpt_update_texture(None, 0, C.byref(tex)) == INVALID
    assert lib.mcpt_get_material_info(None, C.byref(info)) == INVALID
    assert lib.mcpt_probe_lights(None, 1, p, p, p, C.byref(n)) == INVALID
    assert lib.mcpt_probe_face_classes(None, p) == INVALID


# ------------------------------------------------------------------------------------------------------------------------ GPU helpers
W, H = 64, 64
WHITE, RED, GREEN, LIGHT, GLOSSY = range(5)
DET = 0x2                                                                    # FLAG_DETERMINISTIC


def _same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _scene(pkg):
    return pkg.scenes.cornell_box(W, H, sphere_lon=48, sphere_lat=24)


def _with_materials(pkg, scene, mats, vertex=None, normal=None):
    return pkg.scenes.SceneData(scene.name, scene.vertex if vertex is None else vertex, scene.normal if normal is None else normal, scene.texcoord,
                                scene.face, list(mats), scene.camera, dict(scene.meta))


def _edit(mats, **by_index):
    """A copy of `mats` with the materials named m<i>=dict(field=value) replaced."""
    out = list(mats)
    for k, fields in by_index.items():
        out[int(k[1:])] = dataclasses.replace(out[int(k[1:])], **fields)
    return out


def _camera_rays(r):
    od = kit.camera_rays(r, W, H, 1)[2]
    return od[:, :3], od[:, 3:]


def _look(r, paths=True):
    """Everything the tests compare between an edited and a fresh context."""
    lp, lxi = kit.light_points(0.0, 1.0, 4096, 11)
    out = {"lights": r.probe_lights(), "classes": r.probe_face_classes(), "sample_light": r.probe_sample_light(lp, lxi), "film": render_film(r, 4, 5)}
    if paths:
        o, d = _camera_rays(r)
        out["paths"] = r.probe_paths(o[::7], d[::7], seed=3)
    return out


def _assert_same_look(a, b):
    for k in a:
        assert _same(a[k], b[k]), k


def _fresh(pkg, scene, flags=DET, **kw):
    return pkg.Renderer(scene, max_depth=6, flags=flags, **kw)


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("gpu_tree", [False, True])
def test_update_with_the_creation_materials_is_the_identity(pkg, gpu_tree):
    scene = _scene(pkg)
    r = _fresh(pkg, scene, DET | (pkg.FLAG_GPU_BVH_BUILD if gpu_tree else 0))
    before = _look(r)
    bytes0 = r.info().device_bytes
    r.update_materials(scene.materials)
    _assert_same_look(before, _look(r))
    mi = r.material_info()
    assert mi.updates == 1 and mi.n_lights == 2 == r.info().n_lights and mi.last_ms > 0
    assert r.info().device_bytes >= bytes0 + 4 * r.info().n_tris             # the per-face scratch of the first call is counted
    r.close()


@pytest.mark.gpu
def test_membership_grows_past_capacity_then_shrinks(pkg):
    scene = _scene(pkg)
    n_sphere = int((scene.face[:, 0, 3] == GLOSSY).sum())
    assert n_sphere > 2000                                                   # several scan blocks, scattered in leaf order
    glow = _edit(scene.materials, m4=dict(radiance=(0.8, 0.5, 0.3)))
    only_sphere = _edit(glow, m3=dict(radiance=(0.0, 0.0, 0.0)))
    r = _fresh(pkg, scene)
    original = _look(r)
    bytes0 = r.info().device_bytes
    for mats, n_lights in ((glow, n_sphere + 2), (only_sphere, n_sphere)):
        r.update_materials(mats)
        f = _fresh(pkg, _with_materials(pkg, scene, mats))
        assert f.info().wide_tree_hash == r.info().wide_tree_hash
        got, want = _look(r), _look(f)
        faces = got["lights"][0]
        assert faces.size == n_lights and np.all(np.diff(faces) > 0)         # the reference's face order
        _assert_same_look(got, want)
        assert r.info().n_lights == f.info().n_lights == r.material_info().n_lights == n_lights
        assert r.info().device_bytes >= bytes0
        f.close()
    r.update_materials(scene.materials)
    _assert_same_look(original, _look(r))                                    # and back: the original picture, bit for bit
    assert r.material_info().updates == 3
    r.close()


@pytest.mark.gpu
def test_light_list_of_more_than_256_scan_blocks(pkg):
    """66 060 faces are 259 blocks of the light list's scan, so every thread of mt_offsets_kernel (csrc/materials.hip) sums a run of per = 2
    block sums and most runs are empty: the level of the scan that S-cornell's nine blocks never reach.  The sphere becomes an emitter on a live
    context -- against a fresh context of the edited scene, bit for bit --, then a random half of it is hidden -- against a fresh context of the
    sub-scene (tests/visibility_ref.py), faces mapped.  Three contexts of this size are created, with the host builder; the test prints what two of
    the creations took."""
    scene = pkg.scenes.cornell_box(W, H, sphere_lon=256, sphere_lat=130)
    nf = scene.face.shape[0]
    sphere = scene.face[:, 0, 3] == GLOSSY
    assert nf == 66060 and (nf + 255) // 256 == 259 and int(sphere.sum()) > 65536
    glow = _edit(scene.materials, m4=dict(radiance=(0.8, 0.5, 0.3)))
    glowing = _with_materials(pkg, scene, glow)
    flags = DET | pkg.FLAG_DYNAMIC
    lp, lxi = kit.light_points(0.0, 1.0, 4096, 11)
    t0 = time.perf_counter()
    r = _fresh(pkg, scene, flags)
    t1 = time.perf_counter()
    f = _fresh(pkg, glowing, flags)
    print("[66 060 faces] context creation, host builder: %.2f s and %.2f s" % (t1 - t0, time.perf_counter() - t1))
    assert f.info().wide_tree_hash == r.info().wide_tree_hash
    r.update_materials(glow)
    n_lights = int(sphere.sum()) + 2
    assert r.info().n_lights == f.info().n_lights == r.material_info().n_lights == n_lights
    got, want = r.probe_lights(), f.probe_lights()
    assert got[0].size == n_lights and np.all(np.diff(got[0]) > 0)
    assert _same(got, want)
    assert np.array_equal(r.probe_face_classes(), f.probe_face_classes())
    assert _same(r.probe_sample_light(lp, lxi), f.probe_sample_light(lp, lxi))
    f.close()
    # a random half of the sphere hidden: the flags of the scan are no longer one run of ones
    mask = np.ones(nf, np.uint8); mask[sphere] = np.random.default_rng(23).uniform(size=int(sphere.sum())) < 0.5
    sub, new_of_old = V.sub_scene(pkg, glowing, mask)
    s = _fresh(pkg, sub, flags)
    r.set_face_visibility(mask)
    n_lights = int(mask[sphere].sum()) + 2
    assert 0.45 * sphere.sum() < n_lights < 0.55 * sphere.sum()
    assert r.info().n_lights == s.info().n_lights == r.material_info().n_lights == n_lights
    assert r.visibility_info().n_hidden_emitters == int(sphere.sum()) + 2 - n_lights
    got, want = r.probe_lights(), s.probe_lights()
    assert np.all(np.diff(got[0]) > 0) and np.array_equal(new_of_old[got[0]], want[0])
    assert _same(got[1], want[1]) and _same(got[2], want[2])
    assert np.array_equal(r.probe_face_classes()[mask != 0], s.probe_face_classes())
    sr, ss = r.probe_sample_light(lp, lxi), s.probe_sample_light(lp, lxi)
    assert np.array_equal(new_of_old[sr[:, 8].astype(np.int64)], ss[:, 8].astype(np.int64))
    keep = [0, 1, 2, 3, 4, 5, 6, 7, 9]
    assert _same(sr[:, keep], ss[:, keep])
    r.close(); s.close()


@pytest.mark.gpu
def test_thresholds(pkg):
    base = _scene(pkg)
    # the lamp's second triangle gets a material of its own, so that one face can be the only light
    mats = list(base.materials) + [dataclasses.replace(base.materials[LIGHT], name="light2")]
    scene = _with_materials(pkg, base, mats)
    scene.face[11, :, 3] = 5
    assert (scene.face[:, 0, 3] == 5).sum() == 1
    r = _fresh(pkg, scene)
    nt = r.info().n_tris
    dim = 0.005 / np.sqrt(3.0)                                               # |radiance| = 0.005: emissive, but not in the light list
    cases = {
        "dim sphere": (_edit(mats, m4=dict(radiance=(dim, dim, dim))), 2),
        "every face": ([dataclasses.replace(m, radiance=(0.3, 0.2, 0.1)) for m in mats], nt),
        "one face": (_edit(mats, m3=dict(radiance=(0.0, 0.0, 0.0))), 1),
    }
    for name, (edited, n_lights) in cases.items():
        r.update_materials(edited)
        f = _fresh(pkg, _with_materials(pkg, scene, edited))
        assert f.info().wide_tree_hash == r.info().wide_tree_hash
        assert r.info().n_lights == f.info().n_lights == n_lights, name
        got, want = _look(r), _look(f)
        _assert_same_look(got, want)
        f.close()
    r.update_materials(_edit(mats, m4=dict(radiance=(dim, dim, dim))))
    plain = _fresh(pkg, scene)
    assert not np.array_equal(render_film(r, 4, 5), render_film(plain, 4, 5))                        # the dim sphere shows in the film
    r.close(); plain.close()


@pytest.mark.gpu
def test_lobe_classes(pkg):
    scene = _scene(pkg)
    edited = _edit(scene.materials, m0=dict(ks=(0.2, 0.2, 0.2), ns=50.0), m1=dict(ks=(0.1, 0.3, 0.1), ns=50.0), m2=dict(ks=(0.3, 0.1, 0.1), ns=50.0),
                   m4=dict(ns=10000.0))
    r = _fresh(pkg, scene)
    o1, d1 = _camera_rays(r); o2, d2 = kit.box_rays(0.0, 1.0, 3000, 3)
    o = np.concatenate([o1, o2]); d = np.concatenate([d1, d2])
    before = r.probe_trace4(o, d)
    classes0 = r.probe_face_classes()
    r.update_materials(edited)
    f = _fresh(pkg, _with_materials(pkg, scene, edited))
    assert f.info().wide_tree_hash == r.info().wide_tree_hash
    classes = r.probe_face_classes()
    assert np.array_equal(classes, f.probe_face_classes()) and not np.array_equal(classes, classes0)
    mat = scene.face[:, 0, 3]
    assert np.all(classes[mat == GLOSSY] == 2) and np.all(classes[mat <= GREEN] == 1) and np.all(classes[mat == LIGHT] == 0)
    after = r.probe_trace4(o, d)
    assert (before[1] >= 0).mean() > 0.3
    assert _same(before[0], after[0]) and np.array_equal(before[1], after[1])   # the tie ranks are untouched: the same t, the same face
    assert _same(render_film(r, 4, 5), render_film(f, 4, 5))
    r.close(); f.close()


@pytest.mark.gpu
def test_constant_colour_and_map_kd(pkg):
    scene = _scene(pkg)
    uv = np.random.default_rng(2).uniform(0, 1, (64, 2)).astype(np.float32)
    r = _fresh(pkg, scene)
    film0 = render_film(r, 4, 5)
    # a 1x1 Kd through update_texture
    blue = _edit(scene.materials, m1=dict(kd=(0.1, 0.2, 0.7)))
    r.update_texture(RED, np.asarray(blue[RED].kd, np.float32).reshape(1, 1, 3))
    f = _fresh(pkg, _with_materials(pkg, scene, blue))
    assert _same(r.probe_texture(RED, uv), f.probe_texture(RED, uv))
    film = render_film(r, 4, 5)
    assert _same(film, render_film(f, 4, 5)) and not np.array_equal(film, film0)
    assert r.material_info().updates == 0                                    # a texture edit is not a material update
    f.close()
    # ... and found by update_materials itself when the list's kd differs from the one held
    purple = _edit(scene.materials, m1=dict(kd=(0.5, 0.1, 0.6)), m4=dict(ns=20.0))
    r.update_materials(purple)
    f = _fresh(pkg, _with_materials(pkg, scene, purple))
    assert _same(r.probe_texture(RED, uv), f.probe_texture(RED, uv)) and _same(render_film(r, 4, 5), render_film(f, 4, 5))
    f.close()
    # the wrong size is refused and changes nothing
    film = render_film(r, 4, 5)
    with pytest.raises(pkg.McptError) as e:
        r.update_texture(RED, np.zeros((2, 2, 3), np.float32))
    assert "status %d" % INVALID in str(e.value)
    with pytest.raises(pkg.McptError):
        r.update_texture(len(scene.materials), np.zeros((1, 1, 3), np.float32))
    assert _same(render_film(r, 4, 5), film)
    # the red wall re-pointed at the green wall's texture
    r.update_materials(purple, map_kd=[0, GREEN, 2, 3, 4])
    twin = _edit(purple, m1=dict(kd=scene.materials[GREEN].kd))
    f = _fresh(pkg, _with_materials(pkg, scene, twin))
    assert _same(r.probe_texture(RED, uv), f.probe_texture(RED, uv)) and _same(render_film(r, 4, 5), render_film(f, 4, 5))
    r.close(); f.close()


@pytest.mark.gpu
def test_image_texture_is_replaced(pkg):
    scene = pkg.scenes.bathroom_stress(48, 32, detail=4, tex_size=8)
    other = pkg.scenes.value_noise_texture(8, 9, (0.2, 0.6, 0.3), 0.3)
    edited = _edit(scene.materials, m1=dict(texture=other))
    r = _fresh(pkg, scene); f = _fresh(pkg, _with_materials(pkg, scene, edited))
    assert f.info().wide_tree_hash == r.info().wide_tree_hash
    film0 = render_film(r, 4, 5)
    r.update_materials(edited)                                                # finds the changed image itself
    uv = np.random.default_rng(4).uniform(-1, 2, (256, 2)).astype(np.float32)
    assert _same(r.probe_texture(1, uv), f.probe_texture(1, uv))
    film = render_film(r, 4, 5)
    assert _same(film, render_film(f, 4, 5)) and not np.array_equal(film, film0)
    with pytest.raises(pkg.McptError) as e:
        r.update_texture(1, np.zeros((8, 4, 3), np.float32))
    assert "status %d" % INVALID in str(e.value)
    # back to back: the second call's texels must not overtake the first call's copy
    r.update_texture(1, pkg.material_texels(scene.materials[0])); r.update_texture(1, pkg.material_texels(edited[1]))
    assert _same(render_film(r, 4, 5), film)
    r.close(); f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["materials first", "vertices first"])
def test_with_a_vertex_update(pkg, order):
    scene = _scene(pkg)
    moved = kit.moved_sphere(pkg, scene)
    v, n = moved.vertex, moved.normal
    glow = _edit(scene.materials, m4=dict(radiance=(0.8, 0.5, 0.3)))
    r = _fresh(pkg, scene, DET | pkg.FLAG_DYNAMIC)
    f = _fresh(pkg, _with_materials(pkg, scene, glow, v, n))
    assert list(r.info().centre) == list(f.info().centre)
    if order == "materials first":
        r.update_materials(glow); r.update_vertices(v, n)
    else:
        r.update_vertices(v, n); r.update_materials(glow)
    r.validate_trees()
    got, want = _look(r, paths=False), _look(f, paths=False)
    assert _same(got["lights"], want["lights"]) and _same(got["sample_light"], want["sample_light"])
    # (the refitted tree is not the freshly built one, but closest hit and any hit do not depend on the tree)
    differ = np.any(bits(got["film"]) != bits(want["film"]), axis=-1)
    print("[materials + vertices] %s: %d of %d pixels differ from the fresh context" % (order, int(differ.sum()), differ.size))
    assert _same(got["film"], want["film"])
    # ... and the same two edits in the other order end in the same state, tree included
    g = _fresh(pkg, scene, DET | pkg.FLAG_DYNAMIC)
    if order == "materials first":
        g.update_vertices(v, n); g.update_materials(glow)
    else:
        g.update_materials(glow); g.update_vertices(v, n)
    _assert_same_look(got, _look(g, paths=False))
    r.close(); f.close(); g.close()


@pytest.mark.gpu
def test_ordering_without_a_sync(pkg):
    scene = _scene(pkg)
    # an edit that keeps the light count, so that the update itself has no reason to synchronise: the lamp's colour, a wall's, a mirror sphere
    glow = _edit(scene.materials, m3=dict(radiance=(4.0, 9.0, 14.0)), m4=dict(ns=10000.0), m1=dict(kd=(0.1, 0.2, 0.7)))
    r = _fresh(pkg, scene); old = _fresh(pkg, scene); new = _fresh(pkg, _with_materials(pkg, scene, glow))
    r.clear()
    r.render(4, seed=5)
    r.update_materials(glow)
    r.render(4, seed=6, first_sample=4)
    both = r.read_accum()
    old.render(4, seed=5); new.render(4, seed=6, first_sample=4)
    a, b = old.read_accum(), new.read_accum()
    assert _same(both, a + b)
    assert not np.array_equal(b, render_film(old, 4, 6))
    for x in (r, old, new):
        x.close()


@pytest.mark.gpu
def test_refusals_change_nothing(pkg):
    scene = _scene(pkg)
    r = _fresh(pkg, scene)
    before = _look(r, paths=False)
    r.render_features(4, seed=5); r.features()
    nan = _edit(scene.materials, m3=dict(radiance=(17.0, float("nan"), 4.0)))
    inf = _edit(scene.materials, m4=dict(ns=float("inf")))
    dark = [dataclasses.replace(m, radiance=(0.0, 0.0, 0.0)) for m in scene.materials]
    faint = _edit(scene.materials, m3=dict(radiance=(0.005, 0.0, 0.0)))       # emissive, but no face would be left in the list
    for mats, kd, status in ((scene.materials[:-1], None, INVALID), (scene.materials + scene.materials[:1], None, INVALID),
                             (scene.materials, [0, 1, 2, 3, 5], INVALID), (scene.materials, [0, -1, 2, 3, 4], INVALID), (nan, None, INVALID),
                             (inf, None, INVALID), (dark, None, NO_LIGHTS), (faint, None, NO_LIGHTS)):
        with pytest.raises(pkg.McptError) as e:
            r.update_materials(mats, map_kd=kd)
        assert "status %d" % status in str(e.value)
    assert r.lib.mcpt_update_materials(r.ctx, None, len(scene.materials)) == INVALID
    n = C.c_uint32(0)
    assert r.lib.mcpt_probe_lights(r.ctx, 1, None, None, None, C.byref(n)) == INVALID and n.value == 2
    r.features()                                                              # still there after the refused calls
    assert r.material_info().updates == 0
    _assert_same_look(before, _look(r, paths=False))
    r.close()


@pytest.mark.gpu
def test_clone_and_derived_buffers(pkg):
    scene = _scene(pkg)
    glow = _edit(scene.materials, m4=dict(radiance=(0.8, 0.5, 0.3), ns=10000.0), m0=dict(kd=(0.2, 0.6, 0.7)))
    r = _fresh(pkg, scene)
    r.render_features(4, seed=5); r.denoise()
    r.update_materials(glow)
    for call in (r.features, r.denoise):                                      # gone, as on a context that never had them
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % INVALID in str(e.value)
    c = r.clone()
    f = _fresh(pkg, _with_materials(pkg, scene, glow))
    want = _look(f)
    _assert_same_look(_look(c), want)
    _assert_same_look(_look(r), want)
    c.update_materials(scene.materials)                                       # a clone carries the host tables: it can be edited in turn
    plain = _fresh(pkg, scene)
    _assert_same_look(_look(c), _look(plain))
    _assert_same_look(_look(r), want)                                         # the source did not change with its clone
    for x in (r, c, f, plain):
        x.close()


@pytest.mark.gpu
def test_recursive_integrator(pkg):
    scene = _scene(pkg)
    glow = _edit(scene.materials, m4=dict(radiance=(0.8, 0.5, 0.3)), m1=dict(ks=(0.2, 0.2, 0.2), ns=80.0))
    r = _fresh(pkg, scene, integrator=pkg.INTEGRATOR_RECURSIVE_NEE)
    r.update_materials(glow)
    f = _fresh(pkg, _with_materials(pkg, scene, glow), integrator=pkg.INTEGRATOR_RECURSIVE_NEE)
    _assert_same_look(_look(r, paths=False), _look(f, paths=False))
    r.close(); f.close()


@pytest.mark.gpu
def test_facade_update_materials(pkg, tmp_path):
    exe = kit.build_facade("facade_materials.cpp", tmp_path)
    a = pkg.scenes.cornell_box(44, 30, sphere_lon=24, sphere_lat=12)
    b = _with_materials(pkg, a, _edit(a.materials, m4=dict(radiance=(0.8, 0.5, 0.3), ns=10000.0), m1=dict(kd=(0.1, 0.2, 0.7)), m3=dict(radiance=(9.0, 9.0, 9.0))))
    obj_a = a.write(str(tmp_path / "a")); obj_b = b.write(str(tmp_path / "b"))
    outs = [str(tmp_path / n) for n in ("edited.bin", "fresh.bin", "refused.bin", "refused_fresh.bin")]
    k = 5
    line = kit.run_facade(exe, [obj_a, obj_b, str(k)] + outs)
    w, h = int(line[0]), int(line[1])
    assert (w, h, int(line[2])) == (44, 30, k)
    edited, fresh, refused, refused_fresh = [np.fromfile(p, np.float32).reshape(h, w, 4) for p in outs]
    assert np.all(edited[..., 3] == k)                                        # the picture restarted and ends at k samples
    assert _same(edited, fresh)
    assert np.all(refused[..., 3] == k + 1)                                   # refused edits did not restart it ...
    assert _same(refused, refused_fresh)                                      # ... and left the look as it was


@pytest.mark.gpu
def test_cli_light_pulse(pkg, tmp_path):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    out = str(tmp_path / "img")
    p = kit.run_cli([obj, "--turntable", "3", "--light-pulse", "0.6", "--spp", "4", "--depth", "5", "--out", out])
    assert p.returncode == 0, p.stderr[-2000:]
    imgs = kit.turntable_frames(out)
    assert len(set(imgs)) == 3
    p = kit.run_cli([obj, "--turntable", "3", "--light-pulse", "0.6", "--reproject", "8", "--spp", "4", "--out", out])
    assert p.returncode == 2 and "--light-pulse" in p.stderr
