"""-m gpu: the ray-generation stage (csrc/camera.hip) through the C ABI -- that with the PINHOLE model it is today's camera,
ray for ray and film for film; that the film of every model is made of exactly the rays the probe shows; every ray of every model against the
float64 restatement of tests/camera_ref.py within S_BOUND, which tests/test_camera_ref.py derives on the CPU; autofocus and the plane in focus;
refusals and what the calls leave alone; the C++ facade and mcpt_cli.

The device draws its own pixel jitter and lens sample, rng_block(pixel, sample, 0): the tests read them through probe_rng and hand them to the
restatement.  Films are at most 33 x 17 and 32 x 32 (the facade's and the CLI's 44 x 30 and 40 x 32 apart, as in the other suites).
"""
from __future__ import annotations

import ctypes as C
import glob

import numpy as np
import pytest

from tests import camera_ref as R, endpoints_ref as E, kit
from tests.kit import bits

pytestmark = pytest.mark.gpu

SEED = 20262
INVALID, UNSUPPORTED = 1, 6
W, H = 33, 17


def _pixels(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel(), ys.ravel()], -1).astype(np.int32)


def _xi(r, xy, w, sample, seed):
    """The camera block's four numbers of every pixel of xy for (sample, seed), from the generator itself."""
    key = np.stack([xy[:, 1].astype(np.int64) * w + xy[:, 0], np.full(len(xy), sample), np.zeros(len(xy), np.int64)], 1)
    return r.probe_rng(key.astype(np.uint32), seed)


def _camera(pkg, c, w, h):
    return pkg.scenes.Camera(c["eye"], c["lookat"], c["up"], c["fovy"], w, h)


def _centred_box(pkg, w, h):
    """open_box moved so that the centre every device coordinate is relative to is exactly 0, seen from inside (the panorama has walls all around):
    (o + centre) - centre is then o itself, in fp64 as in fp32, and probe_paths starts from the very origins the stage wrote."""
    s = pkg.scenes.open_box(w, h)
    used = s.vertex[np.unique(s.face[:, :, 0])]
    v = s.vertex - (0.5 * used.min(0) + 0.5 * used.max(0))
    cam = pkg.scenes.Camera((0.05, -0.1, 0.35), (0.0, -0.15, -0.5), (0.0, 1.0, 0.0), 55.0, w, h)
    return kit.with_arrays(pkg, s, vertex=v, camera=cam)


def test_pinhole_stage_is_todays_camera_ray_for_ray(pkg):
    """PINHOLE probe_camera_rays against probe_cast_ray fed the generator's own jitter, bit for bit: on the two films of E.FILMS that fit the
    suite's size and three cameras of E.camera_cases (a wide view, a skewed up, an eye 1e6 away), samples 0, 1 and 7 -- with the model never set
    and with PINHOLE set explicitly."""
    n_rays = 0
    for w, h in [f for f in E.FILMS if f[0] <= W and f[1] <= H]:
        scene = pkg.scenes.open_box(w, h)
        r = pkg.Renderer(scene)
        centre = np.array(r.info().centre)
        cams = {c[1]: c[2] for c in E.camera_cases(scene.camera, centre)}
        xy = E.pixel_cases(w, h)[0]
        for k, name in enumerate(("fovy 179.9", "up skewed", "eye + 1e+06")):
            r.set_camera(_camera(pkg, cams[name], w, h))
            if k == 1:
                r.set_camera_model(pkg.CAMERA_PINHOLE)
            assert r.camera_model().model == pkg.CAMERA_PINHOLE
            for sample in (0, 1, 7):
                o, d = r.probe_camera_rays(xy, sample, SEED)
                cast = r.probe_cast_ray(xy, _xi(r, xy, w, sample, SEED)[:, :2])
                assert np.array_equal(d, d.astype(np.float32).astype(np.float64))            # the doubles hold fp32 values
                assert np.array_equal(bits(d.astype(np.float32)), bits(cast[:, 3:6])), (w, h, name, sample)
                assert np.array_equal(bits((o + centre).astype(np.float32)), bits(cast[:, 0:3])), (w, h, name, sample)
                n_rays += len(xy)
        r.close()
    print("%d rays, all equal" % n_rays)
    assert n_rays > 2000


def test_pinhole_stage_is_todays_camera_film_for_film(pkg):
    """open_box 33 x 17, depth 4: one pass of render_camera is render(1, seed, s) bit for bit, colour sums and counts, for s = 0, 1, 2; three passes
    in one call are the three single passes accumulated."""
    r = pkg.Renderer(pkg.scenes.open_box(W, H), max_depth=4)
    r.clear()
    for s in (0, 1, 2):
        r.clear(); r.render_camera(1, SEED, s); a = r.read_accum()
        r.clear(); r.render(1, SEED, s); b = r.read_accum()
        assert np.array_equal(bits(a), bits(b)), "sample %d: %d pixels differ" % (s, (bits(a) != bits(b)).any(-1).sum())
        assert (a[..., 3] == 1).all() and a[..., :3].max() > 0
    r.clear()
    for s in (0, 1, 2):
        r.render_camera(1, SEED, s)
    single = r.read_accum()
    r.clear(); r.render_camera(3, SEED, 0)
    assert np.array_equal(bits(single), bits(r.read_accum())) and (single[..., 3] == 3).all()
    r.close()


MODELS = [("pinhole", dict(model=0)), ("thin_lens", dict(model=1, lens_radius=0.05, focus_distance=0.6, blades=5, blade_rotation=0.3)),
          ("orthographic", dict(model=2, ortho_height=0.5)), ("panorama", dict(model=3))]


@pytest.mark.parametrize("name,params", MODELS, ids=[m[0] for m in MODELS])
def test_the_film_is_made_of_the_probed_rays(pkg, name, params):
    """One pass of render_camera against probe_paths started from the rays probe_camera_rays shows for the same sample and seed: the colour sums
    equal bit for bit (NaN zeroed on both sides), every count 1.  The scene's centre is 0, so the origins pass through probe_paths' world
    coordinates unchanged -- asserted in numpy first, as float32(o) == float32((o + centre) - centre)."""
    r = pkg.Renderer(_centred_box(pkg, W, H), max_depth=4)
    centre = np.array(r.info().centre)
    assert np.array_equal(centre, np.zeros(3))
    r.set_camera_model(**params)
    o, d = r.probe_camera_rays(_pixels(W, H), 0, SEED)
    assert np.array_equal(bits(o.astype(np.float32)), bits(((o + centre) - centre).astype(np.float32)))
    assert np.array_equal(bits(o), bits((o + centre) - centre))
    want = np.nan_to_num(r.probe_paths(o + centre, d, SEED), nan=0.0)
    r.clear(); r.render_camera(1, SEED, 0)
    film = r.read_accum().reshape(-1, 4)
    assert (film[:, 3] == 1).all()
    got = np.nan_to_num(film[:, :3], nan=0.0)
    diff = (bits(got) != bits(want)).any(1)
    assert not diff.any(), "%s: %d of %d pixels differ, first %d: film %s, probe %s" % (name, diff.sum(), len(diff), np.flatnonzero(diff)[0], got[diff][0], want[diff][0])
    assert (got.max(1) > 0).mean() > 0.25                                     # (the view is of lit walls, not of nothing; the panorama also looks out of the open side)
    if name != "pinhole":                                                    # and it is another picture than the pinhole's
        r.clear(); r.render(1, SEED, 0)
        assert not np.array_equal(r.read_accum().reshape(-1, 4)[:, :3], film[:, :3])
    r.close()


def test_rays_against_float64(pkg):
    """Every model of model_cases on every film of R.FILMS and camera of R.CAMERAS, the pixels of R.pixel_cases, samples 0 and 3: each origin
    component within S_BOUND 2^-52 (1 + |x|) of the float64 restatement, each direction component within half an fp32 ulp of it plus that.  No case
    is forgiven; the worst ratio per pixel family and per model is printed.  lens_radius = 0 gives the eye exactly."""
    fams, models, ratios = [], [], []
    used_o = used_d = 0.0
    for w, h in R.FILMS:
        scene = pkg.scenes.open_box(w, h)
        r = pkg.Renderer(scene)
        centre = np.array(r.info().centre)
        cams = {c[1]: c[2] for c in E.camera_cases(scene.camera, centre)}
        xy, _, fam = R.pixel_cases(w, h)
        assert set(fam) == {"corners", "last_column", "xi_edges", "random", "panorama_pole", "panorama_seam"}
        for cname in R.CAMERAS:
            camera = _camera(pkg, cams[cname], w, h)
            r.set_camera(camera)
            cam = R.device_camera(camera, centre)
            for sample in (0, 3):
                xi = _xi(r, xy, w, sample, SEED)
                for name, model, kw in R.model_cases():
                    r.set_camera_model(model=model, lens_radius=kw.get("lens_radius", 0.0), focus_distance=kw.get("focus_distance", 0.0), blades=kw.get("blades", 0),
                                       blade_rotation=kw.get("rotation", 0.0), ortho_height=kw.get("ortho_height", 0.0))
                    o, d = r.probe_camera_rays(xy, sample, SEED)
                    ref_o, ref_d = R.rays(model, cam, w, h, xy, xi, **kw)
                    ratio = R.ray_ratio(o, d, ref_o, ref_d)
                    uo, ud = R.ray_slack_used(o, d, ref_o, ref_d); used_o = max(used_o, uo); used_d = max(used_d, ud)
                    i = int(ratio.argmax())
                    assert ratio[i] <= 1, "film %dx%d, camera %s, %s, sample %d, pixel %s (%s): error / bound %.3g; got %s %s, want %s %s" % (
                        w, h, cname, name, sample, xy[i], fam[i], ratio[i], o[i], d[i], ref_o[i], ref_d[i])
                    if model == R.THIN_LENS and kw["lens_radius"] == 0.0:
                        assert (o == cam[4][None]).all()
                    fams.append(fam); models.append(np.full(len(ratio), name.split(" radius")[0])); ratios.append(ratio)
        r.close()
    fams, models, ratios = np.concatenate(fams), np.concatenate(models), np.concatenate(ratios)
    E.print_worst("camera rays, by pixel family", fams, ratios)
    E.print_worst("camera rays, by model", models, ratios)
    print("%d rays; of the float64 slack (S_BOUND = %g units) the origins use %.3f units, the directions %.3f beyond their half fp32 ulp" % (len(ratios), R.S_BOUND, used_o, used_d))


def test_autofocus_and_the_plane_in_focus(pkg):
    """cornell_box_small 32 x 32: autofocus on a pixel is t dot(d, front) of that pixel's first hit, to the rounding of the three products and two sums
    in float64 (8 x 2^-53 of t sum |d_i front_i|).  With that focus and a lens of radius 1 every ray of 256 samples meets the plane
    dot(x - eye, front) = focus within focus |D| 4 x 2^-24 of eye + focus D(u, v): the fp32 rounding of its direction, scaled to the plane.  A pixel
    that sees nothing and a pixel outside the film are refused."""
    w = h = 32
    scene = pkg.scenes.cornell_box_small(w, h)
    r = pkg.Renderer(scene)
    centre = np.array(r.info().centre)
    hh, front, right, up, eye = R.device_camera(scene.camera, centre)
    face, uvt = r.probe_first_hits()
    worst = 0.0
    for px, py in ((16, 9), (3, 28), (30, 16)):
        assert face[py, px] >= 0
        t = float(uvt[py, px, 2])
        d = r.probe_cast_ray(np.array([[px, py]], np.int32), np.full((1, 2), 0.5, np.float32))[0, 3:6].astype(np.float64)
        f = r.autofocus(px, py)
        assert abs(f - t * float((d * front).sum())) <= 8 * 2.0 ** -53 * t * float(np.abs(d * front).sum()), (px, py, f)
        r.set_camera_model(pkg.CAMERA_THIN_LENS, lens_radius=1.0, focus_distance=f)
        xy = np.array([[px, py]], np.int32)
        key = np.array([[py * w + px, s, 0] for s in range(256)], np.uint32)
        xi = r.probe_rng(key, SEED)
        for s in range(256):
            o, dd = r.probe_camera_rays(xy, s, SEED)
            o, dd = o[0], dd[0]
            u = (float((np.float32(px) + xi[s, 0]) / np.float32(w)) - 0.5) * hh * w / h; v = (float((np.float32(py) + xi[s, 1]) / np.float32(h)) - 0.5) * hh
            D = front + u * right + v * up
            tt = (f - float(((o - eye) * front).sum())) / float((dd * front).sum())
            miss = float(np.linalg.norm(o + tt * dd - (eye + f * D)))
            bound = f * float(np.linalg.norm(D)) * 4 * 2.0 ** -24
            worst = max(worst, miss / bound)
            assert miss <= bound, (px, py, s, miss, bound)
    print("plane in focus: worst miss / bound %.3f" % worst)
    before = bytes(r.camera_model())
    for px, py in ((-1, 0), (w, 0), (0, h), (0, -1)):
        with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_autofocus" % INVALID):
            r.autofocus(px, py)
    c = scene.camera
    r.set_camera(pkg.scenes.Camera(c.eye, (0.5, 0.5, 5.0), c.up, c.fovy, w, h))                  # looks away from the box
    assert (r.probe_first_hits()[0] < 0).all()
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_autofocus: the pixel-centre ray hits nothing" % INVALID):
        r.autofocus(16, 16)
    assert bytes(r.camera_model()) == before
    r.close()


def test_refusals_and_state(pkg):
    """Every range of the model's fields is refused with the model unchanged; fields of other models are ignored; render_camera on a recursive-integrator
    context is unsupported; set_camera keeps the model and a clone carries it (not the ray buffers); the ray buffers are 48 B per pixel, allocated by
    the first render_camera and only then; n_lights, the film of a following render() and the features are what a context gives that never heard of
    camera models."""
    scene = pkg.scenes.open_box(W, H)
    r = pkg.Renderer(scene, max_depth=4); plain = pkg.Renderer(scene, max_depth=4)
    lib = r.lib
    good = dict(model=pkg.CAMERA_THIN_LENS, lens_radius=0.1, focus_distance=2.0, blades=6, blade_rotation=0.5, ortho_height=-3.0)   # (ortho_height: another model's field)
    r.set_camera_model(**good)
    before = bytes(r.camera_model())
    assert r.camera_model().as_dict() == dict(good, struct_size=64)
    nan, inf = float("nan"), float("inf")
    bad = [dict(model=4), dict(model=0xffffffff)]
    bad += [dict(model=1, focus_distance=1.0, lens_radius=x) for x in (-1e-300, -1.0, nan, inf)]
    bad += [dict(model=1, lens_radius=0.1, focus_distance=x) for x in (0.0, -1.0, nan, inf)]
    bad += [dict(model=1, lens_radius=0.1, focus_distance=1.0, blades=x) for x in (1, 2, 17, 1000)]
    bad += [dict(model=1, lens_radius=0.1, focus_distance=1.0, blades=5, blade_rotation=x) for x in (nan, inf, -inf)]
    bad += [dict(model=2, ortho_height=x) for x in (0.0, -1.0, nan, inf)]
    for kw in bad:
        with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_set_camera_model" % INVALID):
            r.set_camera_model(**kw)
        assert bytes(r.camera_model()) == before, kw
    m = pkg.camera_model(**good); m.struct_size = 60
    assert lib.mcpt_set_camera_model(r.ctx, C.byref(m)) == INVALID and bytes(r.camera_model()) == before
    r.set_camera_model(pkg.CAMERA_EQUIRECT, lens_radius=-1.0, focus_distance=nan, blades=99, ortho_height=-1.0)     # fields of other models are ignored
    assert lib.mcpt_set_camera_model(r.ctx, None) == 0 and r.camera_model().model == pkg.CAMERA_PINHOLE             # NULL = PINHOLE
    r.set_camera_model(**good)
    # set_camera keeps the model, a clone carries it
    c = scene.camera
    r.set_camera(pkg.scenes.Camera((0.4, 0.5, 2.0), c.lookat, c.up, 50.0, W, H))
    assert bytes(r.camera_model()) == before
    r.set_camera(c)
    # the ray buffers: the path pool of a whole-film probe job is there already after probe_paths, so device_bytes grows by the buffers alone
    o, d = plain.probe_camera_rays(_pixels(W, H), 0, SEED)
    centre = np.array(r.info().centre)
    r.probe_paths(o + centre, d, SEED)
    i0 = r.camera_model_info()
    assert (i0.model, i0.renders, i0.passes, i0.device_bytes, i0.last_stage_ms) == (pkg.CAMERA_THIN_LENS, 0, 0, 0, 0.0)
    bytes0 = r.info().device_bytes
    r.render_camera(0, SEED, 0)                                              # spp = 0 does nothing
    assert r.info().device_bytes == bytes0 and r.camera_model_info().renders == 0
    r.clear(); r.render_camera(2, SEED, 0)
    i1 = r.camera_model_info()
    assert (i1.renders, i1.passes, i1.device_bytes) == (1, 2, 48 * W * H) and r.info().device_bytes == bytes0 + 48 * W * H and i1.last_stage_ms > 0
    launches = r.counters().launches
    r.render_camera(1, SEED, 2)
    i2 = r.camera_model_info()
    assert (i2.renders, i2.passes, i2.device_bytes) == (2, 3, 48 * W * H) and r.info().device_bytes == bytes0 + 48 * W * H
    assert r.counters().launches == launches + 1 and (r.read_accum()[..., 3] == 3).all()
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_render_camera: first_sample" % INVALID):
        r.render_camera(2, SEED, 2 ** 32 - 1)
    k = r.clone()
    assert bytes(k.camera_model()) == before and k.camera_model_info().device_bytes == 0 and k.camera_model_info().renders == 0
    ko, kd = k.probe_camera_rays(_pixels(W, H)[:64], 1, SEED); ro, rd = r.probe_camera_rays(_pixels(W, H)[:64], 1, SEED)
    assert np.array_equal(bits(ko), bits(ro)) and np.array_equal(bits(kd), bits(rd))
    k.close()
    # what the calls leave alone
    assert r.info().n_lights == plain.info().n_lights
    assert np.array_equal(bits(kit.render_film(r, 1, SEED)), bits(kit.render_film(plain, 1, SEED)))
    r.render_features(4, 5); plain.render_features(4, 5)
    assert np.array_equal(bits(r.features()), bits(plain.features()))
    r.close(); plain.close()
    rec = pkg.Renderer(scene, max_depth=4, integrator=pkg.INTEGRATOR_RECURSIVE_NEE)
    rec.set_camera_model(**good)                                             # the model is state of every context
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_render_camera" % UNSUPPORTED):
        rec.render_camera(1, SEED, 0)
    rec.close()


def test_facade_camera_model(pkg, tmp_path):
    """Render::set_camera_model, render_camera and autofocus through the host classes: the program itself asserts that the PINHOLE film equals
    Render::render's; its thin-lens film is render_camera's with the focus autofocus gave."""
    exe = kit.build_facade("facade_camera.cpp", tmp_path)
    a = pkg.scenes.cornell_box(44, 30, sphere_lon=24, sphere_lat=12)
    obj = a.write(str(tmp_path / "a"))
    out = str(tmp_path / "lens.bin")
    k, px, py = 3, 22, 8
    line = kit.run_facade(exe, [obj, str(k), str(px), str(py), out])
    w, h = int(line[0]), int(line[1])
    assert (w, h, int(line[2])) == (44, 30, k)
    r = pkg.Renderer(a, max_depth=6, flags=pkg.FLAG_DETERMINISTIC)
    f = r.autofocus(px, py)
    assert f == float(line[3]) and 0.5 < f < 3.0
    r.set_camera_model(pkg.CAMERA_THIN_LENS, lens_radius=0.05, focus_distance=f, blades=5)
    r.clear(); r.render_camera(k, 17, 0)
    lens = np.fromfile(out, np.float32).reshape(h, w, 4)
    assert np.array_equal(bits(lens), bits(r.read_accum())) and (lens[..., 3] == k).all()
    r.close()


def test_cli_camera_models(pkg, tmp_path):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    frames = {}
    for name, extra in (("plain", []), ("lens", ["--aperture", "0.05", "--autofocus", "20", "22", "--blades", "6", "--blade-rotation", "15"]),
                        ("fixed", ["--aperture", "0.05", "--focus", "1.9"]), ("ortho", ["--ortho", "1.0"]),
                        ("panorama", ["--panorama"])):
        out = str(tmp_path / name)
        p = kit.run_cli([obj, "--turntable", "2", "--spp", "2", "--depth", "5", "--deterministic", "--out", out] + extra)
        assert p.returncode == 0, p.stderr[-2000:]
        assert ("autofocus: pixel (20, 22)" in p.stdout) == (name == "lens")
        frames[name] = kit.turntable_frames(out, 2)
    assert len({tuple(v) for v in frames.values()}) == 5
    out = str(tmp_path / "still")
    p = kit.run_cli([obj, "--spp", "3", "--batch", "2", "--depth", "5", "--out", out, "--panorama", "--denoise"])
    assert p.returncode == 0 and p.stderr.count("pinhole view") == 1, p.stderr[-2000:]
    assert len(glob.glob(out + "*.png")) >= 2
    for bad, word in ((["--aperture", "0.1"], "--focus"), (["--aperture", "0.1", "--focus", "1", "--autofocus", "1", "1"], "exactly one"), (["--focus", "1"], "--aperture"),
                      (["--ortho", "0"], "H > 0"), (["--ortho", "1", "--panorama"], "exclude"), (["--panorama", "--adaptive", "0.1"], "--adaptive"),
                      (["--aperture", "0.1", "--focus", "1", "--blades", "2"], "[3, 16]"), (["--panorama", "--recursive"], "--recursive")):
        p = kit.run_cli([obj, "--spp", "1", "--out", out] + bad)
        assert p.returncode == 2 and word in p.stderr, (bad, p.stderr[-500:])
    p = kit.run_cli([obj, "--spp", "1", "--out", out, "--aperture", "0.1", "--autofocus", "400", "400"])
    assert p.returncode == 1 and "outside the film" in p.stderr
