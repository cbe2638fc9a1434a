"""Denoised preview, the two opt-in flags of mcpt_denoise_opts (csrc/denoise.hip): emitted light kept apart from reflected
light (MCPT_DENOISE_SPLIT_EMISSION, the emission buffer) and fireflies clamped before the filter (MCPT_DENOISE_CLAMP_FIREFLIES).

CPU tests pin the numpy restatement (tests/denoise_robust_ref.py) and the layout of the options; GPU tests check the emission buffer against
the function-level probes, the filter against the restatement by the rule of tests/test_denoise.py, the bookkeeping of the buffer, the
refusals, and the quality against a converged image next to the filter without the flags.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from tests import kit
from tests.denoise_ref import denoise_ref, pixel_angle
from tests.denoise_robust_ref import CLAMP, DEFAULT_FIREFLY_CLAMP, SPLIT, clamp_fireflies, denoise_robust_ref
from tests.test_denoise import THETA, _assert_matches_ref, _close_frac, _planar, _tonemap

FLAGS = {"split": SPLIT, "clamp": CLAMP, "both": SPLIT | CLAMP}


def _kw(flags):
    return dict(split_emission=bool(flags & SPLIT), clamp_fireflies=bool(flags & CLAMP))


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_ref_without_flags_is_the_reference_filter():
    rng = np.random.default_rng(11)
    h, w = 21, 34
    film = kit.synthetic_film(h, w, 4)
    feat = np.zeros((h, w, 8), np.float32)
    feat[..., :3] = rng.uniform(0.0, 0.9, (h, w, 3)); feat[..., 3] = rng.choice([0.25, 0.5, 1.0], (h, w))
    feat[..., 4:7] = rng.normal(size=(h, w, 3)) * 0.2 + (0, 0, 1); feat[..., 7] = rng.uniform(1.5, 2.5, (h, w))
    emis = rng.uniform(0, 1, (h, w, 4)).astype(np.float32)
    for kw in (dict(), dict(iterations=2, sigma_color=2.0, sigma_normal=16.0, sigma_depth=1.0)):
        assert np.array_equal(denoise_robust_ref(film, feat, emis, THETA, flags=0, firefly_clamp=3.0, **kw), denoise_ref(film, feat, THETA, **kw))
        assert np.array_equal(denoise_robust_ref(film, feat, None, THETA, **kw), denoise_ref(film, feat, THETA, **kw))


def _band(h=24, w=32, albedo=0.5, irr=0.8, e=(6.0, 4.0, 2.0), spp=4):
    """A planar image of constant irradiance whose columns 14 .. 16 are partly covered by a light: coverage 0.75 (so they count as surface),
    albedo scaled by the coverage, and a quarter of the samples carrying the radiance e.  Returns film, feat, emis and the true image."""
    film, feat = _planar(h, w, albedo=albedo, irr=irr, spp=spp)
    band = np.zeros((h, w), bool); band[:, 14:17] = True
    emis = np.zeros((h, w, 4), np.float32)
    emis[band, :3] = np.asarray(e, np.float32) * 0.25; emis[band, 3] = 0.25
    feat[band, :3] = albedo * 0.75; feat[band, 3] = 0.75
    truth = np.where(band[..., None], np.float32(albedo * 0.75 * irr) + emis[..., :3], np.float32(albedo * irr))
    film[..., :3] = truth * spp
    return film, feat, emis, truth.astype(np.float64), band


def test_ref_split_keeps_emitted_light_out_of_the_filter():
    film, feat, emis, truth, band = _band()
    out = denoise_robust_ref(film, feat, emis, THETA, flags=SPLIT)
    assert np.abs(out[..., :3] - truth).max() <= 1e-5 and np.all(out[..., 3] == 1)
    plain = denoise_robust_ref(film, feat, emis, THETA, flags=0)
    near = np.zeros_like(band); near[:, 13:18] = True                      # the band and its neighbours
    assert np.all(np.abs(plain[near][:, :3] / truth[near] - 1.0).max(-1) > 0.10)


def test_ref_split_clamps_at_zero():
    film, feat, emis, truth, band = _band()
    emis[band, :3] *= 8.0                                                    # an estimate far above what the film holds
    out = denoise_robust_ref(film, feat, emis, THETA, flags=SPLIT)
    assert np.all(np.isfinite(out)) and np.all(out[..., :3] >= 0)
    assert np.allclose(out[~band][:, :3], 0.4, rtol=0.5)                     # the reflected part of the band is 0, never negative


def test_ref_clamp_removes_a_firefly():
    film, feat = _planar(20, 28)
    film[9, 13, :3] *= 100.0
    out = denoise_robust_ref(film, feat, None, THETA, flags=CLAMP, firefly_clamp=1.0)
    assert np.abs(out[..., :3] - 0.4).max() <= 1e-5
    plain = denoise_robust_ref(film, feat, None, THETA, flags=0)
    assert np.abs(plain[..., :3] - 0.4).max() > 0.1
    # continuous at the threshold: a pixel exactly k times its neighbours is left alone, one just above moves by just as little
    film, feat = _planar(20, 28)
    film[9, 13, :3] *= 2.0
    at = denoise_robust_ref(film, feat, None, THETA, flags=CLAMP, firefly_clamp=2.0)
    assert np.array_equal(at, denoise_robust_ref(film, feat, None, THETA, flags=0))
    film[9, 13, :3] *= np.float32(1.0 + 1e-6)
    assert np.abs(denoise_robust_ref(film, feat, None, THETA, flags=CLAMP, firefly_clamp=2.0) - at).max() <= 1e-5


def test_ref_pixel_without_valid_neighbour_is_never_clamped():
    film, feat = _planar(12, 12)
    feat[4:7, 4:7, 3] = 0.25; feat[5, 5, 3] = 1.0                           # an island: all eight neighbours are invalid
    film[5, 5, :3] *= 1000.0
    film[0, 0, :3] *= 1000.0                                                 # a corner has three neighbours: clamped
    valid = feat[..., 3] >= 0.5
    irr = film[..., :3].astype(np.float64) / 4 / 0.5
    got, hot = clamp_fireflies(np.where(valid[..., None], irr, 0.0), valid, 1.0)
    assert not hot[5, 5] and np.array_equal(got[5, 5], irr[5, 5]) and hot[0, 0] and hot.sum() == 1
    a = denoise_robust_ref(film, feat, None, THETA, flags=CLAMP, firefly_clamp=1.0)
    b = denoise_robust_ref(film, feat, None, THETA, flags=0)
    assert np.array_equal(a[5, 5], b[5, 5]) and abs(a[5, 5, 0] - 400.0) < 1e-3
    one = denoise_robust_ref(film[5:6, 5:6], feat[5:6, 5:6], None, THETA, flags=CLAMP, firefly_clamp=1.0)   # a 1 x 1 image
    assert abs(one[0, 0, 0] - 400.0) < 1e-3


def test_options_layout_and_constants(pkg):
    assert C.sizeof(pkg.DenoiseOpts) == 32 and pkg.DenoiseOpts.flags.offset == 20 and pkg.DenoiseOpts.firefly_clamp.offset == 24
    assert [f[0] for f in pkg.DenoiseOpts._fields_][-3:] == ["flags", "firefly_clamp", "reserved"] and pkg.DenoiseOpts.reserved.size == 4
    assert (pkg.DENOISE_SPLIT_EMISSION, pkg.DENOISE_CLAMP_FIREFLIES) == (SPLIT, CLAMP) == (1, 2)
    header = open(os.path.join(kit.ROOT, "include", "mcpt.h")).read()
    assert re.search(r"#define\s+MCPT_DENOISE_SPLIT_EMISSION\s+0x1u", header) and re.search(r"#define\s+MCPT_DENOISE_CLAMP_FIREFLIES\s+0x2u", header)
    assert float(re.search(r"#define\s+MCPT_DENOISE_DEFAULT_FIREFLY_CLAMP\s+([0-9.]+)f", header).group(1)) == DEFAULT_FIREFLY_CLAMP
    kit.assert_exports(pkg, ["mcpt_read_emission"], ["emission"])
    assert pkg.load_library().mcpt_read_emission(None, np.zeros(4, np.float32).ctypes.data_as(C.c_void_p)) == 1


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _scene(pkg, which, size=None):
    if which == "cornell":
        return pkg.scenes.cornell_box_small(*(size or (96, 80)))
    return pkg.scenes.veach_mis(*(size or (80, 45)))


def _emission_from_probes(r, scene, spp, seed):
    """The emission buffer composed from the function-level probes: rng -> cast_ray -> binary-tree closest hit -> the material's radiance."""
    h, w = scene.camera.height, scene.camera.width
    pix = np.arange(h * w, dtype=np.uint32)
    rad = np.array([m.radiance for m in scene.materials], np.float32)
    emit = np.array([np.linalg.norm(m.radiance) > 1e-4 for m in scene.materials])
    e = np.zeros((h * w, 3), np.float32); hits = np.zeros(h * w)
    for s in range(spp):
        keys = np.stack([pix, np.full_like(pix, s), np.zeros_like(pix)], 1)
        xi = r.probe_rng(keys, seed=seed)[:, :2]
        ray = r.probe_cast_ray(np.stack([pix % w, pix // w], 1).astype(np.int32), xi)
        o = np.tile(np.asarray(scene.camera.eye, np.float64), (h * w, 1))
        t, tri, u, v = r.probe_trace(o, ray[:, 3:6].astype(np.float64))
        mat = scene.face[np.maximum(tri, 0), 0, 3]
        lit = (tri >= 0) & emit[mat]
        e[lit] += rad[mat[lit]]; hits += lit
    return np.concatenate([e / np.float32(spp), (hits / spp)[:, None]], 1).reshape(h, w, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cornell", "veach"])
def test_emission_equals_the_probes(pkg, which):
    scene = _scene(pkg, which, (64, 64) if which == "cornell" else None)
    r = pkg.Renderer(scene, max_depth=4)
    r.render(4, seed=7); r.render_features(spp=4, seed=7)
    feat = r.features()
    r.denoise(iterations=1, split_emission=True)
    got = r.emission()
    assert np.array_equal(r.features(), feat)                               # the lazy emission pass leaves the features alone
    want = _emission_from_probes(r, scene, 4, 7)
    r.close()
    share = float(np.mean(got[..., 3] > 0))
    print("[emission] %s: %.2f %% of the pixels see a light" % (which, 100 * share))
    assert 0.01 < share < 0.50
    assert np.array_equal(got[..., 3] > 0, got[..., :3].max(-1) > 0)
    assert got.shape == want.shape and _close_frac(got, want, 1e-5) >= 0.999
    assert np.all(got[..., 3] + feat[..., 3] <= 1.0 + 1e-6)                  # a sample is a surface hit, an emitter hit or a miss


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cornell", "veach"])
def test_lazy_and_same_pass_emission_are_bit_equal(pkg, which):
    scene = _scene(pkg, which)
    r = pkg.Renderer(scene, max_depth=4)
    r.render(2, seed=3)
    r.render_features(spp=5, seed=9)
    f_before = r.features()
    r.denoise(iterations=1, split_emission=True)                            # allocates the buffer and fills it lazily
    lazy = r.emission()
    r.render_features(spp=5, seed=9)                                        # the context owns the buffer: filled in the same traversal
    same = r.emission()
    f_after = r.features()
    r.render_features(spp=3, seed=9)
    other = r.emission()
    r.close()
    assert lazy[..., 3].max() > 0
    assert np.array_equal(kit.bits(lazy), kit.bits(same))
    assert np.array_equal(kit.bits(f_before), kit.bits(f_after))           # the 8 feature floats do not depend on the emission output
    assert not np.array_equal(other, same)


_STATE = {}


def _rendered(pkg, which):
    """(scene, renderer, film, features, emission) of a 4-spp film with its own features, rendered once per scene and left unchanged."""
    if which not in _STATE:
        scene = _scene(pkg, which)
        r = pkg.Renderer(scene, max_depth=8)
        r.render(4, seed=7); r.render_features(spp=4, seed=7)
        r.denoise(iterations=1, split_emission=True)
        _STATE[which] = (scene, r, r.read_accum(), r.features(), r.emission())
    return _STATE[which]


@pytest.fixture(scope="module", autouse=True)
def _close_renderers():
    yield
    for s in _STATE.values():
        s[1].close()
    _STATE.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("flags", sorted(FLAGS))
@pytest.mark.parametrize("which", ["cornell", "veach"])
def test_kernel_matches_the_restatement(pkg, which, flags, iterations):
    scene, r, film, feat, emis = _rendered(pkg, which)
    out = r.denoise(iterations=iterations, **_kw(FLAGS[flags]))
    ref = denoise_robust_ref(film, feat, emis, pixel_angle(scene.camera), flags=FLAGS[flags], iterations=iterations)
    _assert_matches_ref(out, ref)
    plain = denoise_ref(film, feat, pixel_angle(scene.camera), iterations=iterations)
    assert np.abs(ref - plain).max() > 1e-2                                 # (the flag did something on this film)


@pytest.mark.gpu
def test_kernel_matches_the_restatement_with_other_sigmas_and_clamp(pkg):
    scene, r, film, feat, emis = _rendered(pkg, "veach")
    kw = dict(iterations=4, sigma_color=2.0, sigma_normal=32.0, sigma_depth=1.0, firefly_clamp=3.0)
    out = r.denoise(**kw, **_kw(SPLIT | CLAMP))
    _assert_matches_ref(out, denoise_robust_ref(film, feat, emis, pixel_angle(scene.camera), flags=SPLIT | CLAMP, **kw))
    other = r.denoise(**dict(kw, firefly_clamp=1.0), **_kw(SPLIT | CLAMP))
    assert np.abs(other - out).max() > 1e-3                                 # firefly_clamp is read


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (2, 9), (63, 3), (65, 5), (130, 7)])
def test_kernel_matches_the_restatement_across_block_and_halo_edges(pkg, size):
    scene = pkg.scenes.cornell_box_small(*size)
    r = pkg.Renderer(scene, max_depth=8)
    r.render(4, seed=7); r.render_features(spp=4, seed=7)
    film, feat = r.read_accum(), r.features()
    outs = {name: r.denoise(**_kw(f)) for name, f in sorted(FLAGS.items(), reverse=True)}     # "split" first: the emission is held afterwards
    emis = r.emission()
    r.close()
    for name, f in FLAGS.items():
        _assert_matches_ref(outs[name], denoise_robust_ref(film, feat, emis, pixel_angle(scene.camera), flags=f))


@pytest.mark.gpu
def test_half_empty_film_and_device_pointer(pkg):
    scene = pkg.scenes.cornell_box_small(64, 48)
    r = pkg.Renderer(scene, max_depth=8)
    r.render_tiles(4, 7, 0, 2, 0)                                           # every other 8x8 tile: the rest of the film has count 0
    r.render_features(spp=4, seed=7)
    film, feat = r.read_accum(), r.features()
    out = r.denoise(**_kw(SPLIT | CLAMP))
    emis = r.emission()
    empty = film[..., 3] == 0
    assert 0.3 < empty.mean() < 0.7 and np.all(out[empty] == 0)
    ref = denoise_robust_ref(film, feat, emis, pixel_angle(scene.camera), flags=SPLIT | CLAMP)
    _assert_matches_ref(out, ref)
    import torch
    t = torch.from_numpy(film.copy()).cuda()
    torch.cuda.synchronize()
    r.clear()                                                               # the context film is empty now: only the pointer's film can give `ref`
    via_ptr = r.denoise(device_ptr=t.data_ptr(), **_kw(SPLIT | CLAMP))
    r.close()
    assert np.array_equal(kit.bits(via_ptr), kit.bits(out))


@pytest.mark.gpu
def test_emission_is_dropped_and_rendered_again(pkg):
    scene, r = kit.cornell(pkg, dynamic=True)
    buf = np.zeros((scene.camera.height, scene.camera.width, 4), np.float32)
    r.render(2, seed=5); r.render_features(spp=4, seed=5)
    assert r.lib.mcpt_read_emission(r.ctx, buf.ctypes.data_as(C.c_void_p)) == 1          # nobody asked for the split yet
    r.denoise(split_emission=True)
    old = r.emission()
    assert old[..., :3].max() > 0
    mats = [dataclasses.replace(m, radiance=tuple(2.0 * x for x in m.radiance)) for m in scene.materials]
    r.update_materials(mats)
    assert r.lib.mcpt_read_emission(r.ctx, buf.ctypes.data_as(C.c_void_p)) == 1          # dropped with the features
    r.render_features(spp=4, seed=5)
    r.denoise(split_emission=True)
    assert np.array_equal(r.emission(), old * np.float32([2, 2, 2, 1]))
    r.set_camera(scene.camera)
    assert r.lib.mcpt_read_emission(r.ctx, buf.ctypes.data_as(C.c_void_p)) == 1
    with pytest.raises(pkg.McptError):
        r.emission()
    with pytest.raises(pkg.McptError):
        r.denoise(split_emission=True)                                      # no features either
    # a reprojection call renders features itself: the context owns the buffer, so the emission of the new view comes with them
    r.render_features(spp=4, seed=5)
    r.reproject_camera(scene.camera, feature_spp=4, feature_seed=5)
    assert np.array_equal(r.emission(), old * np.float32([2, 2, 2, 1]))
    r.close()


@pytest.mark.gpu
def test_emission_buffer_is_counted_in_device_bytes(pkg):
    scene = pkg.scenes.cornell_box_small(40, 30)
    n = 40 * 30
    r = pkg.Renderer(scene, max_depth=2)
    r.render(1, seed=1)
    b0 = r.info().device_bytes
    r.render_features(spp=2, seed=1)
    assert r.info().device_bytes - b0 == n * 32                             # a context that never asked: the features alone
    r.denoise(clamp_fireflies=True)
    b1 = r.info().device_bytes
    r.render_features(spp=2, seed=1); r.denoise(); r.denoise(clamp_fireflies=True, firefly_clamp=4.0)
    assert r.info().device_bytes == b1                                      # never asked: nothing added
    r.denoise(split_emission=True)
    b2 = r.info().device_bytes
    assert b2 - b1 == n * 16
    r.render_features(spp=3, seed=2); r.denoise(split_emission=True, clamp_fireflies=True); r.denoise()
    assert r.info().device_bytes == b2
    clone = r.clone(0)
    clone.render(1, seed=1)
    c0 = clone.info().device_bytes
    clone.render_features(spp=2, seed=1)
    assert clone.info().device_bytes - c0 == n * 32                         # a clone starts without the buffer ...
    with pytest.raises(pkg.McptError):
        clone.emission()                                                    # ... and without an emission
    clone.close(); r.close()


@pytest.mark.gpu
def test_refusals_change_nothing(pkg):
    r = pkg.Renderer(pkg.scenes.cornell_box_small(16, 16), max_depth=2)
    r.render(1, seed=1)

    def status(**fields):
        o = pkg.DenoiseOpts(); o.struct_size = C.sizeof(pkg.DenoiseOpts)
        for k, v in fields.items():
            setattr(o, k, v)
        return r.lib.mcpt_denoise(r.ctx, None, C.byref(o))

    # the options are checked before "no features": the message names the option
    assert status(flags=0x4) == 1 and b"flags" in r.lib.mcpt_last_error()
    assert status(flags=SPLIT, firefly_clamp=0.5) == 1 and b"firefly_clamp" in r.lib.mcpt_last_error()
    assert status(flags=SPLIT) == 1 and b"no features" in r.lib.mcpt_last_error()
    r.render_features(spp=2, seed=1)
    want = r.denoise()
    b = r.info().device_bytes
    for bad in (dict(flags=0x4), dict(flags=0x80000001), dict(flags=CLAMP, firefly_clamp=-1.0), dict(flags=CLAMP, firefly_clamp=0.5),
                dict(flags=CLAMP, firefly_clamp=float("nan")), dict(flags=SPLIT | CLAMP, firefly_clamp=float("inf")), dict(firefly_clamp=0.5)):
        assert status(**bad) == 1, bad
    assert r.lib.mcpt_read_emission(r.ctx, None) == 1
    assert r.info().device_bytes == b                                       # a refused split allocates nothing
    out = np.zeros((16, 16, 4), np.float32)
    assert r.lib.mcpt_read_denoised(r.ctx, out.ctypes.data_as(C.c_void_p)) == 0 and np.array_equal(out, want)
    with pytest.raises(pkg.McptError):
        r.emission()
    assert status(flags=SPLIT | CLAMP, firefly_clamp=1.0) == 0
    assert r.lib.mcpt_read_emission(r.ctx, None) == 1                       # NULL output, with an emission held
    r.close()


def _quality_both(pkg, scene, depth):
    """tests/test_denoise.py::_quality's protocol -- a 4-spp film against 4096 spp, raw 4 spp = 1 -- for the filter without the flags and with
    both, on the same film and features: {name: (RMSE ratio, mean shift)}."""
    r = pkg.Renderer(scene, max_depth=depth)
    r.render(4096, seed=99)
    ref = r.read_accum(); ref = ref[..., :3] / ref[..., 3:]
    r.clear()
    r.render(4, seed=7)
    raw = r.read_accum(); raw = raw[..., :3] / raw[..., 3:]
    r.render_features(spp=4, seed=7)
    den = {"old": r.denoise()[..., :3], "robust": r.denoise(split_emission=True, clamp_fireflies=True)[..., :3]}
    r.close()
    out = {}
    for name, d in den.items():
        out[name] = (float(np.sqrt(np.mean((d - ref) ** 2)) / np.sqrt(np.mean((raw - ref) ** 2))), float(d.mean() / raw.mean() - 1.0))
        print("[quality] %s %-6s RMSE ratio %.3f  mean shift %+.4f" % (scene.name, name, *out[name]))
    return out


@pytest.mark.gpu
def test_quality_cornell_is_not_worse(pkg):
    """S-cornell 256x256, depth 8, 4 spp against 4096 spp.  Measured on the MI355X: RMSE ratio 0.880 without the flags, 0.701 with both
    (default k = 4), mean -3.8 % and -3.2 %."""
    q = _quality_both(pkg, pkg.scenes.cornell_box(256, 256), 8)
    assert q["robust"][0] <= q["old"][0] and abs(q["robust"][1]) < 0.06


@pytest.mark.gpu
def test_quality_veach_is_better(pkg):
    """S-veach 320x180, unbounded depth, 4 spp against 4096 spp.  Measured on the MI355X: RMSE ratio 1.978 without the flags, 0.997 with
    both (default k = 4) -- no longer worse than the raw film --, mean -11.4 % and -3.3 %."""
    q = _quality_both(pkg, pkg.scenes.veach_mis(320, 180), 0)
    assert q["robust"][0] < q["old"][0] and abs(q["robust"][1]) < 0.15
    assert q["robust"][0] < 1.0                                             # better than the unfiltered film


@pytest.mark.gpu
def test_facade_robust_matches_the_restatement(pkg, tmp_path):
    exe = kit.build_facade("facade_denoise_robust.cpp", tmp_path)
    scene = pkg.scenes.cornell_box_small(48, 32)
    obj = scene.write(str(tmp_path / "scene"))
    outs = [str(tmp_path / n) for n in ("dev.rgb", "film.bin", "feat.bin", "emis.bin")]
    line = kit.run_facade(exe, [obj, "8", "6", "1.5"] + outs)
    assert line == ["48", "32", "8"]
    dev = np.fromfile(outs[0], np.uint8).reshape(32, 48, 3).astype(int)
    film = np.fromfile(outs[1], np.float32).reshape(32, 48, 4); feat = np.fromfile(outs[2], np.float32).reshape(32, 48, 8)
    emis = np.fromfile(outs[3], np.float32).reshape(32, 48, 4)
    assert np.all(film[..., 3] == 8) and emis[..., 3].max() > 0
    want = _tonemap(denoise_robust_ref(film, feat, emis, pixel_angle(scene.camera), flags=SPLIT | CLAMP, firefly_clamp=1.5))
    assert np.abs(dev - want).max() <= 1
    assert np.abs(_tonemap(denoise_ref(film, feat, pixel_angle(scene.camera))) - want).max() > 1       # (not the filter without the flags)


@pytest.mark.gpu
def test_cli_denoise_robust(pkg, tmp_path):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    imgs = {}
    for name, flag in (("plain", "--denoise"), ("robust", "--denoise-robust")):
        out = str(tmp_path / name)
        p = kit.run_cli([obj, "--spp", "4", "--batch", "2", "--depth", "6", flag, "--out", out])
        assert p.returncode == 0, p.stderr[-2000:]
        imgs[name] = open(out + "4_denoised.png", "rb").read()
    assert len(imgs["robust"]) > 100 and imgs["robust"] != imgs["plain"]
