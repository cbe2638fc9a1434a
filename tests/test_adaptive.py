"""Adaptive sampling: rendering an arbitrary tile list, the per-tile error estimate and its compaction (csrc/adaptive.hip), the
pass schedule of mcpt_render_adaptive, and its public surfaces.

CPU tests pin the C ABI surface and the numpy restatement (tests/adaptive_ref.py); GPU tests check the tile-list path against full renders,
the kernels against the restatement, the driver against tile-list renders of the same sample ranges, and the image quality against uniform
sampling at the same sample count.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import adaptive_ref as ar, kit
from tests.kit import bits

NEW_SYMBOLS = ["mcpt_render_tile_list", "mcpt_render_adaptive", "mcpt_read_tile_error", "mcpt_probe_tile_error"]
INVALID = 1


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_adaptive_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS)


def test_null_context_is_an_invalid_argument(pkg):
    lib = pkg.load_library()
    buf = np.zeros(64, np.float32); lst = np.zeros(4, np.uint32); n = C.c_uint32(0)
    bp = buf.ctypes.data_as(C.c_void_p); lp = lst.ctypes.data_as(C.c_void_p)
    assert lib.mcpt_render_tile_list(None, 1, 0, 0, lp, 1) == INVALID
    assert lib.mcpt_render_adaptive(None, 0, 0, None, None) == INVALID
    assert lib.mcpt_read_tile_error(None, bp) == INVALID
    assert lib.mcpt_probe_tile_error(None, bp, bp, 0.1, 16, bp, lp, C.byref(n)) == INVALID


def _film(h, w, mean, count):
    f = np.zeros((h, w, 4), np.float32)
    f[..., :3] = np.asarray(mean, np.float32) * np.float32(count); f[..., 3] = count
    return f


def test_ref_constant_films_have_no_error():
    for mean in (0.0, 0.3, (0.2, 0.5, 0.9), 4.0):
        E, c = ar.tile_error(_film(13, 21, mean, 8), _film(13, 21, mean, 8))
        assert E.shape == (2, 3) and np.all(E == 0) and np.all(c == 16)


def test_ref_hand_computed_tile():
    h = _film(8, 8, 0.25, 4); o = _film(8, 8, 0.25, 4)
    o[2, 5, :3] = np.float32(0.5625) * 4                                  # sqrt: 0.5 vs 0.75 on all three channels
    o[6, 1, 0] = 1.0 * 4                                                  # 0.5 vs 1 on one channel
    E, c = ar.tile_error(h, o)
    assert E[0, 0] == pytest.approx(0.75) and c[0, 0] == 8
    e = ar.pixel_error(h, o)
    assert e[2, 5] == pytest.approx(0.75) and e[6, 1] == pytest.approx(0.5) and np.count_nonzero(e) == 2
    assert list(ar.active_list(E, c, 0.75, 16)) == [0] and list(ar.active_list(E, c, 0.7500001, 16)) == []
    assert list(ar.active_list(E, c, 0.75, 8)) == []                     # at max_spp: capped, not active


def test_ref_clamps_above_one():
    h = _film(8, 8, 3.0, 2); o = _film(8, 8, 1.5, 6)                    # both display as white: no error
    E, _ = ar.tile_error(h, o)
    assert E[0, 0] == 0
    o = _film(8, 8, 0.25, 6)
    E, _ = ar.tile_error(h, o)
    assert E[0, 0] == pytest.approx(1.5)                                  # 3 x |1 - 0.5|


def test_ref_schedule():
    assert ar.schedule(16, 1024) == [(0, 16, 8), (16, 16, 8), (32, 32, 16), (64, 64, 32), (128, 128, 64), (256, 256, 128), (512, 512, 256)]
    assert ar.allowed_counts(16, 1024) == [16, 32, 64, 128, 256, 512, 1024]
    assert ar.schedule(16, 1000)[-1] == (512, 488, 244) and ar.allowed_counts(16, 1000) == [16, 32, 64, 128, 256, 512, 1000]
    assert ar.schedule(2, 3) == [(0, 2, 1), (2, 1, 0)]                    # the last pass has one sample: O only
    assert ar.pass_ranges(2, 3, 3) == ([(0, 1)], [(1, 1), (2, 1)])
    assert ar.pass_ranges(16, 1024, 32) == ([(0, 8), (16, 8)], [(8, 8), (24, 8)])
    assert ar.schedule(8, 8) == [(0, 8, 4)]


# ------------------------------------------------------------------------------------------------------------------------ GPU
W, H = 68, 52                                                             # 9 x 7 tiles, the last column and row partial


def _tile_mask(tiles, w=W, h=H):
    ty, tx = ar.tiles_shape(h, w)
    m = np.zeros((ty * 8, tx * 8), bool)
    for t in np.asarray(tiles).reshape(-1):
        y, x = divmod(int(t), tx)
        m[8 * y:8 * y + 8, 8 * x:8 * x + 8] = True
    return m[:h, :w]


def _n_tiles(w=W, h=H):
    ty, tx = ar.tiles_shape(h, w)
    return ty * tx


@pytest.mark.gpu
def test_tile_list_of_all_tiles_equals_render(pkg):
    scene = pkg.scenes.cornell_box_small(W, H)
    perm = np.random.default_rng(1).permutation(_n_tiles()).astype(np.uint32)
    for flags, spp in ((pkg.FLAG_DETERMINISTIC, 4), (0, 1)):             # spp 1 with default flags: the tiles split over the sub-pipelines
        a = pkg.Renderer(scene, max_depth=6, flags=flags); b = pkg.Renderer(scene, max_depth=6, flags=flags)
        a.render(spp, seed=3, first_sample=5)
        b.render_tile_list(spp, 3, 5, perm)
        fa, fb = a.read_accum(), b.read_accum()
        a.close(); b.close()
        assert np.all(fa[..., 3] == spp)
        assert np.array_equal(bits(fa), bits(fb)), flags


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["mis", "recursive", "mega"])
def test_tile_list_subset_equals_the_full_render(pkg, which, monkeypatch):
    scene = pkg.scenes.cornell_box_small(W, H)
    kw = dict(max_depth=5, flags=pkg.FLAG_DETERMINISTIC)
    if which == "recursive":
        kw["integrator"] = pkg.INTEGRATOR_RECURSIVE_NEE
    if which == "mega":                                                   # read in mcpt_create only
        monkeypatch.setenv("MCPT_PIPELINE", "mega")
    full = pkg.Renderer(scene, **kw); part = pkg.Renderer(scene, **kw)
    monkeypatch.delenv("MCPT_PIPELINE", raising=False)
    rng = np.random.default_rng(7)
    tiles = rng.choice(_n_tiles(), size=_n_tiles() // 3, replace=False).astype(np.uint32)
    tiles = np.concatenate([tiles, [np.uint32(_n_tiles() - 1)]]) if _n_tiles() - 1 not in tiles else tiles   # the corner tile: partial both ways
    full.render(3, seed=11, first_sample=2)
    part.render_tile_list(3, 11, 2, tiles)
    ff, fp = full.read_accum(), part.read_accum()
    full.close(); part.close()
    m = _tile_mask(tiles)
    assert np.array_equal(bits(ff[m]), bits(fp[m]))
    assert np.all(fp[~m] == 0) and np.all(fp[m][:, 3] == 3)


@pytest.mark.gpu
def test_a_list_that_grows_between_unsynchronised_calls(pkg):
    """The longer second list replaces the device list and its staging buffer while the first call may still be reading them: the pair equals the
    same two calls with a synchronisation between them, bit for bit.  24 x 16 pixels = six tiles, lists of two and then five, one sample."""
    w, h = 24, 16
    scene = pkg.scenes.cornell_box_small(w, h)
    first, second = np.asarray([4, 1], np.uint32), np.asarray([0, 1, 2, 3, 5], np.uint32)
    films = []
    for synchronised in (False, True):
        r = pkg.Renderer(scene, max_depth=4)
        r.render_tile_list(1, 9, 0, first)
        if synchronised:
            r.sync()
        r.render_tile_list(1, 9, 1, second)
        films.append(r.read_accum())
        r.close()
    assert np.array_equal(bits(films[0]), bits(films[1]))
    count = _tile_mask(first, w, h).astype(np.float32) + _tile_mask(second, w, h)      # each call sampled its own tiles, once
    assert np.array_equal(films[0][..., 3], count)


@pytest.mark.gpu
def test_bad_tile_lists_are_refused(pkg):
    r = pkg.Renderer(pkg.scenes.cornell_box_small(W, H), max_depth=4)
    prior = np.random.default_rng(2).uniform(0, 2, (H, W, 4)).astype(np.float32)
    r.write_accum(prior)
    for bad in ([0, 5, 5], [0, _n_tiles()], [2 ** 31]):
        with pytest.raises(pkg.McptError):
            r.render_tile_list(2, 0, 0, np.asarray(bad, np.uint32))
    assert r.lib.mcpt_render_tile_list(r.ctx, 2, 0, 0, None, 3) == INVALID
    assert r.lib.mcpt_render_tile_list(r.ctx, 2, 0, 0, None, 0) == 0       # nothing to do
    r.render_tile_list(2, 0, 0, np.zeros(0, np.uint32))
    assert np.array_equal(bits(r.read_accum()), bits(prior))
    r.close()


@pytest.mark.gpu
def test_adaptive_option_errors(pkg):
    r = pkg.Renderer(pkg.scenes.cornell_box_small(16, 16), max_depth=4)
    for kw in (dict(min_spp=3), dict(min_spp=2, max_spp=1), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold=-1.0)):
        with pytest.raises(pkg.McptError):
            r.render_adaptive(**kw)
    with pytest.raises(pkg.McptError):
        r.render_adaptive(first_sample=2 ** 32 - 8, min_spp=4, max_spp=16)
    with pytest.raises(pkg.McptError):
        r.tile_error()                                                    # no adaptive call yet
    o = pkg.AdaptiveOpts(); o.struct_size = 4
    assert r.lib.mcpt_render_adaptive(r.ctx, 0, 0, C.byref(o), None) == INVALID
    assert np.all(r.read_accum() == 0)
    r.close()


def _synthetic_halves(h, w, max_spp, rng):
    """H and O with per-tile uniform counts, means up to 1.5, some tiles at max_spp, and tiles whose error is exactly 0.75 or 1.5."""
    ty, tx = ar.tiles_shape(h, w)
    nH = np.repeat(np.repeat(rng.integers(1, 6, (ty, tx)), 8, 0), 8, 1)[:h, :w].astype(np.float32)
    nO = np.repeat(np.repeat(rng.integers(1, 6, (ty, tx)), 8, 0), 8, 1)[:h, :w].astype(np.float32)
    capped = np.zeros((ty, tx), bool); capped[0, 1] = capped[1, 2] = capped[ty - 1, tx - 1] = True
    cm = np.repeat(np.repeat(capped, 8, 0), 8, 1)[:h, :w]
    nH[cm] = max_spp // 2; nO[cm] = max_spp - max_spp // 2
    mh = rng.uniform(0, 1.5, (h, w, 3)).astype(np.float32); mo = rng.uniform(0, 1.5, (h, w, 3)).astype(np.float32)
    ties = {(1, 0): (0.25, 0.5625), (1, 1): (0.5625, 1.0), (0, 2): (0.25, 1.0), (ty - 1, 0): (1.0, 0.5625)}   # e = 0.75, 0.75, 1.5, 0.75
    for (y, x), (a, b) in ties.items():
        mh[8 * y:8 * y + 8, 8 * x:8 * x + 8] = a; mo[8 * y:8 * y + 8, 8 * x:8 * x + 8] = b
    Hf = np.concatenate([mh * nH[..., None], nH[..., None]], -1).astype(np.float32)
    Of = np.concatenate([mo * nO[..., None], nO[..., None]], -1).astype(np.float32)
    return Hf, Of, ties


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(68, 52), (8, 8), (150, 37)])
def test_probe_matches_the_reference(pkg, size):
    w, h = size
    r = pkg.Renderer(pkg.scenes.cornell_box_small(w, h), max_depth=2)
    rng = np.random.default_rng(w * h)
    max_spp = 16
    Hf, Of, ties = _synthetic_halves(h, w, max_spp, rng) if min(ar.tiles_shape(h, w)) >= 3 else (None, None, {})
    if Hf is None:
        Hf = _film(h, w, 0.25, 3); Of = _film(h, w, 0.5625, 5)
    E_ref, c_ref = ar.tile_error(Hf, Of)
    for thr in (0.75, 0.3, 1e-9, 5.0):
        err, lst = r.probe_tile_error(Hf, Of, thr, max_spp)
        assert np.abs(err - E_ref).max() <= 1e-6
        want = ar.active_list(E_ref, c_ref, thr, max_spp)
        assert np.array_equal(lst, want), thr
    for (y, x) in ties:
        assert E_ref[y, x] in (0.75, 1.5)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(264, 256), (520, 512), (1001, 799)])
def test_probe_matches_the_reference_at_the_second_level_of_the_scan(pkg, size):
    """Films large enough for the second level of the compaction (csrc/adaptive.hip): 1 056 tiles are 264 error blocks, two blocks of
    ad_scatter_kernel; 4 160 tiles are 1 040 error blocks, so every thread of ad_scan_kernel sums a run of per = 2 and most runs are empty;
    12 600 tiles give per = 4 with a partial last tile column and row.  Nothing is rendered: two caller films through mcpt_probe_tile_error.
    The thresholds: every tile active, none, about half -- the middle of the widest gap among the central tenth of the reference's sorted
    errors, so that no tile lies within the probe's 1e-6 of it --, and a pair of films whose only active tiles are tile 0, the last tile and
    the first tile of the second scan thread's run (tile 4 * per)."""
    w, h = size
    ty, tx = ar.tiles_shape(h, w)
    n_tiles = ty * tx; nb = (n_tiles + 3) // 4; per = (nb + 1023) // 1024
    assert (n_tiles, nb > 256, per) == {(264, 256): (1056, True, 1), (520, 512): (4160, True, 2), (1001, 799): (12600, True, 4)}[size]
    r = pkg.Renderer(pkg.scenes.cornell_box_small(w, h), max_depth=2)
    rng = np.random.default_rng(w * h)
    max_spp = 16
    Hf, Of, ties = _synthetic_halves(h, w, max_spp, rng)
    E_ref, c_ref = ar.tile_error(Hf, Of)
    flat = np.sort(E_ref.reshape(-1)); mid = flat[int(0.45 * n_tiles):int(0.55 * n_tiles)]
    k = int(np.argmax(np.diff(mid)))
    half = float(np.float32(0.5 * (mid[k] + mid[k + 1])))
    assert mid[k] + 1e-5 < half < mid[k + 1] - 1e-5
    for name, thr, cap, count in (("all", 0.0, 1000, n_tiles), ("none", 5.0, max_spp, 0), ("half", half, max_spp, None), ("ties", 0.75, max_spp, None)):
        err, lst = r.probe_tile_error(Hf, Of, thr, cap)
        print("%dx%d %s: max |err - ref| %.3g, %d of %d tiles active" % (w, h, name, np.abs(err - E_ref).max(), lst.size, n_tiles))
        assert np.abs(err - E_ref).max() <= 1e-6
        want = ar.active_list(E_ref, c_ref, thr, cap)
        assert count is None or want.size == count, name
        assert np.array_equal(lst, want), name
    assert 0.4 * n_tiles < ar.active_list(E_ref, c_ref, half, max_spp).size < 0.6 * n_tiles
    # the same film twice has no error anywhere; three tiles get one: the first, the last, and the first of scan thread 1's run
    three = [0, 4 * per, n_tiles - 1]
    Os = Hf.copy()
    for t in three:
        y, x = divmod(t, tx)
        Hs = Hf[8 * y:8 * y + 8, 8 * x:8 * x + 8]; Ot = Os[8 * y:8 * y + 8, 8 * x:8 * x + 8]    # (views: mean 0.25 against mean 1, e = 3 * 0.5)
        Hs[..., 3:] = 2.0; Hs[..., :3] = 0.5                                  # two samples each: never a capped tile
        Ot[..., 3:] = 2.0; Ot[..., :3] = 2.0
    E3, c3 = ar.tile_error(Hf, Os)
    err, lst = r.probe_tile_error(Hf, Os, 0.75, max_spp)
    assert np.abs(err - E3).max() <= 1e-6
    assert ar.active_list(E3, c3, 0.75, max_spp).tolist() == three and E3.reshape(-1)[three].tolist() == [1.5, 1.5, 1.5]
    assert lst.tolist() == three
    r.close()


def _adaptive_case(pkg):
    scene = pkg.scenes.cornell_box_small(W, H)
    fl = pkg.FLAG_DETERMINISTIC
    one = pkg.Renderer(scene, max_depth=8, flags=fl)
    one.render_adaptive(seed=5, first_sample=3, min_spp=8, max_spp=8)
    E0 = one.tile_error()
    one.close()
    thr = float(np.median(E0))
    r = pkg.Renderer(scene, max_depth=8, flags=fl)
    st = r.render_adaptive(seed=5, first_sample=3, min_spp=8, max_spp=64, threshold=thr)
    film, E = r.read_accum(), r.tile_error()
    r.close()
    return scene, thr, st, film, E, E0


@pytest.mark.gpu
def test_adaptive_consistency(pkg):
    scene, thr, st, film, E, E0 = _adaptive_case(pkg)
    cnt = film[..., 3]
    ty, tx = ar.tiles_shape(H, W)
    pad = np.full((ty * 8, tx * 8), np.nan); pad[:H, :W] = cnt
    blocks = pad.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty, tx, 64)
    c_t = np.nanmax(blocks, -1)
    assert np.all(np.nanmin(blocks, -1) == c_t)                           # uniform per tile
    allowed = ar.allowed_counts(8, 64)
    assert set(np.unique(c_t)) <= set(allowed)
    assert c_t.min() == 8 and c_t.max() == 64
    assert np.all(E[c_t < 64] < thr) and np.all(c_t[E >= thr] == 64)
    assert np.array_equal(E[c_t == 8], E0[c_t == 8])                    # pass 0's estimate is the final one there
    assert st.pixel_samples == int(cnt.sum())
    assert st.tiles_converged == int((E < thr).sum()) and st.tiles_capped == int((E >= thr).sum())
    assert st.passes == allowed.index(64) + 1


@pytest.mark.gpu
def test_adaptive_equals_tile_list_renders_of_its_ranges(pkg):
    scene, thr, st, film, E, _ = _adaptive_case(pkg)
    fl = pkg.FLAG_DETERMINISTIC
    c_t = film[::8, ::8, 3]
    ty, tx = c_t.shape
    for c in np.unique(c_t):
        tiles = np.flatnonzero(c_t.reshape(-1) == c).astype(np.uint32)
        r = pkg.Renderer(scene, max_depth=8, flags=fl)
        r.render_tile_list(int(c), 5, 3, tiles)
        f = r.read_accum(); r.close()
        m = _tile_mask(tiles)
        assert np.array_equal(f[m][:, 3], film[m][:, 3])
        np.testing.assert_allclose(film[m][:, :3], f[m][:, :3], rtol=1e-5, atol=1e-6)
    # the half films, rebuilt from the pass ranges: the reference error of what they hold is what the device reported
    rh = pkg.Renderer(scene, max_depth=8, flags=fl); ro = pkg.Renderer(scene, max_depth=8, flags=fl)
    for c, n, nh in ar.schedule(8, 64):
        tiles = np.flatnonzero(c_t.reshape(-1) > c).astype(np.uint32)
        if nh:
            rh.render_tile_list(nh, 5, 3 + c, tiles)
        ro.render_tile_list(n - nh, 5, 3 + c + nh, tiles)
    E_ref, _ = ar.tile_error(rh.read_accum(), ro.read_accum())
    rh.close(); ro.close()
    assert np.abs(E_ref - E).max() <= 1e-5


@pytest.mark.gpu
def test_adaptive_leaves_the_rest_alone(pkg):
    scene, thr, st, film, E, _ = _adaptive_case(pkg)
    fl = pkg.FLAG_DETERMINISTIC
    r = pkg.Renderer(scene, max_depth=8, flags=fl)
    prior = np.random.default_rng(4).uniform(0, 3, (H, W, 4)).astype(np.float32)
    prior[..., 3] = np.round(prior[..., 3] * 10)
    r.write_accum(prior)
    st2 = r.render_adaptive(seed=5, first_sample=3, min_spp=8, max_spp=64, threshold=thr)
    got = r.read_accum()
    assert st2.pixel_samples == st.pixel_samples and np.array_equal(r.tile_error(), E)
    np.testing.assert_allclose(got, prior + film, rtol=1e-6, atol=1e-5)
    # a uniform render afterwards is the same as on a fresh context
    r.clear()
    r.render(4, seed=9)
    fresh = pkg.Renderer(scene, max_depth=8, flags=fl)
    fresh.render(4, seed=9)
    assert np.array_equal(bits(r.read_accum()), bits(fresh.read_accum()))
    info = r.info(); info_fresh = fresh.info()
    assert info.device_bytes - info_fresh.device_bytes >= 32 * W * H      # the half films are counted
    clone = r.clone()
    with pytest.raises(pkg.McptError):
        clone.tile_error()                                                # a clone starts without the adaptive buffers
    clone.close(); r.close(); fresh.close()


def _quality(pkg, scene, depth):
    """(adaptive RMSE / uniform RMSE at the same sample count, adaptive mean / reference mean - 1, uniform spp) at the defaults, against
    4096 spp."""
    r = pkg.Renderer(scene, max_depth=depth)
    r.render(4096, seed=99)
    ref = r.read_accum()
    r.clear()
    st = r.render_adaptive(seed=7)
    ad = r.read_accum()
    n_px = scene.camera.width * scene.camera.height
    spp = int(round(st.pixel_samples / n_px))
    r.clear()
    r.render(spp, seed=7)
    un = r.read_accum()
    r.close()
    ratio = ar.display_rmse(ad, ref) / ar.display_rmse(un, ref)
    mean_ad = (ad[..., :3] / ad[..., 3:]).mean(); mean_ref = (ref[..., :3] / ref[..., 3:]).mean()
    print("[quality] %s  adaptive %.1f spp/pixel, %d passes  RMSE ratio %.3f  mean shift %+.4f" % (
        scene.name, st.pixel_samples / n_px, st.passes, ratio, mean_ad / mean_ref - 1))
    return ratio, float(mean_ad / mean_ref - 1), spp


@pytest.mark.gpu
def test_quality_cornell(pkg):
    """S-cornell 128x128, depth 8, defaults, against uniform sampling with the same total samples; 4096 spp as the reference.  Measured on
    the MI355X: 498.6 samples per pixel in 7 passes, display RMSE ratio 0.989, mean -0.07 % -- barely better than uniform."""
    ratio, shift, _ = _quality(pkg, pkg.scenes.cornell_box(128, 128), 8)
    assert ratio < 1.0 and abs(shift) < 0.01


@pytest.mark.gpu
def test_quality_veach(pkg):
    """S-veach 160x90, unbounded depth, defaults, against uniform sampling with the same total samples; 4096 spp as the reference.  Measured
    on the MI355X: 208.3 samples per pixel in 7 passes, display RMSE ratio 0.940, mean +0.75 %."""
    ratio, shift, _ = _quality(pkg, pkg.scenes.veach_mis(160, 90), 0)
    assert ratio < 1.0 and abs(shift) < 0.01


@pytest.mark.gpu
def test_facade_render_adaptive(pkg, tmp_path):
    exe = kit.build_facade("facade_adaptive.cpp", tmp_path)
    obj = pkg.scenes.cornell_box_small(44, 30).write(str(tmp_path / "scene"))
    outs = [str(tmp_path / n) for n in ("dev.bin", "scene.bin", "next.bin")]
    line = kit.run_facade(exe, [obj, "4", "32", "0.05"] + outs)
    w, h, passes, largest = int(line[0]), int(line[1]), int(line[2]), int(line[3])
    assert (w, h) == (44, 30) and passes >= 1
    dev = np.fromfile(outs[0], np.float32).reshape(h, w, 4); sc = np.fromfile(outs[1], np.float32).reshape(h, w, 4)
    assert np.array_equal(dev, sc)
    assert largest == dev[..., 3].max() and largest in ar.allowed_counts(4, 32)
    nxt = np.fromfile(outs[2], np.float32).reshape(h, w, 4)               # one uniform frame after it: counts + 1, samples not reused
    assert np.all(nxt[..., 3] == dev[..., 3] + 1)


@pytest.mark.gpu
def test_cli_adaptive_with_denoise(pkg, tmp_path):
    obj = pkg.scenes.cornell_box_small(40, 32).write(str(tmp_path / "scene"))
    out = str(tmp_path / "img")
    p = kit.run_cli([obj, "--spp", "32", "--adaptive", "0.05", "--min-spp", "4", "--depth", "6", "--denoise", "--out", out])
    assert p.returncode == 0, p.stderr[-2000:]
    assert "adaptive:" in p.stdout
    for name in ("img32.png", "img_spp.png", "img32_denoised.png"):              # (a uniform spp map compresses to under 100 bytes)
        with open(str(tmp_path / name), "rb") as f:
            assert f.read(8) == b"\x89PNG\r\n\x1a\n", name
    p = kit.run_cli([obj, "--spp", "32", "--adaptive", "0.05", "--gpus", "2", "--out", out])
    assert p.returncode == 2 and "--adaptive" in p.stderr
