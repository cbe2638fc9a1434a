"""-m gpu: the light-probe stage (csrc/shprobe.hip) through the C ABI -- every ray against the float64 restatement of
tests/shprobe_ref.py within S_BOUND, which tests/test_shprobe_ref.py derives on the CPU; the projection and its reduction tree against the fp32
restatement, bit for bit; that a pass's scratch film is made of exactly the rays the probe shows; the class bytes against a brute-force trace;
the lamp's analytic solid angle and form factor; the resolve; bookkeeping; live scenes; refusals; the C++ facade and mcpt_cli.

The device draws its own directions from rng_block(item, sample, 0): the tests read the numbers through probe_rng and hand them to the
restatement.  The scenes are open_box and copies of it; probe counts are 1, 3, 4, 5 and 17 (a partial block, exactly one block and more than
one block of the projection kernel at 4 probes per block), the analytic test's 1024 apart.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import bake_ref, kit, shprobe_ref as R
from tests.kit import bits

pytestmark = pytest.mark.gpu

SEED = 20281
INVALID, UNSUPPORTED = 1, 6
RADIANCE = np.array([17.0, 12.0, 4.0], np.float32)           # open_box's lamp
COUNTS = (1, 3, 4, 5, 17)
F32 = np.float32

# World positions in open_box's frame (the box is [0, 1]^3, open towards +z; the lamp is [0.35, 0.65]^2 at y = 0.999, facing down, 1 mm under
# the ceiling): the centre, a probe in the 1-mm gap ABOVE the lamp (every ray of its lower half first meets the lamp from behind; off both
# diagonals of the lamp's quad), one in front of the open side, one above the ceiling and one beside the green wall (outside: they see walls
# from behind and the sky), then twelve inside.  Checked on the CPU with directions of the same stratification: kit.brute_force_trace in fp64 and
# in fp32 name the same face for every one of 1088 rays, and 1 of them falls under the three "unsure" criteria.
PROBES = np.array([[0.5, 0.5, 0.5], [0.45, 0.9993, 0.56], [0.5, 0.5, 1.6], [0.5, 1.2, 0.5], [1.3, 0.5, 0.5], [0.64, 0.15, 0.54], [0.32, 0.80, 0.15], [0.64, 0.80, 0.28],
                   [0.82, 0.80, 0.11], [0.67, 0.10, 0.50], [0.45, 0.26, 0.36], [0.74, 0.35, 0.22], [0.66, 0.46, 0.74], [0.29, 0.36, 0.74], [0.51, 0.51, 0.29],
                   [0.11, 0.85, 0.17], [0.25, 0.65, 0.9]], np.float64)


def _xi(r, first, n, sample, seed):
    """Block 0's first two numbers of items first .. first + n - 1 for (sample, seed), from the generator itself."""
    key = np.stack([np.arange(first, first + n), np.full(n, sample), np.zeros(n, np.int64)], 1)
    return r.probe_rng(key.astype(np.uint32), seed)[:, :2]


def _centred_box(pkg, black=False):
    """open_box moved so that the centre every device coordinate is relative to is exactly 0 (section 25's copy): (o + centre) - centre is then o
    itself and probe_paths starts from the very origins the stage wrote.  black: every non-emissive material with kd = ks = 0.  Returns the
    scene and the shift (world positions of open_box's frame less the shift are positions of this scene)."""
    s = pkg.scenes.open_box(16, 16)
    used = s.vertex[np.unique(s.face[:, :, 0])]
    shift = 0.5 * used.min(0) + 0.5 * used.max(0)
    out = kit.with_arrays(pkg, s, vertex=s.vertex - shift)
    if black:
        out.materials = [m if any(m.radiance) else pkg.scenes.Material(m.name) for m in s.materials]
    return out, shift


def _lamp_faces(scene):
    return np.flatnonzero(np.array([any(scene.materials[m].radiance) for m in scene.face[:, 0, 3]]))


def _verdicts(scene, o, d, centre):
    """kit.brute_force_trace's verdict per ray: (class 0 miss / 1 front / 2 back, first meets the lamp from behind, unsure) -- unsure by
    test_known_answer_per_item's three criteria: fp64 and fp32 arithmetic name different faces, the hit lies within 1e-4 of the winning face's
    edge, or a second face lies within 1e-4 (relative) behind the first."""
    t64, f64, u64, v64 = kit.brute_force_trace(scene, o + centre, d, centre=centre)
    t32, f32, _, _ = kit.brute_force_trace(scene, o + centre, d, dtype=np.float32, centre=centre)
    t2nd, _, _, _ = kit.brute_force_trace(scene, o + centre + d * (np.where(f64 >= 0, t64, 0.0) * (1 + 1e-4))[:, None], d, t1=0.0, centre=centre)
    hit = f64 >= 0
    unsure = (f64 != f32) | (hit & (np.minimum(np.minimum(u64, v64), 1 - u64 - v64) < 1e-4)) | (hit & np.isfinite(t2nd) & (t2nd < 2e-4 * np.where(hit, t64, 1.0)))
    nl = scene.normal[scene.face[np.where(hit, f64, 0)][:, 0, 1]]
    front = (d * nl).sum(1) < 0
    cls = np.where(hit, np.where(front, 1, 2), 0).astype(np.uint8)
    return cls, hit & np.isin(f64, _lamp_faces(scene)) & ~front, unsure


def _check_rays(r, world, sample, seed, first=0, n=None):
    """probe_sh_rays against the restatement: origins equal world - centre, every direction within S_BOUND and in its slot's cell."""
    total = 64 * len(world)
    n = total - first if n is None else n
    o, d = r.probe_sh_rays(sample, seed, first, n)
    item = np.arange(first, first + n)
    centre = np.array(r.info().centre)
    assert np.array_equal(bits(o), bits((world - centre[None])[item >> 6]))
    assert np.array_equal(d, d.astype(F32).astype(np.float64))                   # the doubles hold fp32 values
    ref = R.rays(item & 63, _xi(r, first, n, sample, seed))
    ratio = R.dir_ratio(d, ref)
    bad = np.flatnonzero(~(ratio <= 1.0))
    assert bad.size == 0, "%d of %d rays beyond S_BOUND, first: item %d, ratio %.3g" % (bad.size, n, first + bad[0], ratio[bad[0]])
    # the cell: z between the borders of band jx (fp32 numbers: rounding cannot cross them); the azimuth between the borders of sector jy, up to the
    # fp32 rounding of x and y -- a border direction b = (cos, sin), cross(b, (x, y)) moves by at most 2^-24 (|x| + |y|) under it -- and the float64 slack
    # (S_BOUND 2^-52 (1 + |x|) per component: under 1e-14)
    jx = (item & 7).astype(np.float64); jy = ((item & 63) >> 3).astype(np.float64)
    assert (d[:, 2] >= 1 - 2 * (jx + 1) / 8).all() and (d[:, 2] <= 1 - 2 * jx / 8).all()
    tol = 2.0 ** -24 * (np.abs(d[:, 0]) + np.abs(d[:, 1])) + 1e-14
    for a, sign in ((2 * np.pi * jy / 8, 1.0), (2 * np.pi * (jy + 1) / 8, -1.0)):
        assert (sign * (np.cos(a) * d[:, 1] - np.sin(a) * d[:, 0]) >= -tol).all()
    return float(ratio.max()), R.slack_used(d, ref), o, d


@pytest.mark.parametrize("count", COUNTS)
def test_rays_against_float64(pkg, count):
    """Every origin and direction of probe_sh_rays for samples 0, 1 and 7: origins equal to the host's world - centre, directions within S_BOUND
    units 2^-52 (1 + |x|) plus half an fp32 ulp of the restatement, none forgiven; every direction in its slot's cell; a sub-range of items
    equals the same rows of the whole, bit for bit."""
    r = pkg.Renderer(pkg.scenes.open_box(16, 16))
    world = PROBES[:count]
    r.set_sh_probes(world)
    for sample in (0, 1, 7):
        worst, used, o, d = _check_rays(r, world, sample, SEED)
        print("%d probes, sample %d: worst ratio %.3f of the bound, slack used beyond the half fp32 ulp %.2f of S_BOUND = %g" % (count, sample, worst, used, R.S_BOUND))
        first, m = (37, 64 * count - 50) if count > 1 else (5, 40)
        so, sd = r.probe_sh_rays(sample, SEED, first, m)
        assert np.array_equal(bits(so), bits(o[first:first + m])) and np.array_equal(bits(sd), bits(d[first:first + m]))
    r.close()


@pytest.mark.parametrize("count", COUNTS)
def test_the_projection_alone(pkg, count):
    """After bake_sh(1, seed, s) for s in (0, 3): read_sh_pass()'s film and probe_sh_rays' directions through the fp32 restatement give the
    accumulators' increase, all 27 per probe, bit for bit; the ray count is 64 x passes; the back and miss counts are the class bytes' counts;
    no accumulator is non-finite."""
    r = pkg.Renderer(pkg.scenes.open_box(16, 16), max_depth=4)
    r.set_sh_probes(PROBES[:count])
    acc, counts = r.read_sh_film()
    assert (acc == 0).all() and (counts == 0).all()
    for k, s in enumerate((0, 3)):
        r.bake_sh(1, SEED, s)
        film, cls = r.read_sh_pass()
        _, d = r.probe_sh_rays(s, SEED)
        assert (film[:, 3] == 1).all() and set(np.unique(cls)) <= {0, 1, 2}
        want = (acc + R.project(film, d)).astype(F32)
        got, got_counts = r.read_sh_film()
        assert np.isfinite(got).all()
        diff = bits(got) != bits(want)
        assert not diff.any(), "%d of %d accumulators differ, first %s: %s, wanted %s" % (diff.sum(), diff.size, np.argwhere(diff)[0], got[diff][0], want[diff][0])
        counts = counts + np.stack([np.full(count, 64), (cls.reshape(count, 64) == 2).sum(1), (cls.reshape(count, 64) == 0).sum(1)], 1).astype(np.uint32)
        assert np.array_equal(got_counts, counts) and (got_counts[:, 0] == 64 * (k + 1)).all()
        acc = got
    assert (np.abs(acc).max((1, 2)) > 0).all()                                     # (every probe sees light)
    if count > 2:
        assert counts[1, 1] >= 40 and counts[2, 2] >= 80                           # (the probe in the gap above the lamp; the one in front of the open side)
    r.close()


def _film_against_paths(r, scene, centre, seed):
    """One pass at sample 0 on a context whose centre is 0: the scratch film equals probe_paths started from the probed rays, bit for bit (NaN
    zeroed on both sides), but for rays that first meet the lamp from BEHIND, whose record is float32(-Le) + probe_paths' L.  Returns the
    number of those."""
    assert np.array_equal(centre, np.zeros(3))
    o, d = r.probe_sh_rays(0, seed)
    assert np.array_equal(bits(o), bits((o + centre) - centre))
    want = r.probe_paths(o + centre, d, seed)
    _, behind, _ = _verdicts(scene, o, d, centre)
    want[behind] = -RADIANCE[None] + want[behind]
    want = np.nan_to_num(want, nan=0.0)
    assert want.dtype == np.float32
    r.bake_sh(1, seed, 0)
    film, cls = r.read_sh_pass()
    assert (film[:, 3] == 1).all()
    got = np.nan_to_num(film[:, :3], nan=0.0)
    diff = (bits(got + F32(0)) != bits(want + F32(0))).any(1)                      # (+ 0: a -0 sum is a 0)
    assert not diff.any(), "%d of %d items differ, first %d: film %s, probe %s" % (diff.sum(), len(diff), np.flatnonzero(diff)[0], got[diff][0], want[diff][0])
    assert (got != 0).any(1).mean() > 0.3
    return int(behind.sum())


def test_the_pass_film_is_made_of_the_probed_rays(pkg):
    """On the centred open_box with max_depth 4, at sample 0: the pass film equals probe_paths(o + centre, d, seed) bit for bit with count 1
    everywhere; the rays kit.brute_force_trace shows first meeting the lamp from behind -- the lower half of the probe in the 1-mm gap above the
    lamp -- are float32(-Le) + L instead: probe_paths treats them as camera rays, which see a lamp's back lit, and the stage takes exactly that
    radiance out beforehand."""
    scene, shift = _centred_box(pkg)
    r = pkg.Renderer(scene, max_depth=4)
    r.set_sh_probes(PROBES - shift[None])
    behind = _film_against_paths(r, scene, np.array(r.info().centre), SEED)
    print("%d of %d rays first meet the lamp from behind" % (behind, 64 * len(PROBES)))
    assert behind >= 16
    r.close()


def test_classes_against_brute_force(pkg):
    """The class byte of every item of a pass (miss, front, back) equals kit.brute_force_trace's verdict for every item the brute force can
    decide; at most 1 % are left out."""
    scene, shift = _centred_box(pkg)
    r = pkg.Renderer(scene, max_depth=2)
    r.set_sh_probes(PROBES - shift[None])
    for sample in (0, 5):
        r.bake_sh(1, SEED, sample)
        _, cls = r.read_sh_pass()
        o, d = r.probe_sh_rays(sample, SEED)
        want, behind, unsure = _verdicts(scene, o, d, np.array(r.info().centre))
        print("sample %d: left out %d of %d items (%.3f %%); classes %s" % (sample, unsure.sum(), len(cls), 100.0 * unsure.mean(), np.bincount(cls, minlength=3)))
        assert unsure.mean() <= 0.01
        bad = ~unsure & (cls != want)
        assert not bad.any(), "%d items differ, first %d: class %d, wanted %d" % (bad.sum(), np.flatnonzero(bad)[0], cls[bad][0], want[bad][0])
        assert (np.bincount(cls, minlength=3) > 30).all()
    r.close()


def test_known_answer_analytic(pkg):
    """The one larger shape: 1024 probes, all at the centre of the black-walled box, one pass, N = 65 536 rays.  L is Le on the lamp's front and 0
    elsewhere, so with Omega the lamp's solid angle from the point (the rectangle [0.35, 0.65]^2 at height h = 0.499: 4 atan(a b / (h sqrt(a^2 + b^2
    + h^2)))), p = Omega / 4 pi and F the point-to-rectangle form factor: the mean over probes of c0 / (Y0 Le) is within 5 x 4 pi sqrt(p (1 - p) / N)
    of Omega, that of the y coefficient c1 / (0.4886025 Le) within 5 x 4 pi sqrt(p / N) of pi F, and the x and z coefficients within the same
    bound of 0 -- the unstratified binomial bounds; stratification only lowers the variance."""
    scene, shift = _centred_box(pkg, black=True)
    r = pkg.Renderer(scene, max_depth=4)
    n = 1024; N = 64 * n
    r.set_sh_probes(np.tile(np.array([0.5, 0.5, 0.5]) - shift, (n, 1)))
    r.bake_sh(1, SEED, 0)
    film, cls = r.read_sh_pass()
    seen = (film[:, :3] == RADIANCE[None]).all(1)
    assert (seen | (film[:, :3] == 0).all(1)).all() and (film[:, 3] == 1).all()
    c = r.read_sh(pkg.SH_RADIANCE).astype(np.float64)
    a = b = 0.15; h = 0.499
    omega = 4.0 * math.atan(a * b / (h * math.sqrt(a * a + b * b + h * h)))
    F = bake_ref.form_factor_rect(-a, a, -b, b, h)
    p = omega / (4 * math.pi)
    tol0 = 5 * 4 * math.pi * math.sqrt(p * (1 - p) / N); tol1 = 5 * 4 * math.pi * math.sqrt(p / N)
    for ch in range(3):
        le = float(RADIANCE[ch])
        m0 = c[:, ch, 0].mean() / (0.28209479177387814 * le)
        my, mz, mx = (c[:, ch, k].mean() / (0.4886025119029199 * le) for k in (1, 2, 3))
        print("channel %d: Omega %.6f, measured %.6f (off %.2e, allowed %.2e); pi F %.6f, measured %.6f (off %.2e, allowed %.2e); x %.2e, z %.2e" % (
            ch, omega, m0, m0 - omega, tol0, math.pi * F, my, my - math.pi * F, tol1, mx, mz))
        assert abs(m0 - omega) <= tol0
        assert abs(my - math.pi * F) <= tol1
        assert abs(mx) <= tol1 and abs(mz) <= tol1
    assert abs(seen.mean() - p) <= 5 * math.sqrt(p * (1 - p) / N)
    # the irradiance a small surface at the point receives, facing up: E = pi F Le, within the two bounds' share of it
    E = pkg.sh_eval(r.read_sh(pkg.SH_IRRADIANCE), [0.0, 1.0, 0.0]).mean(0)
    print("E(+y) = %s, analytic pi F Le = %s (three bands of a small lamp: not a check)" % (E, math.pi * F * RADIANCE))
    r.close()


@pytest.mark.parametrize("count", (1, 5))
def test_resolve(pkg, count):
    """read_sh(SH_RADIANCE) equals resolve() of the raw film, bit for bit, after 1 and after 3 passes; SH_IRRADIANCE equals it times the three
    fp32 band factors, bit for bit; everything is 0 before the first pass."""
    r = pkg.Renderer(pkg.scenes.open_box(16, 16), max_depth=4)
    r.set_sh_probes(PROBES[:count])
    assert (r.read_sh(pkg.SH_RADIANCE) == 0).all() and (r.read_sh(pkg.SH_IRRADIANCE) == 0).all()
    for passes in (1, 2):
        r.bake_sh(passes, SEED, 10)
        acc, counts = r.read_sh_film()
        rad = r.read_sh(pkg.SH_RADIANCE); irr = r.read_sh(pkg.SH_IRRADIANCE)
        assert np.array_equal(bits(rad), bits(R.resolve(acc, counts[:, 0])))
        assert np.array_equal(bits(irr), bits((R.BAND_FACTOR[R.BAND][None, None] * rad).astype(F32))) and np.array_equal(bits(irr), bits(R.resolve(acc, counts[:, 0], True)))
        assert (rad[0, :, 0] > 0).all() and (rad[:, :, 0] != 0).all()           # (the centre probe; elsewhere a path's L may be negative: the pipeline's own)
    assert (counts[:, 0] == 192).all()
    r.close()


def test_bookkeeping(pkg):
    """Three single passes of samples 0, 1, 2 equal one call of three, bit for bit; another sample gives other bits; clear_sh zeroes accumulators
    and counts; sh_info counts bakes and passes; device_bytes rises by 144 B per probe at set_sh_probes and by 64 x 65 B per probe more at the
    first bake, and returns to its old value after set_sh_probes(None); a clone has no probes."""
    r = pkg.Renderer(pkg.scenes.open_box(16, 16), max_depth=4)
    n = 5
    # the pools of a 64 n-item probe job exist after this; drop everything again: from here on device_bytes moves by the probes' buffers alone
    r.set_sh_probes(PROBES[:n]); r.bake_sh(1, SEED, 0); r.set_sh_probes(None)
    assert r.sh_info().n_probes == 0 and r.sh_info().device_bytes == 0 and r.read_sh().shape == (0, 3, 9)
    bytes0 = r.info().device_bytes
    r.set_sh_probes(PROBES[:n])
    assert r.info().device_bytes == bytes0 + 144 * n and r.sh_info().device_bytes == 144 * n
    r.bake_sh(0, SEED, 0)                                                        # passes = 0 does nothing
    assert r.info().device_bytes == bytes0 + 144 * n and r.sh_info().bakes == 1
    for s in (0, 1, 2):
        r.bake_sh(1, SEED, s)
    assert r.info().device_bytes == bytes0 + (144 + 64 * 65) * n and r.sh_info().device_bytes == (144 + 64 * 65) * n
    single = r.read_sh_film()
    r.clear_sh()
    zero = r.read_sh_film()
    assert (zero[0] == 0).all() and (zero[1] == 0).all()
    launches = r.counters().launches; paths = r.counters().paths
    r.bake_sh(3, SEED, 0)
    assert r.counters().launches == launches + 1 and r.counters().paths == paths + 3 * 64 * n
    three = r.read_sh_film()
    assert np.array_equal(bits(single[0]), bits(three[0])) and np.array_equal(single[1], three[1]) and (three[1][:, 0] == 192).all()
    r.clear_sh(); r.bake_sh(3, SEED, 1)
    assert not np.array_equal(bits(r.read_sh_film()[0]), bits(three[0]))
    i = r.sh_info()
    assert (i.n_probes, i.bakes, i.passes) == (n, 6, 10) and i.last_stage_ms > 0 and i.struct_size == 56
    k = r.clone()
    assert k.sh_info().n_probes == 0 and k.sh_info().device_bytes == 0
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_bake_sh: no probes" % INVALID):
        k.bake_sh(1, SEED, 0)
    k.close()
    r.set_sh_probes(PROBES[:3])                                                  # a list of another length drops the per-item buffers until its first bake
    assert r.info().device_bytes == bytes0 + 144 * 3 and (r.read_sh_film()[0] == 0).all()
    r.set_sh_probes(None)
    assert r.info().device_bytes == bytes0
    r.close()


def test_live_scene(pkg):
    """A FLAG_DYNAMIC context on the centred box: after update_vertices (the lamp lowered and shifted, which keeps the bounding box) the pass
    film is again made of the probed rays, traced through the scene as it is NOW; after rebuild() the probes and accumulators are as before and
    the next pass still adds project(its film, its rays), so the origins followed the centre; the render film, the bake points and the bake
    film are bit for bit what they were before any of the probe calls (compared before the update, which moves the lamp's bake point)."""
    scene, shift = _centred_box(pkg)
    r = pkg.Renderer(scene, max_depth=4, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_DETERMINISTIC)
    centre = np.array(r.info().centre)
    pts = pkg.bake_points(np.arange(scene.face.shape[0]), F32(0.25), F32(0.5))
    r.set_bake_points(pts); r.bake(2, SEED, 0)
    before = (kit.render_film(r, 2, SEED), r.read_bake_film(), r.probe_bake_rays(0, SEED))
    world = PROBES - shift[None]
    r.set_sh_probes(world)
    assert _film_against_paths(r, scene, centre, SEED) >= 16
    r.read_sh(pkg.SH_IRRADIANCE); r.read_sh_pass(); r.sh_info(); r.clear_sh(); r.bake_sh(2, SEED, 3)
    after = (r.read_accum(), r.read_bake_film(), r.probe_bake_rays(0, SEED))
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1])) and r.bake_info().n_points == len(pts)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before[2], after[2]))
    r.clear_sh()
    lamp = _lamp_faces(scene)
    v = scene.vertex.copy()
    lv = np.unique(scene.face[lamp][:, :, 0])
    v[lv, 1] -= 0.2; v[lv, 0] += 0.05
    moved = kit.with_arrays(pkg, scene, v)
    assert all(np.array_equal(a, b) for a, b in zip(kit.used_bounds(scene), kit.used_bounds(moved)))
    r.update_vertices(v)
    r.clear_sh()
    behind = _film_against_paths(r, moved, centre, SEED)
    print("after the update: %d rays first meet the lamp from behind" % behind)
    assert behind >= 1                                                           # (the gap probe now looks down on the lowered lamp's back from 0.2 above)
    acc, counts = r.read_sh_film()
    o, d = r.probe_sh_rays(1, SEED)
    for builder in (pkg.REBUILD_DEVICE, pkg.REBUILD_HOST):
        r.rebuild(builder)
        again = r.read_sh_film()
        assert np.array_equal(bits(again[0]), bits(acc)) and np.array_equal(again[1], counts) and r.sh_info().n_probes == len(world)
        o2, d2 = r.probe_sh_rays(1, SEED)
        assert np.array_equal(bits(o2), bits(world - np.array(r.info().centre)[None]).repeat(64, 0)) and np.array_equal(bits(d2), bits(d))
        r.bake_sh(1, SEED, 1)
        film, cls = r.read_sh_pass()
        want = (acc + R.project(film, d2)).astype(F32)
        acc, counts = r.read_sh_film()
        assert np.array_equal(bits(acc), bits(want)) and (counts[:, 0] == again[1][:, 0] + 64).all()
        o, d = r.probe_sh_rays(1, SEED)
    assert np.array_equal(bits(r.read_bake_film()), bits(before[1])) and r.bake_info().n_points == len(pts)
    r.close()


def test_refusals(pkg):
    """Every refusal leaves probes, accumulators and device_bytes as they were: a NaN or infinite coordinate (the message names the probe),
    n = 1 048 576, a null list, bake_sh past 2^32 samples, an unknown read_sh mode, an item range past the end; bake_sh without probes and
    read_sh_pass before any pass are MCPT_ERR_INVALID_ARG; bake_sh on a recursive-integrator context is MCPT_ERR_UNSUPPORTED."""
    scene = pkg.scenes.open_box(16, 16)
    r = pkg.Renderer(scene, max_depth=4)
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_bake_sh: no probes" % INVALID):
        r.bake_sh(1, SEED, 0)
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_read_sh_pass" % INVALID):
        r.read_sh_pass()
    n = 5
    r.set_sh_probes(PROBES[:n])
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_read_sh_pass" % INVALID):
        r.read_sh_pass()
    r.bake_sh(2, SEED, 0)
    state = (r.read_sh_film(), r.read_sh_pass(), r.probe_sh_rays(0, SEED), r.info().device_bytes)
    for k, value in ((0, np.nan), (3, np.inf), (4, -np.inf)):
        bad = PROBES[:n].copy(); bad[k, k % 3] = value
        with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_set_sh_probes: probe %d:" % (INVALID, k)):
            r.set_sh_probes(bad)
    buf = np.ascontiguousarray(PROBES)
    assert r.lib.mcpt_set_sh_probes(r.ctx, buf.ctypes.data, 1048576) == INVALID and b"1 048 575" in r.lib.mcpt_last_error()
    assert r.lib.mcpt_set_sh_probes(r.ctx, None, 5) == INVALID
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_bake_sh: first_sample" % INVALID):
        r.bake_sh(2, SEED, 2 ** 32 - 1)
    out = np.zeros((n, 27), F32)
    assert r.lib.mcpt_read_sh(r.ctx, 2, out.ctypes.data) == INVALID and (out == 0).all()
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_probe_sh_rays" % INVALID):
        r.probe_sh_rays(0, SEED, 64 * n - 3, 4)
    r._n_sh = n
    now = (r.read_sh_film(), r.read_sh_pass(), r.probe_sh_rays(0, SEED), r.info().device_bytes)
    for a, b in zip(state[:3], now[:3]):
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
    assert state[3] == now[3] and r.sh_info().n_probes == n
    r.close()
    rec = pkg.Renderer(scene, max_depth=4, integrator=pkg.INTEGRATOR_RECURSIVE_NEE)
    rec.set_sh_probes(PROBES[:n])                                                # the probes are state of every context
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_bake_sh" % UNSUPPORTED):
        rec.bake_sh(1, SEED, 0)
    rec.close()


def test_facade_sh(pkg, tmp_path):
    """Render::set_sh_probes, bake_sh and read_sh through the host classes: the program sets 5 probes, bakes 2 passes in two calls and asserts
    the refusals itself; its coefficients are what the same calls give through the C ABI, bit for bit."""
    exe = kit.build_facade("facade_sh.cpp", tmp_path)
    scene = pkg.scenes.open_box(16, 16)
    obj = scene.write(str(tmp_path / "a"))
    out = str(tmp_path / "sh.bin")
    line = kit.run_facade(exe, [obj, out])
    assert int(line[0]) == 5
    got = np.fromfile(out, np.float32).reshape(2, 5, 3, 9)
    r = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DETERMINISTIC)
    r.set_sh_probes(PROBES[:5]); r.bake_sh(1, 17, 0); r.bake_sh(1, 17, 1)
    assert np.array_equal(bits(got[0]), bits(r.read_sh(pkg.SH_RADIANCE))) and np.array_equal(bits(got[1]), bits(r.read_sh(pkg.SH_IRRADIANCE)))
    assert (got[0][0, :, 0] > 0).all() and (got[0][:, :, 0] != 0).all()
    r.close()


def test_cli_sh_grid(pkg, tmp_path):
    """mcpt_cli --sh-grid 2 2 2 on open_box writes 8 lines of 31 numbers -- position, 27 coefficients, back-hit share in [0, 1] --, the positions
    the cell centres of the scene's bounds; --sh-irradiance gives other coefficients; the option's misuse is refused."""
    scene = pkg.scenes.open_box(16, 16)
    obj = scene.write(str(tmp_path / "scene"))
    rows = {}
    for name, extra in (("radiance", []), ("irradiance", ["--sh-irradiance"])):
        out = str(tmp_path / (name + ".txt"))
        p = kit.run_cli([obj, "--ref-index-order", "--sh-grid", "2", "2", "2", out, "--sh-passes", "4", "--depth", "4"] + extra)
        assert p.returncode == 0 and "baked 8 probes" in p.stdout, p.stderr[-2000:]
        with open(out) as f:
            lines = [l for l in f.read().splitlines() if l.strip()]
        assert len(lines) == 8
        rows[name] = np.array([[float(x) for x in l.split()] for l in lines])
        assert rows[name].shape == (8, 31) and np.isfinite(rows[name]).all()
        assert ((rows[name][:, 30] >= 0) & (rows[name][:, 30] <= 1)).all()
        assert np.allclose(rows[name][:, :3], R.grid(*kit.used_bounds(scene), 2, 2, 2), atol=1e-6)
        assert (rows[name][:, 3] != 0).all() and rows[name][:, 3].mean() > 0
    assert np.allclose(rows["irradiance"][:, 3], np.pi * rows["radiance"][:, 3], rtol=1e-5) and not np.allclose(rows["irradiance"][:, 4], rows["radiance"][:, 4])
    out = str(tmp_path / "bad.txt")
    for bad, word in ((["--sh-passes", "4"], "--sh-grid"), (["--sh-grid", "0", "2", "2", out], "[1, 1024]"), (["--sh-grid", "2", "2", "2", out, "--recursive"], "--recursive"),
                      (["--sh-grid", "2", "2", "2", out, "--sh-passes", "0"], "N >= 1")):
        p = kit.run_cli([obj, "--ref-index-order", "--spp", "1"] + bad)
        assert p.returncode == 2 and word in p.stderr, (bad, p.stderr[-500:])
