"""-m gpu: the bake stage's direct-light mode (bk_direct_kernel in csrc/bake.hip, DESIGN.md section 27 "Direct light") through the C ABI -- that
OFF is the stage as it was, every probed term against the float64 restatement of tests/bake_direct_ref.py within BOUND (which
tests/test_bake_direct_ref.py derives on the CPU), that the film is made of exactly the probed terms, the known answer under the lamp and the
variance it buys, unbiasedness with indirect light, live scenes, refusals and what the calls leave alone, the C++ facade and mcpt_cli.

The device draws its light sample from rng_block(item, sample, 0xFFFFFFFF): the tests read the numbers through probe_rng and hand them, with the
probed rays, to the restatement.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

from tests import bake_direct_ref as D, bake_ref as R, kit, shade_ref
from tests.kit import bits

pytestmark = pytest.mark.gpu

SEED = D.SEED
INVALID = 1
RADIANCE = np.array([17.0, 12.0, 4.0], np.float32)           # open_box's lamp


def _xi(r, first, n, sample, seed, block=D.DIRECT_BLOCK):
    key = np.stack([np.arange(first, first + n), np.full(n, sample), np.full(n, block)], 1)
    return r.probe_rng(key.astype(np.uint32), seed)[:, :3]


def _both_runs(r, scene, sample, seed, first=0, n=None, **pose):
    """The restatement in both types from the device's own rays and random numbers: (r64, r32, left out, rays)."""
    o, d, nn, dead = r.probe_bake_rays(sample, seed, first, n)
    centre = np.array(r.info().centre)
    xi = _xi(r, first, len(o), sample, seed)
    r64 = D.terms(scene, centre, o, nn, d, xi, np.float64, dead, **pose); r32 = D.terms(scene, centre, o, nn, d, xi, np.float32, dead, **pose)
    left = r64.ill | D.unsure_rows(scene, centre, o, d, r64, r32, vertex=pose.get("vertex"), visible=pose.get("visible"))
    return r64, r32, left, (o, d, nn, dead)


def _check_rows(r, scene, sample, seed, first=0, n=None, **pose):
    """probe_bake_direct against the float64 restatement: the integer columns equal and every float within BOUND on the kept rows, at most 2 % of
    the rows left out (lists of 257 or more).  (floats, ints, r64, left out, worst units)."""
    r64, r32, left, rays = _both_runs(r, scene, sample, seed, first, n, **pose)
    f, k = r.probe_bake_direct(sample, seed, first, n)
    if len(left) >= 257:
        assert left.mean() <= D.EXCLUSION_CAP, "%d of %d rows left out" % (left.sum(), len(left))
    keep = ~left
    want = np.stack([r64.hit_face, r64.front, r64.light_face, r64.state], 1)
    bad = keep & (k != want).any(1)
    assert not bad.any(), "%d rows differ in face / front / light / state, first %d: device %s, restatement %s" % (bad.sum(), np.flatnonzero(bad)[0], k[bad][0], want[bad][0])
    assert np.array_equal(k[:, 2], r64.light_face), "the sampled light differs from light_index' pick"
    live = keep & (r64.state != D.DEAD)
    units = D.worst_units(f, r64, live)
    print("%4d rows (%d left out), sample %d: worst units of BOUND = %g: %s" % (len(left), left.sum(), sample, D.BOUND, ", ".join("%s %.2f" % kv for kv in units.items())))
    assert max(units.values()) <= D.BOUND, units
    assert (f[r64.state == D.DEAD] == 0).all()
    return f, k, r64, left, units


def _lamp_faces(scene):
    return shade_ref.light_faces(scene)


# ------------------------------------------------------------------------------------------------------------------------ 1
def test_off_is_the_stage_as_it_was(pkg):
    """A context that never called the setter, one set to OFF and one set to MIS and back to OFF give bit-identical bake films over three passes;
    device_bytes moves as tests/test_bake.py says (33 B per point, 48 B more from the first bake) in either mode: the mode costs no memory."""
    scene = pkg.scenes.open_box(16, 16)
    pts = D.family_points(pkg, scene, 1000)
    films = []
    for setup in ((), (pkg.BAKE_DIRECT_OFF,), (pkg.BAKE_DIRECT_MIS, pkg.BAKE_DIRECT_OFF)):
        r = pkg.Renderer(scene, max_depth=4)
        for mode in setup:
            r.set_bake_direct(mode)
        r.set_bake_points(pts)
        assert r.bake_info().direct_mode == pkg.BAKE_DIRECT_OFF
        r.bake(3, SEED, 0)
        films.append(r.read_bake_film())
        r.close()
    assert (films[0][:, 3] == 3).all() and (films[0][:, :3] != 0).any()
    assert np.array_equal(bits(films[0]), bits(films[1])) and np.array_equal(bits(films[0]), bits(films[2]))
    n = 300
    for mode in (pkg.BAKE_DIRECT_OFF, pkg.BAKE_DIRECT_MIS):
        r = pkg.Renderer(scene, max_depth=4)
        r.set_bake_direct(mode)
        r.set_bake_points(pts[:n]); r.bake(1, SEED, 0); r.set_bake_points(None)     # (the pools of an n-item job exist after this)
        bytes0 = r.info().device_bytes
        r.set_bake_points(pts[:n])
        assert r.info().device_bytes == bytes0 + 33 * n and r.bake_info().device_bytes == 33 * n
        r.probe_bake_direct(0, SEED)                                               # (scratch only)
        assert r.info().device_bytes == bytes0 + 33 * n
        r.bake(2, SEED, 0)
        assert r.info().device_bytes == bytes0 + 81 * n and r.bake_info().device_bytes == 81 * n and r.bake_info().direct_mode == mode
        r.close()


# ------------------------------------------------------------------------------------------------------------------------ 2
def test_probed_terms_against_float64(pkg):
    """The centred, black-walled box at max_depth 4, family and interior points on both sides, list lengths 1, 63, 65, 257 and 1000, samples 0, 1
    and 7: every row of probe_bake_direct within BOUND of the float64 restatement, nothing forgiven beyond the rows left out (at most 2 %); the
    states, faces and sides equal on the kept rows; a sub-range of the probe equals the rows of the whole, bit for bit."""
    scene = D.centred_box(pkg, black=True)
    r = pkg.Renderer(scene, max_depth=4)
    worst = {}; rows = out = 0; states = np.zeros(5, np.int64)
    last = None
    for pts, sample in D.box_lists(pkg, scene):
        if last is not pts:
            r.set_bake_points(pts); last = pts
        f, k, r64, left, units = _check_rows(r, scene, sample, SEED)
        for key, x in units.items():
            worst[key] = max(worst.get(key, 0.0), x)
        rows += len(left); out += int(left.sum()); states += np.bincount(k[:, 3], minlength=5)
        if len(pts) >= 65:
            first, m = 37, len(pts) - 50
            sf, sk = r.probe_bake_direct(sample, SEED, first, m)
            assert np.array_equal(bits(sf), bits(f[first:first + m])) and np.array_equal(sk, k[first:first + m])
    print("%d rows, %d left out (%.3f %%); states dead..counted %s; the device's worst units of BOUND = %g: %s" % (rows, out, 100.0 * out / rows, states, D.BOUND, worst))
    assert out / rows <= D.EXCLUSION_CAP and (states[[D.NO_PDF, D.BELOW, D.COUNTED]] > 0).all()
    only = r.probe_bake_direct(0, SEED, 3, 5)
    assert r.lib.mcpt_probe_bake_direct(r.ctx, 0, SEED, 3, 5, None, only[1].ctypes.data) == 0 and r.lib.mcpt_probe_bake_direct(r.ctx, 0, SEED, 3, 5, only[0].ctypes.data, None) == 0
    r.close()


def test_light_pick_on_nine_lights(pkg):
    """nine_light_scene: the sampled light's face is light_index' pick for every row -- random numbers, and xi0 at the k / 9 edges: among 65 536 items one lies within 2^-13 of
    every edge, as probe_rng shows --; the states meet the restatement's on the kept rows
    and all five occur (the sphere occludes)."""
    scene = shade_ref.nine_light_scene(pkg, 16, 16)
    r = pkg.Renderer(scene, max_depth=4)
    lights = shade_ref.light_faces(scene)
    assert len(lights) == 9 == r.info().n_lights
    N = 65536
    face = np.resize(np.arange(scene.face.shape[0]), N)
    pts = pkg.bake_points(face, np.float32(0.25), np.float32(0.25), (np.arange(N) // scene.face.shape[0]) % 2)
    r.set_bake_points(pts)
    xi = _xi(r, 0, N, 0, SEED)
    f, k = r.probe_bake_direct(0, SEED)
    idx, clamped = shade_ref.light_index(xi[:, 0], 9)
    live = k[:, 3] != D.DEAD
    assert np.array_equal(k[live, 2], lights[idx][live]) and live.mean() > 0.9
    edges = np.arange(1, 9, dtype=np.float64) / 9.0
    near = np.abs(xi[:, 0].astype(np.float64)[:, None] - edges[None]).min(0)
    print("nearest xi0 to each edge k / 9: %s (2^-24 = %.1e); picks per light %s" % (near, 2.0 ** -24, np.bincount(idx, minlength=9)))
    assert (near <= 2.0 ** -13).all() and (np.bincount(idx[live], minlength=9) > 0).all()
    # states and terms of a sub-range against the restatement (the brute force is 528 faces per ray)
    sub = slice(0, 1200)
    r.set_bake_points(pts[sub])
    r64, r32, left, _ = _both_runs(r, scene, 0, SEED)
    f, k = r.probe_bake_direct(0, SEED)
    keep = ~left
    print("left out %d of %d rows; states %s" % (left.sum(), len(left), np.bincount(k[:, 3], minlength=5)))
    assert np.array_equal(k[keep, 3], r64.state[keep]) and np.array_equal(k[keep, 0], r64.hit_face[keep])
    assert (np.bincount(k[keep, 3], minlength=5)[1:] > 0).all()
    r.close()


# ------------------------------------------------------------------------------------------------------------------------ 3
def test_the_film_is_the_probed_terms(pkg):
    """The centred open_box with lit walls, 1000 family points, MIS mode: after clear_bake(); bake(1, seed, 0) every colour sum is
    float32(float32(add - sub) + L) bit for bit (NaN zeroed on both sides) and every count 1 -- add and sub from the device's own
    probe_bake_direct, L from probe_paths started from the probed rays.  Then one call of three passes equals three single passes."""
    scene = D.centred_box(pkg)
    r = pkg.Renderer(scene, max_depth=4)
    centre = np.array(r.info().centre)
    assert np.array_equal(centre, np.zeros(3))
    pts = D.family_points(pkg, scene, 1000)
    r.set_bake_points(pts); r.set_bake_direct(pkg.BAKE_DIRECT_MIS)
    o, d, nn, dead = r.probe_bake_rays(0, SEED)
    assert not dead.any()
    L = r.probe_paths(o + centre, d, SEED)
    f, k = r.probe_bake_direct(0, SEED)
    delta = f[:, 3:6] - f[:, 0:3]
    assert delta.dtype == np.float32 and L.dtype == np.float32
    want = np.nan_to_num((np.float32(0) + delta) + L, nan=0.0)
    r.clear_bake(); r.bake(1, SEED, 0)
    film = r.read_bake_film()
    assert (film[:, 3] == 1).all()
    got = np.nan_to_num(film[:, :3], nan=0.0)
    diff = (bits(got) != bits(want)).any(1)
    print("%d items: %d with add, %d with sub (%d of them a lamp's front), %d differ" % (len(pts), (f[:, 3:6] != 0).any(1).sum(), (f[:, 0:3] != 0).any(1).sum(), (f[:, 6] != 0).sum(), diff.sum()))
    assert not diff.any(), "%d of %d items differ, first %d: film %s, terms %s" % (diff.sum(), len(diff), np.flatnonzero(diff)[0], got[diff][0], want[diff][0])
    assert (f[:, 3:6] != 0).any(1).sum() > 100 and (f[:, 6] != 0).sum() >= 1 and ((f[:, 0:3] != 0).any(1) & (f[:, 6] == 0)).sum() >= 1
    off = pkg.Renderer(scene, max_depth=4)
    off.set_bake_points(pts); off.bake(1, SEED, 0)
    assert not np.array_equal(bits(off.read_bake_film()), bits(film))             # the mode does something
    off.close()
    r.clear_bake()
    for s in (0, 1, 2):
        r.bake(1, SEED, s)
    single = r.read_bake_film()
    r.clear_bake(); r.bake(3, SEED, 0)
    three = r.read_bake_film()
    assert np.array_equal(bits(single), bits(three)) and (three[:, 3] == 3).all()
    r.close()


# ------------------------------------------------------------------------------------------------------------------------ 4
def test_known_answer_under_the_lamp(pkg):
    """65 536 items of the floor's centre in the black-walled box.  MIS mode: every kept item's record equals the restatement's
    add - sub + [front lamp hit] Le within BOUND units of 2^-24 max|Le|; the mean of the records lies within 5 sigma / sqrt(N) of F Le per channel,
    sigma the restatement's sample deviation over the same random numbers.  OFF mode: the mean of the same items lies within
    5 sqrt(F (1 - F) / N) Le.  The MIS records' sample variance is below the OFF records'; the ratio is printed beside the restatement's.

    On an MI355X: see DESIGN.md section 27."""
    scene = D.centred_box(pkg, black=True)
    r = pkg.Renderer(scene, max_depth=4)
    N = 65536
    pts = pkg.bake_points(np.zeros(N, np.uint32), np.float32(0.0), np.float32(0.5))
    r.set_bake_points(pts)
    r64, r32, left, (o, d, nn, dead) = _both_runs(r, scene, 0, SEED)
    assert left.mean() <= D.EXCLUSION_CAP and not dead.any()
    x0, x1, z0, z1, y = D.lamp_rect(scene)
    F = R.form_factor_rect(x0 - o[0, 0], x1 - o[0, 0], z0 - o[0, 2], z1 - o[0, 2], y - o[0, 1])
    le = RADIANCE.astype(np.float64)
    want = r64.add - r64.sub + r64.mis[:, None] * le[None]
    r.bake(1, SEED, 0)
    off = r.read_bake_film()
    r.set_bake_direct(pkg.BAKE_DIRECT_MIS); r.clear_bake(); r.bake(1, SEED, 0)
    mis = r.read_bake_film()
    assert (mis[:, 3] == 1).all() and (off[:, 3] == 1).all()
    units = np.abs(mis[:, :3].astype(np.float64) - want)[~left].max() / (D.EPS24 * le.max())
    print("%d items, %d left out; worst record %.2f units of BOUND = %g" % (N, left.sum(), units, D.BOUND))
    assert units <= D.BOUND
    sigma = want.std(0, ddof=1)
    mean = mis[:, :3].astype(np.float64).mean(0)
    print("F = %.6f, F Le = %s; MIS mean %s, off by %s (allowed %s)" % (F, F * le, mean, mean - F * le, 5 * sigma / np.sqrt(N)))
    assert (np.abs(mean - F * le) <= 5 * sigma / np.sqrt(N)).all()
    mean_off = off[:, :3].astype(np.float64).mean(0); sigma_off = np.sqrt(F * (1 - F)) * le
    print("OFF mean %s, off by %s (allowed %s)" % (mean_off, mean_off - F * le, 5 * sigma_off / np.sqrt(N)))
    assert (np.abs(mean_off - F * le) <= 5 * sigma_off / np.sqrt(N)).all()
    v_mis = mis[:, :3].astype(np.float64).var(0, ddof=1); v_off = off[:, :3].astype(np.float64).var(0, ddof=1)
    print("variance MIS / OFF per channel: device %s, restatement's prediction %s" % (v_mis / v_off, sigma ** 2 / sigma_off ** 2))
    assert (v_mis < v_off).all()
    r.close()


# ------------------------------------------------------------------------------------------------------------------------ 5
def _point_at(pkg, scene, faces, target, back=0):
    """The bake point on one of `faces` at the world position `target`."""
    for f in faces:
        c = scene.vertex[scene.face[f, :, 0]]
        uv, *_ = np.linalg.lstsq(np.stack([c[1] - c[0], c[2] - c[0]], 1), np.asarray(target, np.float64) - c[0], rcond=None)
        if uv[0] >= 0 and uv[1] >= 0 and uv[0] + uv[1] <= 1 and np.allclose(c[0] + uv[0] * (c[1] - c[0]) + uv[1] * (c[2] - c[0]), target, atol=1e-9):
            return (f, np.float32(uv[0]), np.float32(uv[1]), back)
    raise AssertionError("no face holds %s" % (target,))


def test_unbiased_with_indirect_light(pkg):
    """The lit-walled open_box at depth 4, eight points of 8192 items each -- the floor's centre, a floor corner, a wall, the ceiling beside the
    lamp, a point on the lamp and three back-side points --: per point and channel the MIS mean and the OFF mean differ by at most 5 combined
    standard errors; the back-side points, which look out of the box, have add = 0 in every item."""
    scene = pkg.scenes.open_box(16, 16)
    lamp = _lamp_faces(scene)
    rows = [_point_at(pkg, scene, (0, 1), (0.5, 0.0, 0.5)), _point_at(pkg, scene, (0, 1), (0.03125, 0.0, 0.03125)), _point_at(pkg, scene, (6, 7), (0.0, 0.4, 0.6)),
            _point_at(pkg, scene, (2, 3), (0.25, 1.0, 0.5)), _point_at(pkg, scene, lamp, (0.45, 0.999, 0.55)),
            _point_at(pkg, scene, (0, 1), (0.5, 0.0, 0.5), 1), _point_at(pkg, scene, (6, 7), (0.0, 0.4, 0.6), 1), _point_at(pkg, scene, (2, 3), (0.25, 1.0, 0.5), 1)]
    M = 8192
    cols = [np.repeat(np.array([row[j] for row in rows]), M) for j in range(4)]
    pts = pkg.bake_points(cols[0], cols[1].astype(np.float32), cols[2].astype(np.float32), cols[3].astype(np.uint32))
    r = pkg.Renderer(scene, max_depth=4)
    r.set_bake_points(pts)
    r.bake(1, SEED, 0)
    off = r.read_bake_film()[:, :3].astype(np.float64).reshape(8, M, 3)
    r.set_bake_direct(pkg.BAKE_DIRECT_MIS); r.clear_bake(); r.bake(1, SEED + 1, 0)
    mis = r.read_bake_film()[:, :3].astype(np.float64).reshape(8, M, 3)
    f, k = r.probe_bake_direct(0, SEED + 1)
    assert (k[:, 3] != D.DEAD).all() and np.isfinite(off).all() and np.isfinite(mis).all()
    add = f[:, 3:6].reshape(8, M, 3)
    assert (add[5:] == 0).all() and (add[:3] != 0).any()
    se = np.sqrt(off.var(1, ddof=1) / M + mis.var(1, ddof=1) / M)
    gap = np.abs(off.mean(1) - mis.mean(1))
    for p in range(8):
        print("point %d: OFF mean %s, MIS mean %s, gap / combined s.e. %s; variance MIS / OFF %s" % (p, off[p].mean(0), mis[p].mean(0), gap[p] / np.maximum(se[p], 1e-300), mis[p].var(0) / np.maximum(off[p].var(0), 1e-300)))
    assert (gap <= 5 * se).all()
    assert (off.mean(1)[:5] > 0).all()
    r.close()


# ------------------------------------------------------------------------------------------------------------------------ 6
def test_live_scenes(pkg):
    """A FLAG_DYNAMIC context.  After update_vertices lowers and shifts the lamp the probe meets the restatement from the NEW vertices; after
    update_materials makes the left wall a light and the lamp faint (|radiance| between 0.0001 and 0.01) the light count and the picks follow the
    new list and a front hit on the faint lamp keeps sub = 0; after set_face_visibility hides one triangle of the wall light it is never the
    sampled face and never the first hit; after rebuild() the probe's rows and a bake are bit for bit what they were."""
    scene = pkg.scenes.open_box(16, 16)
    r = pkg.Renderer(scene, max_depth=4, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_DETERMINISTIC)
    pts = D.family_points(pkg, scene, 1000)
    r.set_bake_points(pts); r.set_bake_direct(pkg.BAKE_DIRECT_MIS)
    _check_rows(r, scene, 0, SEED)
    lamp = _lamp_faces(scene)
    v = scene.vertex.copy()
    lv = np.unique(scene.face[lamp][:, :, 0])
    v[lv, 1] -= 0.25; v[lv, 0] += 0.0625
    r.update_vertices(v)
    f1, k1, r64, left, _ = _check_rows(r, scene, 0, SEED, vertex=v)
    old = D.terms(scene, np.array(r.info().centre), *[r.probe_bake_rays(0, SEED)[j] for j in (0, 2, 1)], _xi(r, 0, len(pts), 0, SEED))
    assert (np.abs(old.add - r64.add) > 1e-3).any(1).mean() > 0.1                  # (the move matters)
    # ---- materials: the left wall lights the box, the lamp turns faint
    mats = list(scene.materials)
    wall_mat = int(scene.face[6, 0, 3])
    mats[wall_mat] = dataclasses.replace(mats[wall_mat], radiance=(2.0, 1.0, 0.5))
    lamp_mat = int(scene.face[lamp[0], 0, 3])
    mats[lamp_mat] = dataclasses.replace(mats[lamp_mat], radiance=(0.005, 0.005, 0.002))
    r.update_materials(mats)
    wall = np.flatnonzero(scene.face[:, 0, 3] == wall_mat)
    assert r.info().n_lights == len(wall) == 2
    f2, k2, r64, left, _ = _check_rows(r, scene, 0, SEED, vertex=v, materials=mats)
    live = k2[:, 3] != D.DEAD
    assert np.isin(k2[live, 2], wall).all() and np.array_equal(r64.lights, wall)
    faint = np.isin(k2[:, 0], lamp) & (k2[:, 1] == 1)
    print("%d front hits on the faint lamp" % faint.sum())
    assert faint.sum() >= 5 and (f2[faint, 0:3] == 0).all() and (f2[faint, 6] == 0).all()
    # ---- visibility: one triangle of the wall light hidden
    mask = np.ones(scene.face.shape[0], np.uint8); mask[wall[0]] = 0
    r.set_face_visibility(mask)
    assert r.info().n_lights == 1
    f3, k3, r64, left, _ = _check_rows(r, scene, 0, SEED, vertex=v, materials=mats, visible=mask)
    assert (k3[live, 2] == wall[1]).all() and not (k3[:, 0] == wall[0]).any()
    # ---- rebuild: the leaf order changes, the rows do not
    r.clear_bake(); r.bake(2, SEED, 0)
    film = r.read_bake_film()
    for builder in (pkg.REBUILD_DEVICE, pkg.REBUILD_HOST):
        r.rebuild(builder)
        assert r.bake_info().direct_mode == pkg.BAKE_DIRECT_MIS
        f4, k4 = r.probe_bake_direct(0, SEED)
        assert np.array_equal(bits(f4), bits(f3)) and np.array_equal(k4, k3)
        r.clear_bake(); r.bake(2, SEED, 0)
        assert np.array_equal(bits(r.read_bake_film()), bits(film))
    r.close()


# ------------------------------------------------------------------------------------------------------------------------ 7
def test_refusals_and_neighbours(pkg):
    """An unknown mode is refused and the mode kept; the setter works without points and the mode survives set_bake_points, clear_bake and
    dropping the points; a clone reports OFF; bake_info().direct_mode follows the setter; the probe refuses a range beyond the list; on a
    FLAG_DETERMINISTIC context the film, the features and render_camera() after a direct bake are, bit for bit, those of a context that never
    baked."""
    scene = pkg.scenes.open_box(16, 16)
    r = pkg.Renderer(scene, max_depth=4, flags=pkg.FLAG_DETERMINISTIC); plain = pkg.Renderer(scene, max_depth=4, flags=pkg.FLAG_DETERMINISTIC)
    assert r.bake_info().direct_mode == pkg.BAKE_DIRECT_OFF
    r.set_bake_direct(pkg.BAKE_DIRECT_MIS)                                          # no points yet
    assert r.bake_info().direct_mode == pkg.BAKE_DIRECT_MIS and r.bake_info().device_bytes == 0
    for bad in (2, 7, 0xffffffff):
        with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_set_bake_direct: unknown mode" % INVALID):
            r.set_bake_direct(bad)
        assert r.bake_info().direct_mode == pkg.BAKE_DIRECT_MIS
    assert r.probe_bake_direct(0, SEED)[0].shape == (0, 12)
    pts = D.family_points(pkg, scene, 300)
    r.set_bake_points(pts)
    assert r.bake_info().direct_mode == pkg.BAKE_DIRECT_MIS
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_probe_bake_direct" % INVALID):
        r.probe_bake_direct(0, SEED, 298, 3)
    r.bake(2, SEED, 0); r.clear_bake()
    assert r.bake_info().direct_mode == pkg.BAKE_DIRECT_MIS
    k = r.clone()
    assert k.bake_info().direct_mode == pkg.BAKE_DIRECT_OFF
    k.close()
    r.set_bake_points(None)
    assert r.bake_info().direct_mode == pkg.BAKE_DIRECT_MIS
    r.set_bake_direct(pkg.BAKE_DIRECT_OFF)
    assert r.bake_info().direct_mode == pkg.BAKE_DIRECT_OFF
    r.set_bake_direct(pkg.BAKE_DIRECT_MIS); r.set_bake_points(pts)
    launches = r.counters().launches; paths = r.counters().paths
    r.bake(2, SEED, 0)
    assert r.counters().launches == launches + 1 and r.counters().paths == paths + 2 * len(pts) and (r.read_bake_film()[:, 3] == 2).all()
    assert np.array_equal(bits(kit.render_film(r, 2, SEED)), bits(kit.render_film(plain, 2, SEED)))
    r.clear(); plain.clear(); r.render_camera(2, SEED, 0); plain.render_camera(2, SEED, 0)
    assert np.array_equal(bits(r.read_accum()), bits(plain.read_accum()))
    r.render_features(4, 5); plain.render_features(4, 5)
    assert np.array_equal(bits(r.features()), bits(plain.features()))
    r.close(); plain.close()


# ------------------------------------------------------------------------------------------------------------------------ 8
def _atlas_room(pkg):
    """tests/test_bake.py's room again, the lamp small: a floor whose two triangles fill the lower-left quarter of the texture square under a
    lamp whose texcoords are one point (it covers no texel)."""
    S = pkg.scenes
    vertex = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1], [0.375, 0.5, 0.375], [0.625, 0.5, 0.375], [0.625, 0.5, 0.625], [0.375, 0.5, 0.625]], np.float64)
    normal = np.array([[0, 1, 0], [0, -1, 0]], np.float64)
    texcoord = np.array([[0, 0], [0.5, 0], [0.5, 0.5], [0, 0.5], [0.75, 0.75]], np.float64)
    face = np.zeros((4, 3, 4), np.int32)
    for f, (vi, ni, ti, m) in enumerate((((0, 2, 1), 0, (0, 2, 1), 0), ((0, 3, 2), 0, (0, 3, 2), 0), ((4, 5, 6), 1, (4, 4, 4), 1), ((4, 6, 7), 1, (4, 4, 4), 1))):
        face[f, :, 0] = vi; face[f, :, 1] = ni; face[f, :, 2] = ti; face[f, :, 3] = m
    mats = [S.Material("floor", kd=(0.7, 0.6, 0.5)), S.Material("lamp", kd=(0.5, 0.5, 0.5), radiance=(4.0, 4.0, 4.0))]
    return S.SceneData("atlas-room", vertex, normal, texcoord, face, mats, S.Camera((0.5, 0.3, 2.5), (0.5, 0.2, 0.0), (0, 1, 0), 40.0, 16, 16))


def test_facade_bake_direct(pkg, tmp_path):
    """Render::set_bake_direct through the host classes: the program refuses an unknown mode itself, bakes mcpt_lightmap_points' 12 x 12 map with
    8 samples in MIS mode and writes what the same calls give through the C ABI, bit for bit -- and not what OFF gives."""
    exe = kit.build_facade("facade_bake_direct.cpp", tmp_path)
    scene = _atlas_room(pkg)
    obj = scene.write(str(tmp_path / "a"))
    out = str(tmp_path / "bake.bin")
    line = kit.run_facade(exe, [obj, "12", "12", "8", out])
    n = int(line[0])
    pts, tex = pkg.lightmap_points(scene, 12, 12)
    assert n == len(pts) == 36
    lit = np.fromfile(out, np.float32).reshape(n, 4)
    r = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DETERMINISTIC)
    r.set_bake_points(pts); r.bake(8, 17, 0)
    off = r.read_bake(pkg.BAKE_DIFFUSE)
    r.set_bake_direct(pkg.BAKE_DIRECT_MIS); r.clear_bake(); r.bake(8, 17, 0)
    assert np.array_equal(bits(lit), bits(r.read_bake(pkg.BAKE_DIFFUSE))) and not np.array_equal(bits(lit), bits(off)) and (lit[:, :3] > 0).all()
    r.close()


def _read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    head = data.split(b"\n", 3)
    assert head[0] == b"P6" and head[2] == b"255"
    w, h = (int(x) for x in head[1].split())
    return np.frombuffer(head[3], np.uint8).reshape(h, w, 3)


def test_cli_bake_direct(pkg, tmp_path):
    """mcpt_cli --bake-lightmap 16 16 OUT.ppm --bake-direct writes a lightmap that differs from the one written without the flag, lit on the
    same texels; the flag without --bake-lightmap is refused."""
    obj = _atlas_room(pkg).write(str(tmp_path / "scene"))
    imgs = {}
    for name, extra in (("off", []), ("direct", ["--bake-direct"])):
        out = str(tmp_path / (name + ".ppm"))
        p = kit.run_cli([obj, "--ref-index-order", "--bake-lightmap", "16", "16", out, "--bake-spp", "16", "--depth", "4"] + extra)
        assert p.returncode == 0 and "baked 64 of 256 texels" in p.stdout, p.stderr[-2000:]
        imgs[name] = _read_ppm(out)
    covered = np.zeros((16, 16), bool); covered[:8, :8] = True
    assert (imgs["direct"][covered] > 0).all() and (imgs["direct"][~covered] == 0).all()
    assert not np.array_equal(imgs["off"], imgs["direct"])
    p = kit.run_cli([obj, "--ref-index-order", "--spp", "1", "--bake-direct"])
    assert p.returncode == 2 and "--bake-lightmap" in p.stderr
