"""-m gpu: the surface-baking stage (csrc/bake.hip) through the C ABI -- every ray against the float64 restatement of
tests/bake_ref.py within S_BOUND, which tests/test_bake_ref.py derives on the CPU; that the bake film is made of exactly the rays the probe
shows; two known answers (per item against a brute-force trace, and the lamp's analytic form factor); the DIFFUSE resolve; live scenes
(vertex updates, rebuilds, hidden faces); refusals and what the calls leave alone; the C++ facade and mcpt_cli.

The device draws its own directions from rng_block(item, sample, 0): the tests read the numbers through probe_rng and hand them to the
restatement.  The scenes are open_box and copies of it; lists hold at most a few thousand points, the analytic test's 65 536 apart.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import bake_ref as R, kit
from tests.kit import bits

pytestmark = pytest.mark.gpu

SEED = 20271
INVALID, UNSUPPORTED = 1, 6
RADIANCE = np.array([17.0, 12.0, 4.0], np.float32)           # open_box's lamp
LENGTHS = (1, 63, 65, 257, 1000)                            # partial waves, partial blocks, more than one block


def _xi(r, first, n, sample, seed):
    """Block 0's first two numbers of items first .. first + n - 1 for (sample, seed), from the generator itself."""
    key = np.stack([np.arange(first, first + n), np.full(n, sample), np.zeros(n, np.int64)], 1)
    return r.probe_rng(key.astype(np.uint32), seed)[:, :2]


def _family_points(pkg, scene, n, seed=SEED, faces=None):
    """n points on `scene`: every face (or `faces`) at every (u, v) of R.UV_SET on both sides first -- corners, edges, centroid, 2^-24 off a
    corner --, then random interior ones; cut or filled to n."""
    faces = np.arange(scene.face.shape[0]) if faces is None else np.asarray(faces)
    f, u, v, b = [], [], [], []
    for face in faces:
        for uv in R.UV_SET:
            for back in (0, 1):
                f.append(face); u.append(uv[0]); v.append(uv[1]); b.append(back)
    rng = np.random.default_rng(seed)
    m = max(0, n - len(f))
    a = rng.random((m, 2)); flip = a.sum(1) > 1; a[flip] = 1 - a[flip]
    f += list(rng.choice(faces, m)); u += list(a[:, 0]); v += list(a[:, 1]); b += list(rng.integers(0, 2, m))
    pts = pkg.bake_points(np.array(f[:n]), np.array(u[:n], np.float32), np.array(v[:n], np.float32), np.array(b[:n], np.uint32))
    over = pts["u"].astype(np.float64) + pts["v"].astype(np.float64) > 1.0                 # (fp32 rounding of a point on the far edge)
    pts["v"][over] = np.nextafter(pts["v"][over], np.float32(0))
    return pts


def _interior_points(pkg, scene, n, seed=SEED):
    """n points well inside their faces (every barycentric >= 0.05), all faces, both sides."""
    rng = np.random.default_rng(seed)
    a = rng.random((n, 2)); flip = a.sum(1) > 1; a[flip] = 1 - a[flip]
    a = 0.05 + 0.85 * a
    return pkg.bake_points(rng.integers(0, scene.face.shape[0], n), a[:, 0].astype(np.float32), a[:, 1].astype(np.float32), rng.integers(0, 2, n).astype(np.uint32))


def _box_plus(pkg):
    """open_box and, behind its back wall, three more faces: one with all-zero vertex normals (geometric fallback), one whose normals cancel along
    an edge, and a degenerate one (three collinear corners) with zero normals (dead)."""
    s = pkg.scenes.open_box(16, 16)
    nv, nn = s.vertex.shape[0], s.normal.shape[0]
    vertex = np.concatenate([s.vertex, np.array([[0.2, 0.2, -0.5], [0.8, 0.3, -0.5], [0.4, 0.9, -0.25], [0.125, 0.125, -0.75], [0.25, 0.375, -0.75], [0.375, 0.625, -0.75]])])     # (dyadic: collinear in fp64 too, after the centre is subtracted)
    normal = np.concatenate([s.normal, np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])])
    extra = np.zeros((3, 3, 4), np.int32)
    extra[0, :, 0] = (nv, nv + 1, nv + 2); extra[0, :, 1] = nn                       # zero normals on a proper triangle
    extra[1, :, 0] = (nv, nv + 2, nv + 1); extra[1, :, 1] = (nn + 1, nn + 2, nn + 3)  # cancelling at (u, v) = (0.5, 0)
    extra[2, :, 0] = (nv + 3, nv + 4, nv + 5); extra[2, :, 1] = nn                   # collinear corners, zero normals
    return pkg.scenes.SceneData("open-box-plus", vertex, normal, s.texcoord, np.concatenate([s.face, extra]), s.materials, s.camera, {})


def _centred_box(pkg, black=False):
    """open_box moved so that the centre every device coordinate is relative to is exactly 0 (section 25's copy): (o + centre) - centre is then o
    itself and probe_paths starts from the very origins the stage wrote.  black: every non-emissive material with kd = ks = 0."""
    s = pkg.scenes.open_box(16, 16)
    used = s.vertex[np.unique(s.face[:, :, 0])]
    v = s.vertex - (0.5 * used.min(0) + 0.5 * used.max(0))
    out = kit.with_arrays(pkg, s, vertex=v)
    if black:
        out.materials = [m if any(m.radiance) else pkg.scenes.Material(m.name) for m in s.materials]
    return out


def _check_rays(r, scene, pts, sample, seed, first=0, n=None, vertex=None, normal=None):
    """probe_bake_rays of the set list against the restatement: (worst ratio, rays, slack used)."""
    n = len(pts) - first if n is None else n
    o, d, nn, dead = r.probe_bake_rays(sample, seed, first, n)
    sub = pts[first:first + n]
    ro, rn, rd, rdead = R.rays(xi=_xi(r, first, n, sample, seed), **R.scene_inputs(scene, np.array(r.info().centre), sub, vertex, normal))
    assert np.array_equal(dead.astype(bool), rdead), "dead points differ from the restatement's: %s" % np.flatnonzero(dead.astype(bool) != rdead)[:8]
    assert np.array_equal(d, d.astype(np.float32).astype(np.float64))            # the doubles hold fp32 values
    assert np.isfinite(o).all() and np.isfinite(d).all() and ((d * d).sum(1) > 0.5).all()    # no NaN and no zero direction reaches the trace kernel
    ratio = R.ray_ratio(o, nn, d, ro, rn, rd)
    bad = np.flatnonzero(~(ratio <= 1.0))
    assert bad.size == 0, "%d of %d rays beyond S_BOUND, first: point %d %s, ratio %.3g" % (bad.size, n, first + bad[0], sub[bad[0]], ratio[bad[0]])
    return float(ratio.max()), (o, d, nn, dead), R.slack_used(o, nn, d, ro, rn, rd)


def test_rays_against_float64(pkg):
    """Every origin, normal and direction of the point families on open_box -- and on a copy with a zero-normal, a cancelling and a degenerate face
    -- for list lengths 1, 63, 65, 257 and 1000 and samples 0, 1 and 7: within S_BOUND units 2^-52 (1 + |x|) of the restatement (directions: plus
    half an fp32 ulp), none forgiven; dead exactly where the restatement says; a sub-range of the probe equals the same rows of the whole."""
    n_rays, n_dead, used = 0, 0, np.zeros(3)
    for scene in (pkg.scenes.open_box(16, 16), _box_plus(pkg)):
        r = pkg.Renderer(scene)
        extra = np.arange(scene.face.shape[0] - 3, scene.face.shape[0]) if scene.name == "open-box-plus" else None
        for length in LENGTHS:
            pts = _family_points(pkg, scene, length, SEED + length, faces=extra if length < 257 else None)
            r.set_bake_points(pts)
            for sample in (0, 1, 7):
                worst, (o, d, nn, dead), su = _check_rays(r, scene, pts, sample, SEED)
                used = np.maximum(used, su); n_rays += length; n_dead += int(dead.sum())
                if length >= 65:
                    first, m = 37, length - 50
                    so, sd, sn, sdead = r.probe_bake_rays(sample, SEED, first, m)
                    for a, b in ((so, o), (sd, d), (sn, nn)):
                        assert np.array_equal(bits(a), bits(b[first:first + m]))
                    assert np.array_equal(sdead, dead[first:first + m])
        if extra is not None:
            assert n_dead > 0
            info = r.bake_info()
            assert info.n_dead == 0                                              # (as of the last bake: none yet)
            r.bake(1, SEED, 0)
            o, d, nn, dead = r.probe_bake_rays(0, SEED)
            assert r.bake_info().n_dead == dead.sum() > 0
            lit = r.read_bake(pkg.BAKE_IRRADIANCE); film = r.read_bake_film()
            assert (film[:, 3] == 1).all() and (lit[dead.astype(bool)] == 0).all() and (lit[~dead.astype(bool), 3] == 1).all()
        r.close()
    print("%d rays (%d dead); slack used of S_BOUND = %g: origins %.2f, normals %.2f, directions beyond their half fp32 ulp %.2f" % (n_rays, n_dead, R.S_BOUND, *used))
    assert n_rays > 8000


def test_the_film_is_made_of_the_probed_rays(pkg):
    """On the centred open_box, clear_bake(); bake(1, seed, 0) against probe_paths started from the probed rays with the same seed: the colour sums
    equal bit for bit (NaN zeroed on both sides), every count 1.  One kind of item is not probe_paths' own: a ray that first meets the lamp from
    BEHIND.  probe_paths treats it as a camera ray, which sees a lamp's back lit; the bake takes exactly that radiance out beforehand, so its
    record is float32(-Le) + probe_paths' L, bit for bit again (which rays those are: kit.brute_force_trace).  Then one call of three passes
    equals three single passes, bit for bit."""
    scene = _centred_box(pkg)
    r = pkg.Renderer(scene, max_depth=4)
    centre = np.array(r.info().centre)
    assert np.array_equal(centre, np.zeros(3))
    pts = _family_points(pkg, scene, 1000)
    r.set_bake_points(pts)
    o, d, nn, dead = r.probe_bake_rays(0, SEED)
    assert not dead.any() and np.array_equal(bits(o), bits((o + centre) - centre))
    want = r.probe_paths(o + centre, d, SEED)
    t64, f64, _, _ = kit.brute_force_trace(scene, o + centre, d)
    lamp = _lamp_faces(scene)
    behind = (f64 >= 0) & np.isin(f64, lamp) & ((d * scene.normal[scene.face[np.where(f64 >= 0, f64, 0)][:, 0, 1]]).sum(1) >= 0)
    want[behind] = -RADIANCE[None] + want[behind]
    want = np.nan_to_num(want, nan=0.0)
    print("%d of %d rays first meet the lamp from behind" % (behind.sum(), len(pts)))
    assert behind.sum() >= 1 and want.dtype == np.float32
    r.clear_bake(); r.bake(1, SEED, 0)
    film = r.read_bake_film()
    assert (film[:, 3] == 1).all()
    got = np.nan_to_num(film[:, :3], nan=0.0)
    diff = (bits(got) != bits(want)).any(1)
    assert not diff.any(), "%d of %d items differ, first %d: film %s, probe %s" % (diff.sum(), len(diff), np.flatnonzero(diff)[0], got[diff][0], want[diff][0])
    assert (got != 0).any(1).mean() > 0.1                                       # (half the points look out of the box from its walls' backs: most items are black)
    r.clear_bake()
    for s in (0, 1, 2):
        r.bake(1, SEED, s)
    single = r.read_bake_film()
    r.clear_bake(); r.bake(3, SEED, 0)
    three = r.read_bake_film()
    assert np.array_equal(bits(single), bits(three)) and (three[:, 3] == 3).all()
    r.clear_bake(); r.bake(1, SEED, 1)
    assert not np.array_equal(bits(r.read_bake_film()), bits(film))             # another sample, other rays
    i = r.bake_info()
    assert (i.n_points, i.bakes, i.passes) == (1000, 6, 8) and i.last_stage_ms > 0
    r.close()


def _lamp_faces(scene):
    return np.flatnonzero(np.array([any(scene.materials[m].radiance) for m in scene.face[:, 0, 3]]))


def test_known_answer_per_item(pkg):
    """open_box with black walls: an item's L is the lamp's radiance exactly when kit.brute_force_trace of its probed ray first meets a lamp face
    from the side its normals point to, and 0 otherwise.  Left out: items whose ray the brute force cannot decide -- fp64 and fp32 arithmetic name
    different faces, the hit lies within 1e-4 (relative) of a second face's, or within 1e-4 of the winning face's edge; at most 1 % of them.

    The rays that meet the lamp from behind (29 of these 4000, all from the ceiling) are what bk_unlit_kernel exists for: wf_shade_kernel adds a
    primary hit's emission whatever its side, and the stage takes it out again."""
    scene = _centred_box(pkg, black=True)
    r = pkg.Renderer(scene, max_depth=4)
    centre = np.array(r.info().centre)
    pts = _interior_points(pkg, scene, 4000)
    r.set_bake_points(pts)
    o, d, nn, dead = r.probe_bake_rays(0, SEED)
    t64, f64, u64, v64 = kit.brute_force_trace(scene, o + centre, d)
    t32, f32, _, _ = kit.brute_force_trace(scene, o + centre, d, dtype=np.float32)
    # the second-closest face, by tracing again with the winner's distance as the floor
    t2nd, _, _, _ = kit.brute_force_trace(scene, o + centre + d * (np.where(f64 >= 0, t64, 0.0) * (1 + 1e-4))[:, None], d, t1=0.0)
    hit = f64 >= 0
    unsure = (f64 != f32) | (hit & (np.minimum(np.minimum(u64, v64), 1 - u64 - v64) < 1e-4)) | (hit & np.isfinite(t2nd) & (t2nd < 2e-4 * np.where(hit, t64, 1.0)))
    print("left out: %d of %d items (%.3f %%)" % (unsure.sum(), len(pts), 100.0 * unsure.mean()))
    assert unsure.mean() <= 0.01
    lamp = _lamp_faces(scene)
    nl = scene.normal[scene.face[np.where(hit, f64, 0)][:, 0, 1]]
    lit = hit & np.isin(f64, lamp) & ((d * nl).sum(1) < 0)
    want = np.where(lit[:, None], RADIANCE[None], np.float32(0))
    r.bake(1, SEED, 0)
    film = r.read_bake_film()
    assert (film[:, 3] == 1).all()
    bad = ~unsure & (bits(film[:, :3] + np.float32(0)) != bits(want)).any(1)      # (+ 0: a -0 sum is a 0)
    behind = hit & np.isin(f64, lamp) & ((d * nl).sum(1) >= 0)
    print("%d items differ; %d rays first meet the lamp from behind, %d of the differing items are among them" % (bad.sum(), behind.sum(), (bad & behind).sum()))
    assert not bad.any(), "%d items differ, first %d: %s, wanted %s, face %d" % (bad.sum(), np.flatnonzero(bad)[0], film[bad][0], want[bad][0], f64[bad][0])
    print("%d of %d items see the lamp" % (lit.sum(), len(pts)))
    assert lit.sum() > 20
    r.close()


def test_known_answer_analytic(pkg):
    """The same scene, 65 536 items of ONE point, the floor's centre under the lamp, at 1 spp: each item has its own random numbers.  With p the
    analytic point-to-rectangle form factor of the lamp (fp64 closed form) the share of items that see it is within 5 sqrt(p (1 - p) / N) of
    p; read_bake(BAKE_IRRADIANCE) of each item is float(pi) L bit for bit."""
    scene = _centred_box(pkg, black=True)
    r = pkg.Renderer(scene, max_depth=4)
    N = 65536
    # the floor is faces 0 and 1 = (a, b, c), (a, c, d) of the quad: its centre is the midpoint of the shared edge a - c
    pts = pkg.bake_points(np.zeros(N, np.uint32), np.float32(0.0), np.float32(0.5))
    r.set_bake_points(pts)
    o, d, nn, dead = r.probe_bake_rays(0, SEED, 0, 4)
    p0 = scene.vertex[scene.face[0, :, 0]]
    centre_point = p0[0] + 0.5 * (p0[2] - p0[0])
    assert np.allclose(o, centre_point[None], atol=1e-15) and np.array_equal(nn, np.tile([0.0, 1.0, 0.0], (4, 1)))
    lv = scene.vertex[np.unique(scene.face[_lamp_faces(scene)][:, :, 0])]
    h = lv[0, 1] - centre_point[1]
    p = R.form_factor_rect(lv[:, 0].min() - centre_point[0], lv[:, 0].max() - centre_point[0], lv[:, 2].min() - centre_point[2], lv[:, 2].max() - centre_point[2], h)
    r.bake(1, SEED, 0)
    film = r.read_bake_film()
    assert (film[:, 3] == 1).all()
    seen = (film[:, :3] == RADIANCE[None]).all(1)
    assert (seen | (film[:, :3] == 0).all(1)).all()
    share = seen.mean(); tol = 5.0 * np.sqrt(p * (1 - p) / N)
    print("form factor %.6f, share of %d items %.6f, difference %.2e (allowed %.2e)" % (p, N, share, share - p, tol))
    assert abs(share - p) <= tol
    lit = r.read_bake(pkg.BAKE_IRRADIANCE)
    assert np.array_equal(bits(lit[:, :3] + np.float32(0)), bits(np.float32(np.pi) * film[:, :3] + np.float32(0))) and (lit[:, 3] == 1).all()
    r.close()


def test_bake_diffuse_is_the_texel_times_the_mean(pkg):
    """open_box with a 5 x 3 image on its white material: on the floor, the ceiling and the back wall read_bake(BAKE_DIFFUSE) is
    probe_texture(material, uv of probe_hit_shade) * (sum / count), in fp32, bit for bit, after 1 and after 3 samples."""
    s = pkg.scenes.open_box(16, 16)
    tex = np.random.default_rng(SEED).integers(30, 256, (3, 5, 3)).astype(np.uint8)
    mats = list(s.materials); mats[0] = pkg.scenes.Material("white", kd=(0.7, 0.7, 0.7), map_kd="white.ppm", texture=tex)
    scene = pkg.scenes.SceneData(s.name, s.vertex, s.normal, s.texcoord, s.face, mats, s.camera, {})
    r = pkg.Renderer(scene, max_depth=4)
    white = np.flatnonzero(scene.face[:, 0, 3] == 0)
    pts = _family_points(pkg, scene, 1500, faces=white)
    pts["flags"] = 0
    r.set_bake_points(pts)
    uv = r.probe_hit_shade(pts["face"].astype(np.int32), pts["u"], pts["v"], np.tile([0.0, 0.0, 1.0], (len(pts), 1)))[:, 3:5]
    kd = r.probe_texture(0, uv)
    assert len(np.unique(kd, axis=0)) >= 10                                       # (several texels are in play)
    for spp in (1, 3):
        r.clear_bake(); r.bake(spp, SEED, 0)
        film = r.read_bake_film()
        assert (film[:, 3] == spp).all()
        m = film[:, :3] / film[:, 3:4]
        assert m.dtype == np.float32
        got = r.read_bake(pkg.BAKE_DIFFUSE)
        assert np.array_equal(bits(np.nan_to_num(got[:, :3])), bits(np.nan_to_num(kd * m))) and (got[:, 3] == spp).all()
        assert (got[:, :3].max(1) > 0).mean() > 0.2                                  # (lit, not a film of zeros)
    r.close()


def test_live_scenes(pkg):
    """A FLAG_DYNAMIC context: after update_vertices with a deformation that keeps the bounding box (the lamp tilted and lowered, the floor's
    normals skewed) the probed rays meet the restatement from the NEW vertices and normals; after rebuild() the probed rays and a deterministic
    bake are bit for bit what they were before it; points on faces hidden by set_face_visibility stay alive and keep their rays."""
    scene = pkg.scenes.open_box(16, 16)
    r = pkg.Renderer(scene, max_depth=4, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_DETERMINISTIC)
    pts = _family_points(pkg, scene, 1000)
    r.set_bake_points(pts)
    old = r.probe_bake_rays(0, SEED)
    lamp = _lamp_faces(scene)
    v = scene.vertex.copy(); n = scene.normal.copy()
    lv = np.unique(scene.face[lamp][:, :, 0])
    v[lv[:2], 1] -= 0.2; v[lv, 0] += 0.05
    n[np.unique(scene.face[lamp][:, :, 1])] = np.array([0.3, -0.9, 0.1]) / np.linalg.norm([0.3, -0.9, 0.1])
    fn = np.unique(scene.face[:2][:, :, 1])
    n[fn] = (n[fn] + np.array([[0.2, 0.0, 0.1], [-0.1, 0.0, 0.3], [0.0, 0.0, -0.2], [0.25, 0.0, 0.0]])[:len(fn)])
    lo, hi = kit.used_bounds(scene)
    assert np.array_equal(lo, kit.used_bounds(kit.with_arrays(pkg, scene, v, n))[0]) and np.array_equal(hi, kit.used_bounds(kit.with_arrays(pkg, scene, v, n))[1])
    r.update_vertices(v, n)
    worst, new, used = _check_rays(r, scene, pts, 0, SEED, vertex=v, normal=n)
    moved = (bits(new[0]) != bits(old[0])).any(1) | (bits(new[1]) != bits(old[1])).any(1)
    on_changed = np.isin(pts["face"], np.concatenate([lamp, [0, 1]]))
    assert moved[on_changed].mean() > 0.5 and not moved[~on_changed].any()
    print("after the update: worst ratio %.3f of S_BOUND; %d rays moved" % (worst, moved.sum()))
    # ---- rebuild: the leaf order changes, the points do not
    r.clear_bake(); r.bake(2, SEED, 0)
    film = r.read_bake_film()
    hash0 = r.info().wide_tree_hash; bytes0 = r.info().device_bytes
    r.rebuild(pkg.REBUILD_DEVICE)
    print("rebuild: the tree's hash %s" % ("changed" if r.info().wide_tree_hash != hash0 else "stayed"))
    again = r.probe_bake_rays(0, SEED)
    for a, b in zip(again, new):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(r.read_bake_film()), bits(film))                  # the bake film is kept
    assert r.bake_info().device_bytes == 81 * len(pts) and r.bake_info().n_points == len(pts)
    r.clear_bake(); r.bake(2, SEED, 0)
    assert np.array_equal(bits(r.read_bake_film()), bits(film))
    r.rebuild(pkg.REBUILD_HOST)
    for a, b in zip(r.probe_bake_rays(0, SEED), new):
        assert np.array_equal(bits(a), bits(b))
    r.clear_bake(); r.bake(2, SEED, 0)
    assert np.array_equal(bits(r.read_bake_film()), bits(film))
    # ---- hidden faces: their corners and normals survive the hide, so their points stay alive and keep their rays
    mask = np.ones(scene.face.shape[0], np.uint8); mask[[lamp[0], 4, 5]] = 0
    r.set_face_visibility(mask)
    hidden = r.probe_bake_rays(0, SEED)
    for a, b in zip(hidden, new):
        assert np.array_equal(bits(a), bits(b))
    assert not hidden[3].any()
    r.clear_bake(); r.bake(1, SEED, 0)
    assert (r.read_bake_film()[:, 3] == 1).all() and r.bake_info().n_dead == 0
    r.close()


def test_refusals_and_neighbours(pkg):
    """Every refusal of set_bake_points leaves points and film as they were; bake needs points, the wavefront pipeline and a sample range below
    2^32; device_bytes grows by 33 B per point with the points and by 48 B more with the first bake, and only then; a clone has no points; on a
    FLAG_DETERMINISTIC context the film of a render() after a bake, render_camera() and the features are, bit for bit, those of a context that
    never baked."""
    scene = pkg.scenes.open_box(16, 16)
    r = pkg.Renderer(scene, max_depth=4, flags=pkg.FLAG_DETERMINISTIC); plain = pkg.Renderer(scene, max_depth=4, flags=pkg.FLAG_DETERMINISTIC)
    n = 300
    pts = _family_points(pkg, scene, n)
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_bake: no bake points" % INVALID):
        r.bake(1, SEED, 0)
    assert r.bake_info().device_bytes == 0 and r.read_bake().shape == (0, 4)
    # the pools of an n-item probe job exist after this; drop everything again: from here on device_bytes moves by the bake's buffers alone
    r.set_bake_points(pts); r.bake(1, SEED, 0); r.set_bake_points(None)
    assert r.bake_info().n_points == 0 and r.bake_info().device_bytes == 0
    bytes0 = r.info().device_bytes
    r.set_bake_points(pts)
    assert r.info().device_bytes == bytes0 + 33 * n and r.bake_info().device_bytes == 33 * n
    r.bake(0, SEED, 0)                                                           # spp = 0 does nothing
    assert r.info().device_bytes == bytes0 + 33 * n and r.bake_info().bakes == 1
    r.bake(2, SEED, 0)
    assert r.info().device_bytes == bytes0 + 81 * n and r.bake_info().device_bytes == 81 * n
    film = r.read_bake_film(); rays = r.probe_bake_rays(0, SEED)
    assert (film[:, 3] == 2).all()
    nan, inf = float("nan"), float("inf")
    bad = []
    for k, (field, value) in enumerate((("face", scene.face.shape[0]), ("face", 0xffffffff), ("u", nan), ("v", inf), ("u", -1e-30), ("v", -0.5), ("flags", 2), ("flags", 0x80000001))):
        p = pts.copy(); p[field][(37 * k) % n] = value; bad.append(p)
    p = pts.copy(); p["u"][5] = 0.75; p["v"][5] = np.nextafter(np.float32(0.25), np.float32(1)); bad.append(p)
    for p in bad:
        with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_set_bake_points: point" % INVALID):
            r.set_bake_points(p)
    assert r.lib.mcpt_set_bake_points(r.ctx, None, 5) == INVALID and r.lib.mcpt_set_bake_points(r.ctx, pts.ctypes.data, 0x4000000) == INVALID
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_bake: first_sample" % INVALID):
        r.bake(2, SEED, 2 ** 32 - 1)
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_probe_bake_rays" % INVALID):
        r.probe_bake_rays(0, SEED, n - 3, 4)
    assert r.lib.mcpt_read_bake(r.ctx, 2, film.ctypes.data) == INVALID
    r._n_bake = n
    assert np.array_equal(bits(r.read_bake_film()), bits(film)) and r.bake_info().n_points == n and r.info().device_bytes == bytes0 + 81 * n
    for a, b in zip(r.probe_bake_rays(0, SEED), rays):
        assert np.array_equal(bits(a), bits(b))
    launches = r.counters().launches; paths = r.counters().paths
    r.bake(3, SEED, 2)
    assert r.counters().launches == launches + 1 and r.counters().paths == paths + 3 * n and (r.read_bake_film()[:, 3] == 5).all()
    # setting points again zeroes the film; a list of another length drops the ray arrays until its first bake
    r.set_bake_points(pts[:100])
    assert (r.read_bake_film() == 0).all() and r.info().device_bytes == bytes0 + 33 * 100
    k = r.clone()
    assert k.bake_info().n_points == 0 and k.bake_info().device_bytes == 0
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_bake: no bake points" % INVALID):
        k.bake(1, SEED, 0)
    k.close()
    # what the calls leave alone
    r.bake(2, SEED, 0)
    assert np.array_equal(bits(kit.render_film(r, 2, SEED)), bits(kit.render_film(plain, 2, SEED)))
    r.clear(); plain.clear(); r.render_camera(2, SEED, 0); plain.render_camera(2, SEED, 0)
    assert np.array_equal(bits(r.read_accum()), bits(plain.read_accum()))
    r.render_features(4, 5); plain.render_features(4, 5)
    assert np.array_equal(bits(r.features()), bits(plain.features()))
    assert bytes(r.camera_model()) == bytes(plain.camera_model())
    r.close(); plain.close()
    rec = pkg.Renderer(scene, max_depth=4, integrator=pkg.INTEGRATOR_RECURSIVE_NEE)
    rec.set_bake_points(pts)                                                     # the points are state of every context
    with pytest.raises(pkg.McptError, match="mcpt status %d: mcpt_bake" % UNSUPPORTED):
        rec.bake(1, SEED, 0)
    rec.close()


def _atlas_room(pkg):
    """A floor whose two triangles fill the lower-left quarter [0, 0.5]^2 of the texture square, under a large lamp whose texcoords are one point
    (it covers no texel): what --bake-lightmap needs to show covered and uncovered texels."""
    S = pkg.scenes
    vertex = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1], [-0.5, 0.5, -0.5], [1.5, 0.5, -0.5], [1.5, 0.5, 1.5], [-0.5, 0.5, 1.5]], np.float64)
    normal = np.array([[0, 1, 0], [0, -1, 0]], np.float64)
    texcoord = np.array([[0, 0], [0.5, 0], [0.5, 0.5], [0, 0.5], [0.75, 0.75]], np.float64)
    face = np.zeros((4, 3, 4), np.int32)
    for f, (vi, ni, ti, m) in enumerate((((0, 2, 1), 0, (0, 2, 1), 0), ((0, 3, 2), 0, (0, 3, 2), 0), ((4, 5, 6), 1, (4, 4, 4), 1), ((4, 6, 7), 1, (4, 4, 4), 1))):
        face[f, :, 0] = vi; face[f, :, 1] = ni; face[f, :, 2] = ti; face[f, :, 3] = m
    mats = [S.Material("floor", kd=(0.7, 0.6, 0.5)), S.Material("lamp", kd=(0.5, 0.5, 0.5), radiance=(0.5, 0.5, 0.5))]
    return S.SceneData("atlas-room", vertex, normal, texcoord, face, mats, S.Camera((0.5, 0.3, 2.5), (0.5, 0.2, 0.0), (0, 1, 0), 40.0, 16, 16))


def test_facade_bake(pkg, tmp_path):
    """Render::set_bake_points, bake and read_bake through the host classes: the program bakes mcpt_lightmap_points' 12 x 12 map with 8 samples in two calls and
    asserts the refusals itself; its output is what the same calls give through the C ABI, bit for bit."""
    exe = kit.build_facade("facade_bake.cpp", tmp_path)
    scene = _atlas_room(pkg)
    obj = scene.write(str(tmp_path / "a"))
    out = str(tmp_path / "bake.bin")
    line = kit.run_facade(exe, [obj, "12", "12", "8", out])
    n = int(line[0])
    pts, tex = pkg.lightmap_points(scene, 12, 12)
    assert n == len(pts) == 36 and int(line[1]) == 144
    raw = np.fromfile(out, np.uint8)
    lit = raw[:16 * n].view(np.float32).reshape(n, 4); texel = raw[16 * n:].view(np.uint32)
    assert np.array_equal(texel, tex)
    r = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DETERMINISTIC)
    r.set_bake_points(pts); r.bake(8, 17, 0)
    assert np.array_equal(bits(lit), bits(r.read_bake(pkg.BAKE_DIFFUSE))) and (lit[:, :3] > 0).all()
    r.close()


def _read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    head = data.split(b"\n", 3)
    assert head[0] == b"P6" and head[2] == b"255"
    w, h = (int(x) for x in head[1].split())
    return np.frombuffer(head[3], np.uint8).reshape(h, w, 3)


def test_cli_bake_lightmap(pkg, tmp_path):
    """mcpt_cli --bake-lightmap 16 16 on the atlas room writes a PPM whose covered texels (the lower-left quarter of the texture square: rows and
    columns 0 .. 7) are lit and whose other texels are black; --bake-irradiance gives another picture; the option's misuse is refused."""
    obj = _atlas_room(pkg).write(str(tmp_path / "scene"))
    imgs = {}
    for name, extra in (("diffuse", []), ("irradiance", ["--bake-irradiance"])):
        out = str(tmp_path / (name + ".ppm"))
        p = kit.run_cli([obj, "--ref-index-order", "--bake-lightmap", "16", "16", out, "--bake-spp", "16", "--depth", "4"] + extra)     # (SceneData.write's corner order)
        assert p.returncode == 0 and "baked 64 of 256 texels" in p.stdout, p.stderr[-2000:]
        imgs[name] = _read_ppm(out)
        covered = np.zeros((16, 16), bool); covered[:8, :8] = True
        assert imgs[name].shape == (16, 16, 3) and (imgs[name][covered] > 0).all() and (imgs[name][~covered] == 0).all()
    assert not np.array_equal(imgs["diffuse"], imgs["irradiance"])
    out = str(tmp_path / "bad.ppm")
    for bad, word in ((["--bake-spp", "4"], "--bake-lightmap"), (["--bake-lightmap", "0", "16", out], "[1, 8192]"), (["--bake-lightmap", "16", "16", out, "--recursive"], "--recursive"),
                      (["--bake-lightmap", "16", "16", out, "--panorama"], "camera model"), (["--bake-lightmap", "16", "16", out, "--bake-spp", "0"], "N >= 1")):
        p = kit.run_cli([obj, "--ref-index-order", "--spp", "1"] + bad)
        assert p.returncode == 2 and word in p.stderr, (bad, p.stderr[-500:])
