"""CPU tests (no GPU) of tests/endpoints_ref.py: the float64 restatements of cast_ray, load_hit_shade, tex_color and the tonemap are pinned to the
oracle and to the REAL reference's recorded answers, the constants of the error models (K_HIT, K_T) are measured here, on fp32 replays and never on
the device, the case generators hold the members they promise, and each comparison is shown to catch a planted fault on exactly the cases that
were tampered with.  The device side of the same inputs is tests/test_endpoints_edges.py."""
import os

import numpy as np
import pytest

from tests import endpoints_ref as E
from tests import kit
from tests.kit import bits

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


def _npz(name):
    with np.load(os.path.join(G, name)) as z:
        return {k: z[k] for k in z.files}


def _centre(scene):
    lo, hi = kit.used_bounds(scene)
    return 0.5 * lo + 0.5 * hi


@pytest.fixture(scope="module")
def hit(pkg):
    """(scene, cases, corner records, restatement, the uncontracted replay)."""
    scene, face_family = E.hit_mesh(pkg)
    case = E.hit_cases(scene, face_family)
    rec = E.corner_records(scene)
    args = (rec, case["tri"], case["u"], case["v"], case["d"])
    return scene, case, rec, E.hit_shade_ref(*args), E.hit_shade_replay(*args)


@pytest.fixture(scope="module")
def tone():
    """(films' pixels (N, 4), family (N, 3), the np.float32 chain's y and level)."""
    rgba, family = E.tonemap_cases()
    return (rgba, family) + E.tonemap_replay(rgba)


@pytest.fixture(scope="module")
def tex(pkg):
    """(scene, index of the first texture material, dims, the texel table of those materials)."""
    scene, first, dims = E.texture_scene(pkg)
    return scene, first, dims, np.concatenate([pkg.material_texels(m).reshape(-1, 3) for m in scene.materials[first:]])


# ------------------------------------------------------------------------------------------------------------------------ the restatements are the reference's formulas
def test_cast_ref_is_the_oracles_cast_ray(pkg, orc):
    """Every camera family on every film: the float64 direction within 1e-13 of Oracle.cast_ray's (unit vectors: relative to their length), the
    origin the fp32 rounding of the oracle's eye."""
    S = pkg.scenes
    base = S.open_box(8, 8)
    centre = _centre(base)
    worst = 0.0
    for w, h in E.FILMS:
        xy, xi, fam = E.pixel_cases(w, h)
        pick = np.concatenate([np.flatnonzero(fam == f)[::7] for f in np.unique(fam)])
        for family, name, c in E.camera_cases(base.camera, centre):
            cam = S.Camera(c["eye"], c["lookat"], c["up"], c["fovy"], w, h)
            o = orc.Oracle(S.SceneData(base.name, base.vertex, base.normal, base.texcoord, base.face, base.materials, cam))
            want = np.array([o.cast_ray(int(xy[i, 0]), int(xy[i, 1]), xi[i])[0] for i in pick])
            o.close()
            origin, d = E.cast_ref(cam, centre, w, h, xy[pick], xi[pick])
            err = np.abs(d - want[:, 3:6]).max()
            assert err <= 1e-13, (w, h, name, err)
            assert np.all(np.abs(origin.astype(np.float64) - want[:, 0:3]) <= E.cast_bound(want[:, 0:3])), (w, h, name)
            worst = max(worst, err)
    print("cast_ref against Oracle.cast_ray: worst direction difference %.3g" % worst)


def test_cast_ref_reproduces_the_recorded_reference(pkg):
    """The real reference's own camera rays on S-cornell-small (cs_cam_od): direction to 1e-13, origin equal after the fp32 rounding."""
    p = _npz("ref_paths.npz")
    scene = pkg.scenes.cornell_box_small(64, 64)
    origin, d = E.cast_ref(scene.camera, _centre(scene), 64, 64, p["cs_cam_xy"], p["cs_cam_xi"])
    od = p["cs_cam_od"]
    assert len(od) >= 100 and np.abs(d - od[:, 3:6]).max() <= 1e-13, np.abs(d - od[:, 3:6]).max()
    assert np.array_equal(np.broadcast_to(origin, od[:, 0:3].shape), od[:, 0:3].astype(F32))


def test_tex_ref_is_the_oracles_get_color(pkg, orc, tex):
    """Texture::get_color of the oracle on the fp32-valued uv: the same texel on every case of every texture, the constant colour included."""
    scene, first, dims, table = tex
    n = 0
    for k, (w, h, off) in enumerate(dims):
        img = pkg.material_texels(scene.materials[first + k])
        uv, fam = E.texture_cases(w, h)
        x, y, idx = E.tex_ref(w, h, off, uv)
        fin = np.flatnonzero(np.isfinite(uv).all(1))
        assert len(fin) == len(uv)
        got = np.array([orc.Oracle.texture_get_color(img, float(uv[i, 0]), float(uv[i, 1])) for i in fin])
        bad = np.flatnonzero(np.any(bits(got) != bits(table[idx]), axis=1))
        assert bad.size == 0, (w, h, uv[bad[0]], got[bad[0]], table[idx[bad[0]]])
        n += len(uv)
    assert 5000 <= n <= 20000


def test_tonemap_ref_contains_the_oracles_level(orc, tone):
    """Oracle.tonemap's level (std::pow(m, 0.5f), fp32) is admissible at K_T on every case with a finite mean, and so is the real reference's recorded film."""
    rgba, family, _, _ = tone
    lo, hi, y = E.tonemap_ref(rgba, E.K_T)
    with np.errstate(all="ignore"):
        finite = np.isfinite(rgba[:, :3] / rgba[:, 3:])
    lv = orc.Oracle.tonemap(rgba).astype(np.int64)
    assert finite.sum() >= 10000 and np.all((lv >= lo)[finite] & (lv <= hi)[finite])
    k = _npz("ref_kats.npz")
    lo, hi, y = E.tonemap_ref(np.ascontiguousarray(k["film_accum"], F32), E.K_T)
    u8 = k["film_u8"].astype(np.int64)
    assert u8.size >= 3000 and np.all((u8 >= lo) & (u8 <= hi))


def test_hit_shade_ref_is_the_oracles_record(pkg, orc, hit):
    """Rays aimed at the sampled points of the well-conditioned faces: Oracle.tri_hit's record (Triangle.cpp:68-76 in float64, barycentrics recomputed
    from the ray) carries the restatement's normal and uv to 1e-12 of their absolute-value forms, and its front flag."""
    scene, case, rec, ref, _ = hit
    rng = np.random.default_rng(5)
    sel = np.flatnonzero((case["family"] == "interior") & np.isin(case["face_family"], ("distinct", "uv0", "equal", "zero_corner")))[::9]
    assert len(sel) >= 400
    n_checked = 0
    for i in sel:
        f = int(case["tri"][i]); u, v = float(case["u"][i]), float(case["v"][i])
        P = scene.vertex[scene.face[f, :, 0]]
        ng = np.cross(P[1] - P[0], P[2] - P[0]); ng /= np.linalg.norm(ng)
        d = -ng + 0.3 * rng.normal(size=3); d = (d / np.linalg.norm(d)).astype(F32).astype(np.float64)
        point = (1 - u - v) * P[0] + u * P[1] + v * P[2]
        h, out = orc.Oracle.tri_hit(P.reshape(-1), rec[f, :, :3].astype(np.float64).reshape(-1), rec[f, :, 3:].astype(np.float64).reshape(-1), 0, point - 2.0 * d, d, 1e-4, 1e30)
        if not h:
            continue                                                              # (a point on an edge: the ray's own barycentrics may fall outside)
        r = E.hit_shade_ref(rec, [f], case["u"][i:i + 1], case["v"][i:i + 1], d[None])
        assert np.all(np.abs(out[4:7] - r.n[0]) <= 1e-12 * np.maximum(r.n_abs[0], 1.0)), (f, out[4:7], r.n[0])
        assert abs(out[7] - r.tu[0]) <= 1e-12 * max(r.tu_abs[0], 1.0) and abs(out[8] - r.tv[0]) <= 1e-12 * max(r.tv_abs[0], 1.0), (f, out[7:9], r.tu[0], r.tv[0])
        assert bool(out[9]) == bool(r.front[0]) or abs(r.nd[0]) < 1e-9
        n_checked += 1
    assert n_checked >= 0.95 * len(sel)


# ------------------------------------------------------------------------------------------------------------------------ the constants are measured
def test_k_is_measured(hit, tone):
    """K_HIT: the fp32 replay of load_hit_shade, product-sums contracted and not, the reciprocal square root moved by -1, 0, +1 ulp, against the float64
    restatement.  K_T: the np.float32 tonemap chain against float64.  Each constant is the next power of two at or above twice the worst ratio."""
    scene, case, rec, ref, _ = hit
    worst = np.zeros(len(case["tri"]))
    for contract in (False, True):
        for ulp in (-1, 0, 1):
            out = E.hit_shade_replay(rec, case["tri"], case["u"], case["v"], case["d"], contract, ulp)
            ratio, marginal, bad = E.hit_check(ref, out)
            assert not bad.any(), (contract, ulp, int(bad.sum()))
            worst = np.maximum(worst, ratio)
    E.print_worst("hit record, fp32 replay", case["face_family"], worst, E.K_HIT / 2)
    E.print_worst("hit record, fp32 replay", case["family"], worst, E.K_HIT / 2)
    print("hit record: worst ratio %.3f, K_HIT = %g" % (worst.max(), E.K_HIT))
    assert worst.max() <= E.K_HIT / 2 and E.next_pow2(2 * worst.max()) == E.K_HIT

    rgba, family, y32, _ = tone
    _, _, y = E.tonemap_ref(rgba)
    ratio = E.tonemap_ratio(y, y32)
    E.print_worst("tonemap, np.float32 chain", family.ravel(), ratio.ravel(), E.K_T / 2)
    print("tonemap: worst ratio %.3f, K_T = %g, device factor %g" % (ratio.max(), E.K_T, E.TONEMAP_DEVICE_FACTOR))
    assert ratio.max() <= E.K_T / 2 and E.next_pow2(2 * ratio.max()) == E.K_T


# ------------------------------------------------------------------------------------------------------------------------ the cases hold what they promise
def test_non_vacuity(hit, tone):
    """At the DEVICE's allowance: at least 99 % of the generic tonemap cases have exactly one admissible level and no boundary case more than two; at
    most 1 % of the hit-record cases are marginal."""
    rgba, family, _, _ = tone
    lo, hi, _ = E.tonemap_ref(rgba)
    one = (hi == lo)[family == "generic"].mean()
    print("tonemap: %.2f %% of the generic cases have one level; the boundary cases have at most %d" % (100 * one, (hi - lo)[family == "boundary"].max() + 1))
    assert one >= 0.99 and (hi - lo)[family == "boundary"].max() <= 1 and (hi - lo).min() == 0
    assert ((hi - lo)[family == "boundary"] == 1).sum() >= 255                  # ... and the boundaries really are boundaries
    scene, case, rec, ref, out = hit
    _, marginal, _ = E.hit_check(ref, out)
    print("hit record: %d of %d cases marginal = %.2f %%" % (marginal.sum(), len(marginal), 100 * marginal.mean()))
    assert 8000 <= len(marginal) <= 20000 and 0 < marginal.mean() <= 0.01


def test_every_family_has_the_member_it_promises(pkg, hit, tone, tex):
    S = pkg.scenes
    # camera
    base = S.open_box(8, 8)
    cams = E.camera_cases(base.camera, _centre(base))
    assert {c[0] for c in cams} == {"fovy", "up", "far_eye", "lookat_distance", "axis"}
    assert {c[2]["fovy"] for c in cams} >= {0.001, 1.0, 40.0, 90.0, 170.0, 179.9}
    assert {c[2]["up"] for c in cams} >= {(0.0, 1.0, 0.0), (0.0, 2.5, 0.0), (0.3, 1.0, 0.2)}
    near = [c[2] for c in cams if c[1] == "up 1e-3 rad from the view"][0]
    fr = np.subtract(near["lookat"], near["eye"]); fr /= np.linalg.norm(fr)
    assert np.isclose(np.linalg.norm(np.cross(fr, near["up"])), 1e-3, rtol=1e-3)
    dist = sorted(np.linalg.norm(np.subtract(c[2]["lookat"], c[2]["eye"])) for c in cams if c[0] == "lookat_distance")
    assert np.isclose(dist[0], 1e-12, rtol=1e-3) and np.isclose(dist[1], 1e15, rtol=1e-3)
    assert sorted(np.linalg.norm(np.subtract(c[2]["eye"], _centre(base))) > 9e5 for c in cams if c[0] == "far_eye") == [True, True]
    assert len([c for c in cams if c[0] == "axis"]) == 3
    assert E.FILMS == ((1, 1), (3, 2), (37, 21), (1, 257), (257, 1), (4097, 3), (16384, 2))
    for w, h in E.FILMS:
        xy, xi, fam = E.pixel_cases(w, h)
        assert set(fam) == {"corners", "last_column", "xi_edges", "random"} and len(xy) <= 20000
        assert xy.min() >= 0 and (xy[:, 0] < w).all() and (xy[:, 1] < h).all() and (xi >= 0).all() and (xi <= E.ONE_BELOW).all()
        for p in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2)):
            assert ((xy == p).all(1) & (fam == "corners")).sum() >= 16
        assert ((xy[:, 0] == w - 1) & (xi[:, 0] == E.ONE_BELOW) & (fam == "last_column")).sum() >= 4
        assert set(xi[fam == "xi_edges"].ravel()) <= set(F32(E.XI_SET))
    # hit record
    scene, case, rec, ref, _ = hit
    ff = case["face_family"]
    assert 190 <= scene.n_faces <= 210
    assert set(ff) == {"distinct", "uv0", "cancel3", "cancel6", "equal", "zero_corner", "zero_sum"}
    assert set(case["family"]) == {"corners", "edge_mid", "sum_one", "w_negative", "target", "interior", "nd_0", "nd_1e-7", "nd_1e-4"}
    d = rec[np.unique(case["tri"][ff == "distinct"])]
    for a, b in ((0, 1), (0, 2), (1, 2)):                                        # every corner differs from every other in every channel
        assert np.all(d[:, a, :] != d[:, b, :])
    assert np.all(np.abs(np.linalg.norm(d[:, :, :3].astype(np.float64), axis=2) - 1) > 1e-3)
    mags = np.abs(d[:, :, 3:]).max((1, 2))
    assert (mags <= 1).any() and ((mags > 10) & (mags <= 100)).any() and (mags > 1e5).any() and not rec[np.unique(case["tri"][ff == "uv0"])][:, :, 3:].any()
    at = (case["family"] == "target") & (case["u"] == E.HIT_TARGET[0]) & (case["v"] == E.HIT_TARGET[1])
    assert np.allclose(ref.length[at & (ff == "cancel3")], 1e-3, rtol=1e-2) and (at & (ff == "cancel3")).sum() >= 8
    assert np.allclose(ref.length[at & (ff == "cancel6")], 1e-6, rtol=0.3) and (at & (ff == "cancel6")).sum() >= 4
    assert (ref.length[at & (ff == "zero_sum")] == 0).all() and (~np.isfinite(ref.n).all(1)).sum() >= 8
    assert (rec[np.unique(case["tri"][ff == "zero_corner"])][:, :, :3] == 0).all(2).sum(1).min() == 1
    u64, v64 = case["u"].astype(np.float64), case["v"].astype(np.float64)
    so = case["family"] == "sum_one"
    assert (u64 + v64 == 1)[so].sum() >= 500 and (u64 + v64 > 1)[so].sum() >= 500 and (u64 + v64 < 1)[so].sum() >= 500
    assert np.all((1 - u64 - v64)[case["family"] == "w_negative"] == -E.EPS24)
    assert np.all((F32(1) - case["u"] - case["v"])[case["family"] == "w_negative"] == F32(-E.EPS24))
    exact = (case["family"] == "nd_0") & (ref.nd == 0) & (ref.nd_abs == 0)
    assert exact.sum() >= 24
    for name, lo_, hi_ in (("nd_1e-7", 2e-8, 5e-7), ("nd_1e-4", 5e-5, 2e-4)):
        m = case["family"] == name
        assert m.sum() >= 40 and np.median(np.abs(ref.nd[m])) > lo_ and np.median(np.abs(ref.nd[m])) < hi_ and (ref.nd[m] > 0).any() and (ref.nd[m] < 0).any()
    # texture
    _, first, dims, table = tex
    assert [(w, h) for w, h, _ in dims] == [(1, 1), (1, 1), (1, 7), (7, 1), (8, 5), (255, 3), (1000, 3), (3, 1000), (2000, 1), (4096, 2)]
    assert len(np.unique(table, axis=0)) == len(table) == sum(w * h for w, h, _ in dims)
    for w, h, off in dims:
        uv, fam = E.texture_cases(w, h)
        assert uv.dtype == F32 and np.isfinite(uv).all() and set(fam) == {"texel_edges", "cap", "denormal", "huge", "uniform"}
        assert (fam == "texel_edges").sum() == 5 * sum(n + 1 if n <= 255 else 64 for n in (w, h))
        flat = set(bits(uv).ravel().tolist())
        for x in (-0.0, 0.999, 1 - E.EPS24, 1.0, 2.0, -1.0, 2.0 ** -149, -2.0 ** -149, 1e-38, -1e-38, -2.0 ** -30, 2.0 ** 23 + 0.5, 2.0 ** 24, -2.0 ** 24, 1e10, -1e10, 3e38, -3e38):
            assert int(bits(np.array([x], F32))[0]) in flat, x
        for n, col in ((w, 0), (h, 1)):
            ks = range(n + 1) if n <= 255 else (0, 1, n - 1, n)
            have = set(bits(uv[:, col]).tolist())
            for k in ks:
                e = F32(k) / F32(n)
                assert all(int(bits(E._steps([e], s))[0]) in have for s in (-2, -1, 0, 1, 2)), (n, k)
    # the wide images whose cap lands on a texel edge
    assert int(0.999 * 1000) == 999 and E.tex_ref(2000, 1, 0, np.array([[0.9995, 0.0]], F32))[0][0] == 1998
    # tonemap
    rgba, family, _, lv = tone
    assert set(family.ravel()) == {"boundary", "special", "above_one", "denormal", "generic"}
    assert (family == "boundary").sum() == 255 * 7 * len(E.COUNTS) and set(rgba[(family == "boundary").any(1), 3]) == set(F32(E.COUNTS))
    assert set(lv[family == "boundary"]) == set(range(0, 256))
    sp = (family == "special").any(1)
    assert (rgba[sp, 3] == 0).any() and np.isnan(rgba[sp, :3]).any() and np.isposinf(rgba[sp, :3]).any() and np.isneginf(rgba[sp, :3]).any()
    den = rgba[:, :3][family == "denormal"]
    assert (den != 0).all() and (np.abs(den) < 2.0 ** -126).all()
    assert E.TONEMAP_FILMS == ((1, 1), (3, 2), (37, 21), (255, 1), (1, 257), (64, 5))


def test_tonemap_definition(tone):
    """The definition tonemap_ref pins: a NaN mean gives 0, +inf gives 255, negative and -inf give 0, count 0 with sum 0 gives 0."""
    px = np.array([[np.nan, np.inf, -np.inf, 1], [0, 1, -1, 0], [-0.25, -0.0, 4, 1], [1 + 2.0 ** -23, 1.5, 1e30, 1]], F32)
    lo, hi, _ = E.tonemap_ref(px)
    want = np.array([[0, 255, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]])
    assert np.array_equal(lo, want) and np.array_equal(hi, want)
    assert np.array_equal(E.tonemap_replay(px)[1], want)


# ------------------------------------------------------------------------------------------------------------------------ planted faults
def test_planted_faults_fail_exactly_the_tampered_cases(pkg, hit, tone, tex):
    """On the fp32 replays' own answers -- which pass --, each fault fails the cases it touched and no other."""
    # a texel index moved by one on 1 case in 2000
    scene, first, dims, table = tex
    idx = np.concatenate([E.tex_ref(w, h, off, E.texture_cases(w, h)[0])[2] for w, h, off in dims])
    hit_ = np.arange(len(idx)) % 2000 == 777
    moved = np.where(hit_, np.where(idx + 1 < len(table), idx + 1, idx - 1), idx)
    assert hit_.sum() >= 3 and np.array_equal(np.any(bits(table[moved]) != bits(table[idx]), axis=1), hit_)

    # corners 1 and 2 swapped in tu
    scene, case, rec, ref, out = hit
    assert not E.hit_check(ref, out)[2].any()
    swapped = rec.copy(); swapped[:, 1, 3], swapped[:, 2, 3] = rec[:, 2, 3], rec[:, 1, 3]
    args = (case["tri"], case["u"], case["v"], case["d"])
    bad = E.hit_check(ref, E.hit_shade_replay(swapped, *args))[2]
    moved_by = np.abs(E.hit_shade_ref(swapped, *args).tu - ref.tu)
    zero = ~np.isfinite(ref.n).all(1)
    assert np.all(bad[(moved_by > 2 * E.K_HIT * E.EPS24 * ref.tu_abs) & ~zero]) and not bad[moved_by == 0].any() and bad.mean() > 0.6
    # ... and in the normal, and a uv channel taken for the other
    swapped = rec.copy(); swapped[:, 1, :3], swapped[:, 2, :3] = rec[:, 2, :3], rec[:, 1, :3]
    assert E.hit_check(ref, E.hit_shade_replay(swapped, *args))[2].mean() > 0.6
    swapped = rec.copy(); swapped[:, :, 3], swapped[:, :, 4] = rec[:, :, 4], rec[:, :, 3]
    assert E.hit_check(ref, E.hit_shade_replay(swapped, *args))[2].mean() > 0.8

    # a normal moved by 16 bounds
    comp = np.where(zero, 0, np.argmax(np.where(np.isfinite(ref.n_abs), ref.n_abs, 0), 1))
    shift = 16 * E.K_HIT * E.EPS24 * ref.n_abs[np.arange(len(comp)), comp]
    hit_ = (np.arange(len(comp)) % 97 == 5) & ~zero & (shift > 0)
    t = out.astype(np.float64).copy(); t[hit_, comp[hit_]] += shift[hit_]
    assert hit_.sum() >= 80 and np.array_equal(E.hit_check(ref, t)[2], hit_)

    # a tonemap level moved by one, away from a boundary
    rgba, family, _, lv = tone
    lo, hi, _ = E.tonemap_ref(rgba)
    assert np.all((lv >= lo) & (lv <= hi))
    hit_ = (lo == hi) & (family == "generic") & (np.arange(lv.size).reshape(lv.shape) % 50 == 3)
    t = np.where(hit_, np.where(lv < 255, lv + 1, lv - 1), lv)
    assert hit_.sum() >= 50 and np.array_equal((t < lo) | (t > hi), hit_)

    # a direction moved by 2 ulp
    base = pkg.scenes.open_box(37, 21)
    xy, xi, _ = E.pixel_cases(37, 21)
    for family, name, c in E.camera_cases(base.camera, _centre(base))[::4]:
        cam = pkg.scenes.Camera(c["eye"], c["lookat"], c["up"], c["fovy"], 37, 21)
        origin, d = E.cast_ref(cam, _centre(base), 37, 21, xy, xi)
        got = np.concatenate([np.broadcast_to(origin, d.shape), d.astype(F32)], 1)
        assert E.cast_ratio(got, origin, d).max() <= 1
        hit_ = np.arange(len(d)) % 13 == 4
        got[hit_, 4] = E._steps(got[hit_, 4], 2)
        assert np.array_equal(E.cast_ratio(got, origin, d) > 1, hit_), name
