"""CPU: the restatement of the bake stage's direct-light mode (tests/bake_direct_ref.py) -- the float32 slack S that sizes
the device's bound, the share of rows the comparisons leave out, the estimator's properties in float64, the generator against the oracle's, the struct's layout through a C compiler.  No device is touched."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import bake_direct_ref as D, bake_ref as R, deform_kit as K, kit, shade_ref

NEW_SYMBOLS = ["mcpt_set_bake_direct", "mcpt_probe_bake_direct"]
METHODS = ["set_bake_direct", "probe_bake_direct"]
INVALID = 1
RADIANCE = np.array([17.0, 12.0, 4.0])


def _runs(pkg):
    """Both runs of the restatement over the device test's inputs, row by row: (r64 columns, r32 columns, ill, unsure) concatenated."""
    scene = D.centred_box(pkg, black=True)
    centre = np.zeros(3)
    rows = []
    for pts, sample in D.box_lists(pkg, scene):
        P, N, d, dead, xi = D.cpu_rays(scene, centre, pts, sample, D.SEED)
        r64 = D.terms(scene, centre, P, N, d, xi, np.float64, dead); r32 = D.terms(scene, centre, P, N, d, xi, np.float32, dead)
        rows.append((r64, r32, D.unsure_rows(scene, centre, P, d, r64, r32)))
    return rows


def test_library_exports_the_direct_light_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, METHODS)
    assert (pkg.BAKE_DIRECT_OFF, pkg.BAKE_DIRECT_MIS) == (0, 1)
    lib = pkg.load_library()
    assert lib.mcpt_set_bake_direct(None, 0) == INVALID and lib.mcpt_probe_bake_direct(None, 0, 0, 0, 1, None, None) == INVALID


def test_bake_info_keeps_its_layout_and_names_the_mode(pkg, tmp_path):
    """mcpt_bake_info as a C compiler sees include/mcpt.h: still 56 bytes, direct_mode at reserved[0]'s offset, the constants the header's;
    BakeInfo.direct_mode reads that word."""
    class Named(C.Structure):                                                   # the header's view with the word named
        _fields_ = [("struct_size", C.c_uint32), ("n_points", C.c_uint32), ("n_dead", C.c_uint32), ("bakes", C.c_uint32), ("passes", C.c_uint64),
                    ("last_stage_ms", C.c_double), ("device_bytes", C.c_uint64), ("direct_mode", C.c_uint32)]
    macros = ["MCPT_BAKE_DIRECT_OFF", "MCPT_BAKE_DIRECT_MIS"] + ["MCPT_BAKE_DIRECT_STATE_" + s for s in ("DEAD", "NO_PDF", "BELOW", "OCCLUDED", "COUNTED")]
    c, py, consts = K.c_layout(Named, "mcpt_bake_info", tmp_path, macros)
    assert c[0] == 56 == C.sizeof(pkg.BakeInfo) and c[1:] == py[1:]
    assert c[-1] == pkg.BakeInfo.reserved.offset == 40
    assert consts == [pkg.BAKE_DIRECT_OFF, pkg.BAKE_DIRECT_MIS, D.DEAD, D.NO_PDF, D.BELOW, D.OCCLUDED, D.COUNTED]
    info = pkg.BakeInfo(); info.reserved[0] = 1
    assert info.direct_mode == 1 and info.as_dict()["direct_mode"] == 1


def test_generator_is_the_oracles(orc):
    """bake_direct_ref.rng_block against the oracle's counter_block (which tests/test_gpu_parity.py holds the device's rng_block to), bit for
    bit: blocks 0 and 0xFFFFFFFF, items at both ends of their range, seeds with and without a high word."""
    for seed in (0, D.SEED, 7 + (1 << 32), 2 ** 64 - 1):
        for sample in (0, 1, 7, 2 ** 32 - 1):
            for block in (0, 1, D.DIRECT_BLOCK):
                items = np.array([0, 1, 63, 64, 999, 65535, 0x3fffffe, 2 ** 32 - 1], np.uint32)
                got = D.rng_block(items, sample, block, seed)
                want = np.array([orc.Oracle.rng_block(int(i), sample, block, seed) for i in items])
                assert np.array_equal(kit.bits(got), kit.bits(want)), (seed, sample, block)


def test_float32_slack(pkg):
    """S: the worst difference between the float32 and the float64 run over the device test's own inputs, on well-conditioned rows both runs
    agree on, per class in its unit; BOUND, what the device is allowed, is 4 S rounded up to a power of two.  The states agree on every kept row."""
    worst = {"radiance": 0.0, "weight": 0.0, "pdf": 0.0}
    n = kept = 0
    for r64, r32, unsure in _runs(pkg):
        keep = ~(r64.ill | unsure) & (r64.state != D.DEAD)
        assert np.array_equal(r64.state[keep], r32.state[keep]) and np.array_equal(r64.hit_face[keep], r32.hit_face[keep])
        assert np.array_equal(r64.light_face, r32.light_face)
        for k, x in D.worst_units(r32, r64, keep).items():
            worst[k] = max(worst[k], x)
        n += len(keep); kept += int(keep.sum())
    S = max(worst.values())
    bound = 2.0 ** np.ceil(np.log2(4.0 * S))
    print("%d rows, %d kept; S per class: %s; S = %.2f, 4 S = %.1f, BOUND = %g" % (n, kept, ", ".join("%s %.2f" % kv for kv in worst.items()), S, 4 * S, bound))
    assert n == 3 * sum(D.LENGTHS)
    assert abs(S - D.S_CPU) < 0.01 and bound == D.BOUND, "tests/bake_direct_ref.py states S = %.2f and BOUND = %g" % (D.S_CPU, D.BOUND)


def test_exclusion_cap(pkg):
    """The share of rows the comparisons leave out -- ill conditioned or unsure -- over the device test's inputs: at most 2 %, per list of 257
    points or more and over all rows.  Every state the convex box can show and both kinds of `sub` occur among the kept rows."""
    out = total = 0
    states = np.zeros(5, np.int64); mis = behind = 0
    for r64, r32, unsure in _runs(pkg):
        left = (r64.ill | unsure)
        if len(left) >= 257:
            assert left.mean() <= D.EXCLUSION_CAP, "%d of %d rows" % (left.sum(), len(left))
        out += int(left.sum()); total += len(left)
        states += np.bincount(r64.state[~left], minlength=5)
        mis += int((r64.mis & ~left).sum()); behind += int((~left & ~r64.mis & (r64.sub != 0).any(1)).sum())
    print("left out: %d of %d rows (%.3f %%); kept states dead..counted %s; lights met from the front %d, emitters from behind %d" % (out, total, 100.0 * out / total, states, mis, behind))
    assert out / total <= D.EXCLUSION_CAP
    # (the open box is convex: nothing in it occludes; OCCLUDED is met on nine_light_scene, whose sphere does -- see test_occlusion_on_nine_lights)
    assert (states[[D.NO_PDF, D.BELOW, D.COUNTED]] > 0).all() and mis > 0 and behind > 0


def test_occlusion_on_nine_lights(pkg):
    """nine_light_scene, whose sphere stands between many points and lights: among 600 interior points every state occurs, both runs agree on
    every kept row's state, and at most 2 % of the rows are left out."""
    scene = shade_ref.nine_light_scene(pkg, 16, 16)
    used = scene.vertex[np.unique(scene.face[:, :, 0])]
    centre = 0.5 * used.min(0) + 0.5 * used.max(0)
    pts = D.interior_points(pkg, scene, 600)
    P, N, d, dead, xi = D.cpu_rays(scene, centre, pts, 0, D.SEED)
    r64 = D.terms(scene, centre, P, N, d, xi, np.float64, dead); r32 = D.terms(scene, centre, P, N, d, xi, np.float32, dead)
    left = r64.ill | D.unsure_rows(scene, centre, P, d, r64, r32)
    print("left out: %d of %d rows; states %s" % (left.sum(), len(left), np.bincount(r64.state, minlength=5)))
    assert left.mean() <= D.EXCLUSION_CAP and np.array_equal(r64.state[~left], r32.state[~left])
    assert (np.bincount(r64.state[~left], minlength=5)[1:] > 0).all() and len(r64.lights) == 9


def _floor_centre(scene):
    p0 = scene.vertex[scene.face[0, :, 0]]
    return p0[0] + 0.5 * (p0[2] - p0[0])


def test_weights_of_one_direction_sum_to_one(pkg):
    """A floor point straight below (u, v) = (0.25, 0.25) of the lamp's first triangle, the lamp moved to a height that is an fp32 value (the
    light sample holds its two points in fp32, the cosine ray's hit distance is not rounded): the direction (0, 1, 0) and the distance are then
    the same numbers on both ways to that place, and w_b + w_l = 1 to 1e-12."""
    scene = D.centred_box(pkg, black=True)
    lamp = np.unique(scene.face[shade_ref.light_faces(scene)][:, :, 0])
    v = scene.vertex.copy(); v[lamp, 1] = 0.5 - 2.0 ** -10
    scene = kit.with_arrays(pkg, scene, vertex=v)
    c = scene.vertex[scene.face[shade_ref.light_faces(scene)[0], :, 0]]
    q = ((0.5 * c[0] + 0.25 * c[1]) + 0.25 * c[2]).astype(np.float32).astype(np.float64)
    P = np.array([[q[0], _floor_centre(scene)[1], q[2]]]); N = np.array([[0.0, 1.0, 0.0]])
    r = D.terms(scene, np.zeros(3), P, N, np.array([[0.0, 1.0, 0.0]]), np.array([[0.0, 0.25, 0.25]], np.float32))
    assert r.state[0] == D.COUNTED and r.mis[0] and np.array_equal(r.wo[0], [0.0, 1.0, 0.0])
    assert r.hit_face[0] == r.light_face[0] == shade_ref.light_faces(scene)[0]
    print("w_b = %.15f, w_l = %.15f, sum - 1 = %.2e; p_b = %.6f, p_l = %.6f" % (r.w_b[0], r.w_l[0], r.w_b[0] + r.w_l[0] - 1, r.p_b[0], r.p_l[0]))
    assert abs(r.w_b[0] + r.w_l[0] - 1.0) <= 1e-12 and 0 < r.w_b[0] < 1
    assert np.allclose(r.sub[0], (1 - r.w_b[0]) * RADIANCE, rtol=1e-12) and np.allclose(r.add[0], r.w_l[0] * RADIANCE * r.p_bl[0] / r.p_lf[0], rtol=1e-12)


def _two_strategy_quadrature(scene, g):
    """The expectation of the floor centre's record in the black-walled box by a g x g midpoint rule over the lamp: the light strategy's
    mean of `add` plus the cosine strategy's share w_b Le p_b dw of the same places."""
    P = _floor_centre(scene); N = np.array([0.0, 1.0, 0.0])
    x0, x1, z0, z1, y = D.lamp_rect(scene)
    s = (np.arange(g) + 0.5) / g
    X, Z = np.meshgrid(x0 + s * (x1 - x0), z0 + s * (z1 - z0), indexing="ij")
    q = np.stack([X.ravel(), np.full(g * g, y), Z.ravel()], 1)
    lf = shade_ref.light_faces(scene)
    xi = np.zeros((g * g, 3), np.float32); area = np.zeros(g * g)
    done = np.zeros(g * g, bool)
    for k, f in enumerate(lf):                                                   # each cell's centre in the barycentrics of the triangle that holds it
        c = scene.vertex[scene.face[f, :, 0]]
        uv, *_ = np.linalg.lstsq(np.stack([c[1] - c[0], c[2] - c[0]], 1), (q - c[0]).T, rcond=None)
        inside = ~done & (uv[0] >= -1e-12) & (uv[1] >= -1e-12) & (uv[0] + uv[1] <= 1 + 1e-12)
        xi[inside, 0] = (k + 0.5) / len(lf); xi[inside, 1] = np.clip(uv[0][inside], 0, 1); xi[inside, 2] = np.clip(uv[1][inside], 0, 1)
        area[inside] = 0.5 * np.linalg.norm(np.cross(c[1] - c[0], c[2] - c[0]))
        done |= inside
    assert done.all()
    over = xi[:, 1].astype(np.float64) + xi[:, 2].astype(np.float64) > 1.0          # (rounding on the shared edge: keep the pair unfolded)
    xi[over, 2] = np.nextafter(xi[over, 2], np.float32(0))
    n = g * g
    Pn, Nn = np.tile(P, (n, 1)), np.tile(N, (n, 1))
    light = D.terms(scene, np.zeros(3), Pn, Nn, np.tile([0.0, 1.0, 0.0], (n, 1)), xi)
    # (a cell centre on the lamp's diagonal lies in BOTH lamp triangles: the one that was not sampled may occlude it at t = t2.  The integrand is
    # therefore built from the weights and pdfs, which states OCCLUDED and COUNTED both report; off the diagonal every sample counts.)
    assert (light.state >= D.OCCLUDED).all() and (light.state == D.OCCLUDED).sum() <= g
    counted = light.state == D.COUNTED
    assert np.allclose(light.add[counted], ((light.w_l * light.p_bl / light.p_lf)[:, None] * RADIANCE[None])[counted], rtol=1e-13, atol=0)
    cosine = D.terms(scene, np.zeros(3), Pn, Nn, light.wo, xi)                      # the cosine ray along each cell's direction
    assert cosine.mis.all()
    dA = (x1 - x0) * (z1 - z0) / n
    weight = dA / (len(lf) * area)                                               # area-measure pdf of the light strategy times the cell
    e_light = ((light.w_l * light.p_bl / light.p_lf * weight)[:, None] * RADIANCE[None]).sum(0)
    e_cosine = ((cosine.w_b * light.p_bl / light.p_lf * weight)[:, None] * RADIANCE[None]).sum(0)
    return e_light + e_cosine, e_light, P, (x0, x1, z0, z1, y)


def test_two_strategies_integrate_to_the_form_factor(pkg):
    """Quadrature of the two-strategy estimator at the floor's centre under the black-walled box's lamp, 256 x 256 cells: F Le, F the analytic
    form factor, within the quadrature's own error -- the difference between the 256 and the 128 grid."""
    scene = D.centred_box(pkg, black=True)
    q256, light, P, (x0, x1, z0, z1, y) = _two_strategy_quadrature(scene, 256)
    q128 = _two_strategy_quadrature(scene, 128)[0]
    F = R.form_factor_rect(x0 - P[0], x1 - P[0], z0 - P[2], z1 - P[2], y - P[1])
    err = np.abs(q256 - q128)
    print("F = %.9f; F Le = %s, quadrature %s, off by %s, allowed %s; the light strategy carries %.1f %%" % (F, F * RADIANCE, q256, q256 - F * RADIANCE, err, 100 * light[0] / q256[0]))
    assert (np.abs(q256 - F * RADIANCE) <= err).all() and (err < 1e-4 * F * RADIANCE).all()


def test_points_that_cannot_be_lit_get_exactly_nothing(pkg):
    """A point in the lamp's plane (the cosine at the light is exactly 0: state NO_PDF) and a back-side point whose hemisphere holds no light
    (state BELOW) get add = 0 exactly, in both types."""
    scene = D.centred_box(pkg, black=True)
    x0, x1, z0, z1, y = D.lamp_rect(scene)
    rng = np.random.default_rng(D.SEED)
    n = 500
    xi = rng.integers(0, 1 << 24, (n, 3)).astype(np.float32) / np.float32(1 << 24)
    in_plane = np.stack([rng.uniform(-0.5, 0.5, n), np.full(n, y), rng.uniform(-0.5, 0.5, n)], 1)
    outside = (in_plane[:, 0] < x0) | (in_plane[:, 0] > x1) | (in_plane[:, 2] < z0) | (in_plane[:, 2] > z1)
    below = np.tile(_floor_centre(scene), (n, 1))
    d = np.tile([0.0, -1.0, 0.0], (n, 1))
    for T in (np.float64, np.float32):
        r = D.terms(scene, np.zeros(3), in_plane, np.tile([0.0, -1.0, 0.0], (n, 1)), d, xi, T)
        assert (r.state[outside] == D.NO_PDF).all() and (r.add == 0).all() and (r.w_l == 0).all() and outside.sum() > 300
        r = D.terms(scene, np.zeros(3), below, np.tile([0.0, -1.0, 0.0], (n, 1)), d, xi, T)
        assert (r.state == D.BELOW).all() and (r.add == 0).all() and (r.sub == 0).all()
