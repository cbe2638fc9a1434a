"""Whole paths against the oracle's event log: the `events` scene, the aimed ray families, the perturbation family and the verdict
that tests/test_path_events.py holds `probe_paths` to.  Everything here runs on the CPU and reads the oracle library alone.

The scene.  A unit box whose z = 1 side is open (a path can miss), built so that every branch of the path state machine of
csrc/wavefront.hip (wf_shade_kernel) is met by many paths: a textured floor (16 x 16 value noise, uv_scale 3), a mirror quad (Ns = 10000), a black
quad (Kd = Ks = 0: its BSDF sample has pdf 0 while its light sample is still traced), a faint emitter quad (radiance 0.004 per channel, length
0.0069: above MAT_EMIT_0 = 1e-4, below the light list's 0.01, not zero, so it is added at a first hit and at a later hit but never sampled), an
Ns = 1000 quad, an Ns = 50 sphere of 12 x 6, twelve hanging ceiling lights with a material each and one floating light quad that faces down (its
back is hit from above: `hs.front` false).  170 faces, 21 materials and 26 light triangles: more than WF_LDS_MATS = 16 and WF_LDS_LIGHTS = 8, so
the shade kernel reads both tables from global memory.  What is chosen so that the list meets the conditions of test_path_events.py:
  * every light hangs in a plane of its own, 4e-3 apart: a vertex ON a light that samples a light of the same plane gets the cosine 0.0f exactly
    and with it `pdf == 0`, a verdict that any shift of the vertex turns over (such a path is never decided), and nearly coplanar lights send
    shadow rays along each other's planes (spacing 5e-4: 25 % of the list undecided);
  * they hang 0.1 below the ceiling: at 1e-3 below it, a light sample taken from the ceiling grazes the ceiling itself and a hit point 1e-6
    behind it is shadowed (3.7 % of the random rays undecided at depth 1);
  * radiances of 1.5 ... 4.25: a wall point near a light's plane sees it at a cosine of 1e-2 and its NEE term moves by 1e-4 of itself with a
    1e-6 shift, so at radiances of 6 ... 17 4.5 % of the paths have S_i above the 1e-4 bound (most |L| are then above 1, where the bound is
    relative); walls of albedo 0.85 so that enough paths live to the roulette and the depth limit.
The families: `interior` (4000 random rays) and seven aimed ones, which exist to make the rare events frequent -- random rays alone give a few
dozen mirror-to-light terms: `at_lights` (fronts of the ceiling lights and of the floating light, its back from above, the faint quad),
`at_mirror` (anywhere on it; chains mirror -> ceiling light, mirror -> the floating light's front, mirror -> its back), `at_black`, `at_glossy`
(the Ns = 1000 quad and the sphere), `outward` (through the open side, a third from outside the box), `grazing` (floor hits at a cosine of
1e-3 ... 1e-1) and `deep` (from the back half towards the back: the long paths).

The perturbation family (oracle/mcpt_oracle.cpp, PathAux).  Each magnitude restates a freedom the device is documented to have:
  dp = 2^-20 x the scene's extent.  The device keeps a ray origin and every hit point in fp32 (wavefront.hip: "the fp32 origin `no` is what
       travels", `p32 = to_f3(p64)`), at most 2^-24 of a coordinate each, and an unbounded path has about 20 vertices.
  dd = 1.91e-6 = 4 K 2^-23 (|q| + 1), the bound of tests/shade_ref.py on a sampled direction of a diffuse or mirror pick; a Phong pick gets its
       own budget, that plus 9.5e-7 / max(sin theta, 2^-12) (shade_ref.py's D_q), which the oracle applies as dd (1 + 0.5 / max(sin theta, 2^-12)).
  db = 2^-20: a vertex's throughput factor f cos / pdf is a handful of fp32 products and one v_rcp_f32 (1 ulp), and the path multiplies about
       20 of them.
Members: six that shift every point, turn every direction along +-x, +-y, +-z and scale every factor up (+) or down (-); N_HASHED whose shifts,
turns and signs are hashed from (item, bounce, member); and one hashed member for each magnitude alone.  A member is added only with such a
citation, never to make a failing device path pass.

The verdict.  A path is DECIDED when the plain run and every member give the same event log (and the log holds the whole path).  Its sensitivity
S_i is the largest |L_member - L_plain| over members and channels, its allowance max(1e-4 max(1, |L_i|), S_i) per channel -- 1e-4 is the per-path
bound of test_probe_paths_vs_oracle, not tightened here.  A decided path outside its allowance fails; an undecided one must be finite and >= 0
-- or, where the oracle's own family goes below zero (a light sampled from behind has a negative pdf, SURVEY A-8, and the floating light and the
hanging ceiling lights are seen from behind by design), not below the family's lowest answer less the 1e-4 bound.

MCPT_FLAG_CORRECT_SHADOW_T2 is set throughout: without it the reference's self-occlusion verdict is fp64 noise by design (SURVEY A-9), which
test_self_occlusion_rate_matches_oracle covers statistically.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

SEED = 42
DEPTHS = (1, 2, 4, 5, 6, 0)
REL = 1e-4                                                  # test_probe_paths_vs_oracle's per-path bound
DD = 4 * 2.0 * 2.0 ** -23 * 2.0                             # shade_ref: 4 K 2^-23 (|q| + 1), K = K_ORACLE = 2, |q| <= 1: 1.907e-6
DB = 2.0 ** -20
N_HASHED = 8
MAX_UNDECIDED, MAX_SENSITIVE, MIN_EVENTS = 0.05, 0.02, 200

NEE = ("nee_nopdf", "nee_blocked", "nee_added")
LOBE = ("lobe_diffuse", "lobe_phong", "lobe_mirror", "lobe_pdf0")
EMIT = ("emit_none", "emit_mis", "emit_mirror")
END = ("end_miss0", "end_miss", "end_pdf0", "end_roulette", "end_depth")
FAMILIES = (("interior", 4000), ("at_lights", 3600), ("at_mirror", 1800), ("at_black", 800), ("at_glossy", 600), ("outward", 600), ("grazing", 300), ("deep", 1200))

# quads of the scene: (corner, edge u, edge v, normal)
MIRROR_Q = ((0.55, 0.3, 0.01), (0.4, 0, 0), (0, 0.5, 0), (0, 0, 1))
BLACK_Q = ((0.01, 0.3, 0.2), (0, 0, 0.4), (0, 0.4, 0), (1, 0, 0))
FAINT_Q = ((0.99, 0.55, 0.2), (0, 0, 0.3), (0, 0.3, 0), (-1, 0, 0))
GLOSS_Q = ((0.99, 0.1, 0.5), (0, 0, 0.4), (0, 0.35, 0), (-1, 0, 0))
FLOAT_Q = ((0.1, 0.6, 0.55), (0.2, 0, 0), (0, 0, 0.2), (0, -1, 0))
SPHERE = ((0.38, 0.25, 0.4), 0.2)
LIGHT_SIZE = 0.14
RAD_SCALE = 0.25
N_FRONT = (1600, 800)
WALLS = ((0.85, 0.83, 0.8), (0.8, 0.25, 0.2), (0.25, 0.75, 0.2))
LIGHT_Y0, LIGHT_DY = 0.9, 0.004


def ceiling_lights():
    """(corner, edge u, edge v, normal) of the twelve ceiling lights: a 4 x 3 grid, light k at y = 0.9 - 0.004 k (well below the ceiling: a light
    sample taken from the ceiling does not graze it)."""
    out = []
    for k in range(12):
        cx, cz = 0.125 + 0.25 * (k % 4), 1.0 / 6 + (k // 4) / 3.0
        out.append(((cx - LIGHT_SIZE / 2, LIGHT_Y0 - LIGHT_DY * k, cz - LIGHT_SIZE / 2), (LIGHT_SIZE, 0, 0), (0, 0, LIGHT_SIZE), (0, -1, 0)))
    return out


def _add(m, q, mat):
    o, du, dv, n = (np.asarray(x, float) for x in q)
    m.add_quad(o, o + du, o + du + dv, o + dv, tuple(n), mat)


def events_scene(pkg, width=32, height=32):
    sc = pkg.scenes
    M = sc.Material
    mats = [M("white", kd=WALLS[0]), M("red", kd=WALLS[1]), M("green", kd=WALLS[2]),
            M("floor", kd=(0.6, 0.6, 0.6), map_kd="floor.ppm", texture=sc.value_noise_texture(16, 7, (0.7, 0.65, 0.6))),
            M("mirror", kd=(0.0, 0.0, 0.0), ks=(1.0, 1.0, 1.0), ns=10000.0), M("black"),
            M("faint", kd=(0.5, 0.5, 0.5), radiance=(0.004, 0.004, 0.004)), M("gloss1000", kd=(0.2, 0.25, 0.3), ks=(0.6, 0.55, 0.5), ns=1000.0),
            M("glossy", kd=(0.3, 0.3, 0.3), ks=(0.5, 0.5, 0.5), ns=50.0)]
    WHITE, RED, GREEN, FLOOR, MIRROR, BLACK, FAINT, GLOSS, GLOSSY = range(9)
    for k in range(12):
        mats.append(M("light%d" % k, kd=(0.65, 0.65, 0.65), radiance=tuple(RAD_SCALE * c for c in (6.0 + k, 5.0 + 0.5 * k, 4.0 - 0.25 * k))))
    m = sc._Mesh()
    m.add_grid((0, 0, 0), (1, 0, 0), (0, 0, 1), 2, 2, (0, 1, 0), FLOOR, uv_scale=3.0)
    m.add_grid((0, 1, 0), (1, 0, 0), (0, 0, 1), 1, 1, (0, -1, 0), WHITE)
    m.add_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), 1, 1, (0, 0, 1), WHITE)
    m.add_grid((0, 0, 0), (0, 0, 1), (0, 1, 0), 1, 1, (1, 0, 0), RED)
    m.add_grid((1, 0, 0), (0, 0, 1), (0, 1, 0), 1, 1, (-1, 0, 0), GREEN)
    _add(m, MIRROR_Q, MIRROR); _add(m, BLACK_Q, BLACK); _add(m, FAINT_Q, FAINT); _add(m, GLOSS_Q, GLOSS)
    m.add_uv_sphere(SPHERE[0], SPHERE[1], 12, 6, GLOSSY)
    for k, q in enumerate(ceiling_lights()):
        _add(m, q, 9 + k)
    _add(m, FLOAT_Q, 9)                                                                 # the floating light shares light0's material
    cam = sc._qcam((0.5, 0.5, 2.3), (0.5, 0.5, 0.0), (0, 1, 0), 40.0, width, height)
    scene = m.finish("events", mats, cam, {"kind": "events"})
    assert scene.n_faces == 170 and len(mats) == 21
    return scene


# ------------------------------------------------------------------------------------------------------------------------ rays
def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _on(rng, q, n, margin=0.05):
    o, du, dv, _ = (np.asarray(x, float) for x in q)
    s, t = rng.uniform(margin, 1 - margin, (2, n, 1))
    return o + s * du + t * dv


def _inside(rng, n, lo=(0.05, 0.05, 0.05), hi=(0.95, 0.95, 0.95)):
    return rng.uniform(lo, hi, (n, 3))


def _aim(o, t):
    d = t - o
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


def _via_mirror(rng, target, n, above=None):
    """Rays whose mirror image about the mirror's plane points at `target` points: they reach the mirror at M and leave it towards the target."""
    M = _on(rng, MIRROR_Q, n)
    if above is not None:
        M[:, 1] = rng.uniform(above[0], above[1], n)
    T = target
    back = np.stack([M[:, 0] - T[:, 0], M[:, 1] - T[:, 1], T[:, 2] - M[:, 2]], -1)       # towards where the ray comes from
    back /= np.linalg.norm(back, axis=1, keepdims=True)
    s = rng.uniform(0.1, 0.5, (n, 1))
    for _ in range(6):                                                                 # keep the origin inside the box
        o = M + s * back
        out = np.any((o < 0.02) | (o > 0.98), axis=1, keepdims=True)
        s = np.where(out, s * 0.5, s)
    return M + s * back, -back


def ray_families(seed=2026):
    """[(family, origins, directions)] in the order of FAMILIES; the same list every time."""
    rng = np.random.default_rng(seed)
    n = dict(FAMILIES)
    lights = ceiling_lights()
    out = []
    out.append(("interior",) + (_inside(rng, n["interior"]), _unit(rng, n["interior"])))
    # at_lights: N_FRONT fronts (the ceiling lights from below, the floating light's underside), 600 at the floating light's back from
    # above, 600 at the faint quad
    parts = []
    k = rng.integers(0, 12, N_FRONT[0])
    t = np.concatenate([_on(rng, lights[i], 1) for i in k])
    parts.append(_aim(_inside(rng, N_FRONT[0], hi=(0.95, 0.8, 0.95)), t))
    parts.append(_aim(_inside(rng, N_FRONT[1], lo=(0.05, 0.05, 0.4), hi=(0.5, 0.5, 0.9)), _on(rng, FLOAT_Q, N_FRONT[1])))
    parts.append(_aim(_inside(rng, 600, lo=(0.05, 0.7, 0.4), hi=(0.45, 0.95, 0.9)), _on(rng, FLOAT_Q, 600)))
    parts.append(_aim(_inside(rng, 600), _on(rng, FAINT_Q, 600)))
    out.append(("at_lights", np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])))
    # at_mirror: 600 anywhere on it, 600 mirror -> ceiling light, 300 mirror -> the floating light's underside, 300 mirror -> its back
    parts = [_aim(_inside(rng, 600, lo=(0.05, 0.05, 0.2)), _on(rng, MIRROR_Q, 600))]
    k = rng.integers(0, 12, 600)
    parts.append(_via_mirror(rng, np.concatenate([_on(rng, lights[i], 1) for i in k]), 600))
    parts.append(_via_mirror(rng, _on(rng, FLOAT_Q, 300), 300, above=(0.32, 0.5)))
    parts.append(_via_mirror(rng, _on(rng, FLOAT_Q, 300), 300, above=(0.68, 0.78)))
    out.append(("at_mirror", np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])))
    out.append(("at_black",) + _aim(_inside(rng, n["at_black"], lo=(0.1, 0.05, 0.05)), _on(rng, BLACK_Q, n["at_black"])))
    c, r = np.asarray(SPHERE[0]), SPHERE[1]
    parts = [_aim(_inside(rng, 300, hi=(0.9, 0.95, 0.95)), _on(rng, GLOSS_Q, 300)),
             _aim(_inside(rng, 300, lo=(0.05, 0.5, 0.05)), c + 0.8 * r * _unit(rng, 300))]
    out.append(("at_glossy", np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])))
    # outward: through the open z = 1 side; a third of them from outside the box, looking away
    o = _inside(rng, n["outward"]); t = np.stack([rng.uniform(0.02, 0.98, n["outward"]), rng.uniform(0.02, 0.98, n["outward"]), np.ones(n["outward"])], -1)
    o[::3, 2] += 1.0; t[::3, 2] = 3.0
    out.append(("outward",) + _aim(o, t))
    # grazing: floor hits whose cosine is between 1e-3 and 1e-1 (log-uniform)
    m = n["grazing"]
    p = np.stack([rng.uniform(0.1, 0.9, m), np.zeros(m), rng.uniform(0.1, 0.9, m)], -1)
    cosv = 10.0 ** rng.uniform(-3, -1, m); phi = rng.uniform(0, 2 * np.pi, m)
    d = np.stack([np.sqrt(1 - cosv * cosv) * np.cos(phi), -cosv, np.sqrt(1 - cosv * cosv) * np.sin(phi)], -1)
    s = rng.uniform(0.02, 0.3, (m, 1))
    for _ in range(6):
        o = p - s * d
        bad = np.any((o < 0.02) | (o > 0.98), axis=1, keepdims=True) & (o[:, 1:2] > 0)
        bad |= np.any((o[:, [0, 2]] < 0.02) | (o[:, [0, 2]] > 0.98), axis=1, keepdims=True)
        s = np.where(bad, s * 0.5, s)
    out.append(("grazing", p - s * d, d))
    # deep: from the back half of the box towards its back: the paths that live long enough for the roulette and the depth limit
    back = _unit(rng, n["deep"]); back[:, 2] = -np.abs(back[:, 2])
    out.append(("deep", _inside(rng, n["deep"], hi=(0.95, 0.95, 0.5)), back))
    assert [f for f, _, _ in out] == [f for f, _ in FAMILIES] and all(o.shape == (n[f], 3) and d.shape == o.shape for f, o, d in out)
    return out


# ------------------------------------------------------------------------------------------------------------------------ the log
def decode(row):
    """One path's log as a list of vertex tuples (face, front, nee, lobe, emit, roulette passed, next face or -1, next front) and (end, vertices)."""
    end, nv = int(row[0]), int(row[1])
    vs = []
    for k in range(min(nv, (len(row) - 2) // 2)):
        a, b = int(row[2 + 2 * k]), int(row[3 + 2 * k])
        vs.append((a >> 8, (a >> 7) & 1, a & 3, (a >> 2) & 3, (a >> 4) & 3, (a >> 6) & 1, -1 if b < 0 else b >> 1, 0 if b < 0 else b & 1))
    return vs, (end, nv)


def describe(row):
    vs, (end, nv) = decode(row)
    txt = ["f%d%s nee=%s %s%s%s" % (f, "+" if fr else "-", NEE[nee][4:], LOBE[lobe][5:], " emit=" + EMIT[em][5:] if em else "", " rr" if rr else "")
           + (" -> f%d%s" % (nf, "+" if nfr else "-") if nf >= 0 else "") for f, fr, nee, lobe, em, rr, nf, nfr in vs]
    return "[" + "; ".join(txt) + "] " + END[end][4:] + " after %d" % nv


def event_counts(ev, emissive_face, mask):
    """How often each event kind occurs over the paths `mask` selects (plain run's log `ev`)."""
    e = ev[mask]
    nv = np.minimum(e[:, 1], (e.shape[1] - 2) // 2)
    A, B = e[:, 2::2], e[:, 3::2]
    live = np.arange(A.shape[1])[None, :] < nv[:, None]
    c = {}
    c["front"] = int((live & ((A >> 7) & 1 == 1)).sum()); c["back"] = int((live & ((A >> 7) & 1 == 0)).sum())
    for k, name in enumerate(NEE): c[name] = int((live & ((A & 3) == k)).sum())
    for k, name in enumerate(LOBE): c[name] = int((live & (((A >> 2) & 3) == k)).sum())
    traced = live & (((A >> 2) & 3) != 3) & (B >= 0)                                     # a continuation ray that hit something
    for k, name in enumerate(EMIT): c[name] = int((traced & (((A >> 4) & 3) == k)).sum())
    for k, name in enumerate(END): c[name] = int((e[:, 0] == k).sum())
    c["roulette_pass"] = int((live & ((A >> 6) & 1 == 1)).sum())
    c["pdf0_with_nee_added"] = int((live & (((A >> 2) & 3) == 3) & ((A & 3) == 2)).sum())
    last = A[np.arange(len(e)), np.maximum(nv - 1, 0)]
    c["miss_after_nee_added"] = int(((e[:, 0] == 1) & (nv > 0) & ((last & 3) == 2)).sum())
    nf = np.where(B >= 0, B >> 1, 0)
    c["backface_emitter_hit"] = int((traced & emissive_face[nf] & ((B & 1) == 0)).sum())
    return c


def required_kinds(depth):
    """The kinds a list must hold MIN_EVENTS times at this depth: all of them, less what the depth rules out -- the roulette starts at the
    fifth vertex (bounces > 3), so depths 1, 2 and 4 neither pass nor end by it, and an unbounded path never ends by depth."""
    kinds = ["front", "back"] + list(NEE) + list(LOBE) + list(EMIT) + list(END) + ["roulette_pass", "pdf0_with_nee_added", "miss_after_nee_added", "backface_emitter_hit"]
    if depth in (1, 2, 4): kinds = [k for k in kinds if k not in ("end_roulette", "roulette_pass")]
    if depth == 0: kinds.remove("end_depth")
    return kinds


# ------------------------------------------------------------------------------------------------------------------------ the verdict
def members(extent):
    """The perturbation family: keyword arguments of Oracle.trace_paths_log, one dict per member."""
    dp = 2.0 ** -20 * extent
    out = [dict(dp=dp, dd=DD, db=DB, axis=a, member=a) for a in range(6)]
    out += [dict(dp=dp, dd=DD, db=DB, axis=-1, member=6 + k) for k in range(N_HASHED)]
    out += [dict(dp=dp, axis=-1, member=100), dict(dd=DD, axis=-1, member=101), dict(db=DB, axis=-1, member=102)]
    return out


def judge(oracle, scene, o, d, depth, flags, family=None, seed=SEED):
    """The plain run and the family for one depth: L, log, decided, S, allowance (n, 3)."""
    oracle.set_opts(max_depth=depth, integrator=0, flags=flags)
    used = scene.vertex[np.unique(scene.face[:, :, 0])]
    extent = float((used.max(0) - used.min(0)).max())
    L, ev = oracle.trace_paths_log(o, d, seed=seed)
    decided = ev[:, 1] <= (ev.shape[1] - 2) // 2                                         # the log holds the whole path
    S = np.zeros(len(L)); low = np.minimum(np.nan_to_num(L.astype(np.float64)), 0.0)
    for kw in members(extent):
        Lm, evm = oracle.trace_paths_log(o, d, seed=seed, **kw)
        decided &= np.all(evm == ev, axis=1)
        with np.errstate(invalid="ignore"):
            dl = np.abs(Lm.astype(np.float64) - L.astype(np.float64)).max(1)
        S = np.maximum(S, np.where(np.isfinite(dl), dl, np.inf)); low = np.minimum(low, np.nan_to_num(Lm.astype(np.float64)))
    L64 = L.astype(np.float64)
    decided &= np.all(np.isfinite(L64), axis=1)
    floor = REL * np.maximum(1.0, np.abs(L64))
    return SimpleNamespace(depth=depth, L=L, L64=L64, ev=ev, decided=decided, S=S, floor=floor, low=low - floor, allow=np.maximum(floor, S[:, None]),
                           sensitive=np.any(S[:, None] > floor, axis=1), family=family)


def check(j, got):
    """`got` (n, 3) presented as the device's answer to the paths of `j`: (indices of failing paths, deviation / allowance (n,), deviation /
    max(1, |L|) (n,)).  A decided path fails outside its allowance, any path fails where it is not finite or below `low`: zero, or the most negative
    answer of the oracle's own family less the 1e-4 bound (a light sampled from behind has a negative pdf and subtracts, SURVEY A-8)."""
    g = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        dev = np.abs(g - j.L64)
        ratio = np.where(j.decided, np.nan_to_num((dev / j.allow).max(1), nan=np.inf), 0.0)
        rel = np.where(j.decided, np.nan_to_num((dev / np.maximum(1.0, np.abs(j.L64))).max(1), nan=np.inf), 0.0)
        wrong = ~np.all(np.isfinite(g) & (g >= j.low), axis=1)
    return np.nonzero((ratio > 1.0) | wrong)[0], ratio, rel


def message(j, got, bad, limit=5):
    fam = j.family if j.family is not None else ["?"] * len(j.L)
    return "depth %d: %d paths outside their allowance; " % (j.depth, len(bad)) + " | ".join(
        "path %d (%s) got %r want %r allowance %r S %.3g %s: %s" % (i, fam[i], np.asarray(got[i]).tolist(), j.L[i].tolist(), j.allow[i].tolist(), j.S[i],
                                                                  "decided" if j.decided[i] else "undecided", describe(j.ev[i])) for i in bad[:limit])


def family_table(j, ratio, rel):
    """Per family: paths, undecided, worst deviation / allowance, worst deviation / max(1, |L|) among decided paths."""
    fam = np.asarray(j.family)
    return [(f, int((fam == f).sum()), int((~j.decided[fam == f]).sum()), float(ratio[fam == f].max()), float(rel[fam == f].max())) for f, _ in FAMILIES]
