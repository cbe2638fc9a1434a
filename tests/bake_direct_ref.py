"""Plain numpy restatement of the bake stage's direct-light mode (bk_direct in csrc/bake.hip, DESIGN.md section 27 "Direct light"), the inputs
of its tests and their error model: tests/test_bake_direct_ref.py on the CPU, tests/test_bake_direct.py on the device.  Written from the
definitions in include/mcpt.h and DESIGN.md section 27.

`terms` takes per item the origin P and unit normal N (float64, device coordinates: world less the scene's centre), the fp32 direction d of the
cosine ray and the three fp32 numbers of random-number block 0xFFFFFFFF, and works in ONE floating-point type T after that.  What the
definition itself rounds to fp32 is rounded in either type: n32 = float(N), float(pi), the two WORLD points of the light sample (the light point
and the bake point, as the reference's Render::sample holds them) and the inputs.  First hits and occlusion come from kit.brute_force_trace in
type T, the light pick from shade_ref.light_index, the light table from shade_ref.light_faces.

    A   sub = Le                for a first hit on an emitter (|radiance| > 0.0001) from behind
        sub = (1 - w_b) Le      for a first hit on a LIGHT (|radiance| > 0.01) from its front: p_b = max(d.n32, 0) / pi,
                                p_l = t t / ((cos_l nl) area) with cos_l = -d.n_hit (0 where cos_l == 0), w_b = p_b^2 / (p_b^2 + p_l^2)
        sub = 0                 otherwise
    B   the light sample counts (state 4) if its pdf is finite and > 0 and t2 > 1e-4 (else state 1), cos_p = wo.n32 > 0 (else 2) and nothing but
        the sampled face lies on [1e-4, t2] of the segment (else 3):  p_bl = cos_p / pi, p_lf = pdf / nl, w_l = p_lf^2 / (p_lf^2 + p_bl^2),
        add = (w_l Le) (p_bl / p_lf); w_l, p_bl and p_lf are reported for states 3 and 4, add for state 4 alone.

Error model, in this project's idiom.  S is the worst |float32 run - float64 run| over the device test's own inputs (`box_lists`: the centred,
black-walled open_box, family and interior points on both sides, list lengths 1, 63, 65, 257 and 1000, samples 0, 1 and 7), on rows that are
well conditioned and on which the two runs agree about the first hit and the occlusion: in units of 2^-24 max|Le| for add and sub, of 2^-24 for
the two weights and of 2^-24 |p| for the four pdfs (a pdf has no scale of its own: p_l grows without bound towards a light).  The device gets
BOUND = 4 S rounded up to a power of two, a stand-in for its v_rcp_f32 and the contraction the shared header functions are compiled with.

    S measured on the CPU: 6.23 (a pdf; radiance 0.99, weights 1.33), 4 S = 24.9, so BOUND = 32        (tests/test_bake_direct_ref.py::test_float32_slack)
    the device on an MI355X: see DESIGN.md section 27

Left out of every comparison, at most 2 % of the rows (EXCLUSION_CAP; test_exclusion_cap shows the inputs stay below it):
  ill conditioned  shade_ref.light_edge_inputs' cancellation rule -- a dot product whose terms cancel to less than 1/50 of their absolute sum --
                   on the cosine at the light, on cos_p and, for a light met from its front, on d.n32 and cos_l;
  unsure           rows the brute force cannot decide, by tests/test_bake.py::test_known_answer_per_item's three criteria: the fp64 and fp32 runs
                   name different first hits (or differ on the occlusion), the hit lies within 1e-4 of its face's edge, or a second face (the
                   segment's end, for the occlusion) lies within 2e-4 (relative) of it.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from tests import bake_ref as R, kit, shade_ref

F32 = np.float32
EPS24 = 2.0 ** -24
DIRECT_BLOCK = 0xFFFFFFFF
S_CPU = 6.23                                                # measured by tests/test_bake_direct_ref.py::test_float32_slack
BOUND = 32.0
EXCLUSION_CAP = 0.02
SEED = 20281
LENGTHS = (1, 63, 65, 257, 1000)                            # partial waves, partial blocks, more than one block
SAMPLES = (0, 1, 7)
DEAD, NO_PDF, BELOW, OCCLUDED, COUNTED = range(5)
FLOATS = ("sub", "add", "w_b", "w_l", "p_b", "p_l", "p_bl", "p_lf")


# ------------------------------------------------------------------------------------------------------------------------ the generator
def rng_block(pixel, sample, block, seed):
    """pt_device.h's rng_block: pcg4d of (pixel, sample, block ^ seed_hi 0x9E3779B9, seed_lo), the top 24 bits of each word as k / 2^24.
    (n, 4) float32 for an array of pixels."""
    x = np.asarray(pixel, np.uint32).reshape(-1).copy()
    seed = int(seed)
    y = np.full_like(x, int(sample) & 0xffffffff)
    z = np.full_like(x, (int(block) ^ (((seed >> 32) * 0x9E3779B9) & 0xffffffff)) & 0xffffffff)
    w = np.full_like(x, seed & 0xffffffff)
    a, c = np.uint32(1664525), np.uint32(1013904223)
    x = x * a + c; y = y * a + c; z = z * a + c; w = w * a + c
    for _ in range(2):
        x = x + y * w; y = y + z * x; z = z + x * y; w = w + y * z
        if _ == 0:
            x = x ^ (x >> np.uint32(16)); y = y ^ (y >> np.uint32(16)); z = z ^ (z >> np.uint32(16)); w = w ^ (w >> np.uint32(16))
    return np.stack([(v >> np.uint32(8)).astype(F32) * F32(1.0 / 16777216.0) for v in (x, y, z, w)], 1)


# ------------------------------------------------------------------------------------------------------------------------ the restatement
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cancels(a, b):
    """light_edge_inputs' rule on the dot product a.b: its terms cancel to less than 1/50 of their absolute sum."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return 50.0 * np.abs((a * b).sum(1)) < np.abs(a * b).sum(1)


def _normalize(a, T):
    return a * (T(1.0) / np.sqrt(_dot(a, a)))[:, None]


def _power(p1, p2, T):
    s = p1 * p1 + p2 * p2
    return np.where(s == 0, T(0.0), p1 * p1 / np.where(s == 0, T(1.0), s))


def _trace(vertex, face, keep, origin, direction, T, centre, t1=1e-4):
    """kit.brute_force_trace over the faces `keep` alone: (t, face in the scene's numbering or -1, u, v)."""
    idx = np.flatnonzero(keep)
    t, f, u, v = kit.brute_force_trace(SimpleNamespace(vertex=vertex, face=face[idx]), origin, direction, dtype=T, t1=t1, centre=centre)
    return t, np.where(f >= 0, idx[np.maximum(f, 0)], -1), u, v


def _area(vertex, face, f, T):
    p = vertex[face[f][:, :, 0]].astype(np.float64)
    e1 = (p[:, 1] - p[:, 0]).astype(T); e2 = (p[:, 2] - p[:, 0]).astype(T)
    c = np.cross(e1, e2)
    return T(0.5) * np.sqrt(_dot(c, c))


def terms(scene, centre, P, N, d, xi, dtype=np.float64, dead=None, vertex=None, normal=None, materials=None, visible=None):
    """The two terms of every item in type `dtype`.  P, N: (n, 3) float64; d: (n, 3) fp32 values; xi: (n, 3+) fp32 numbers of block 0xFFFFFFFF.
    vertex / normal / materials: a later pose of `scene`; visible: one byte per face, 0 = hidden (no light, hit by nothing).  A namespace of
    sub (n, 3), add (n, 3), w_b, w_l, p_b, p_l, p_bl, p_lf, hit_face, front, light_face, state -- mcpt_probe_bake_direct's columns -- and of what
    the tests' exclusions need: mis (a light met from its front), ill, wo, t2, hit_t, hit_edge, occ_t, occ_edge."""
    T = np.dtype(dtype).type
    V = np.asarray(scene.vertex if vertex is None else vertex, np.float64); NR = np.asarray(scene.normal if normal is None else normal, np.float64)
    mats = scene.materials if materials is None else materials
    face = scene.face; nf = face.shape[0]
    centre = np.asarray(centre, np.float64)
    P = np.asarray(P, np.float64).reshape(-1, 3); n = P.shape[0]
    dead = np.zeros(n, bool) if dead is None else np.asarray(dead).astype(bool)
    vis = np.ones(nf, bool) if visible is None else np.asarray(visible).astype(bool)
    n32 = np.asarray(N, np.float64).reshape(-1, 3).astype(F32).astype(T); d = np.asarray(d, np.float64).reshape(-1, 3).astype(F32).astype(T)
    xi = np.asarray(xi, F32).reshape(n, -1)
    rad = np.array([m.radiance for m in mats], np.float64)
    rl = np.sqrt((rad * rad).sum(1))
    pi = T(F32(R.PI))
    lights = np.array([f for f in range(nf) if rl[face[f, 0, 3]] > 0.01 and vis[f]], np.int64)
    nl = T(len(lights))
    world = P + centre
    out = SimpleNamespace()
    with np.errstate(all="ignore"):
        # ---- A: the cosine ray's first hit
        t, hf, hu, hv = _trace(V, face, vis, world, d, T, centre)
        hit = hf >= 0; f0 = np.where(hit, hf, 0)
        hw = T(1.0) - hu - hv
        vn = [NR[face[f0][:, k, 1]].astype(F32).astype(T) for k in range(3)]
        hn = _normalize(hw[:, None] * vn[0] + hu[:, None] * vn[1] + hv[:, None] * vn[2], T)
        front = hit & (_dot(hn, d) < 0)
        m = face[f0][:, 0, 3]
        le = rad[m].astype(F32).astype(T)
        behind = hit & ~front & (rl[m] > 0.0001)
        mis = front & (rl[m] > 0.01)
        p_b = np.maximum(_dot(d, n32), T(0.0)) / pi
        cos_l = -_dot(d, hn)
        p_l = np.where(cos_l != 0, (t * t) / ((cos_l * nl) * _area(V, face, f0, T)), T(0.0))
        p_b = np.where(mis, p_b, T(0.0)); p_l = np.where(mis, p_l, T(0.0))
        w_b = np.where(mis, _power(p_b, p_l, T), T(0.0))
        sub = np.where(behind[:, None], le, np.where(mis[:, None], (T(1.0) - w_b)[:, None] * le, T(0.0)))
        ill = mis & (_cancels(d, n32) | _cancels(d, hn))
        # ---- B: one light sample (sample_light of pt_device.h, guard = true)
        li, _ = shade_ref.light_index(xi[:, 0], len(lights))
        lface = lights[li]
        u, v = xi[:, 1], xi[:, 2]
        fold = (u + v) > F32(1.0)
        u, v = np.where(fold, F32(1.0) - u, u), np.where(fold, F32(1.0) - v, v)
        c = V[face[lface][:, :, 0]] - centre                                     # the fp64 corners the device holds
        b1, b2 = u.astype(np.float64)[:, None], v.astype(np.float64)[:, None]
        point = ((((1.0 - b1 - b2) * c[:, 0] + b1 * c[:, 1]) + b2 * c[:, 2]) + centre).astype(F32).astype(T)
        po = world.astype(F32).astype(T)
        uT, vT = u.astype(T), v.astype(T); wT = T(1.0) - uT - vT
        ln = [NR[face[lface][:, k, 1]].astype(F32).astype(T) for k in range(3)]
        lnrm = _normalize(wT[:, None] * ln[0] + uT[:, None] * ln[1] + vT[:, None] * ln[2], T)
        dd = point - po
        d2 = _dot(dd, dd); t2 = np.sqrt(d2)
        wo = dd * (T(1.0) / t2)[:, None]
        cs = -_dot(wo, lnrm)
        pdf = np.where(cs != 0, d2 / cs / _area(V, face, lface, T), T(0.0))
        lrad = rad[face[lface][:, 0, 3]].astype(F32).astype(T)
        state = np.full(n, NO_PDF, np.int32)
        ok = np.isfinite(pdf) & (pdf > 0) & (t2 > T(F32(1e-4)))
        cos_p = _dot(wo, n32)
        above = ok & (cos_p > 0)
        state[ok] = BELOW; state[above] = OCCLUDED
        occ_t = np.full(n, np.inf, T); occ_u = np.zeros(n, T); occ_v = np.zeros(n, T)
        for lf in np.unique(lface[above]):                                       # the sampled face is skipped: one trace per light that was picked
            rows = np.flatnonzero(above & (lface == lf))
            keep = vis.copy(); keep[lf] = False
            occ_t[rows], _, occ_u[rows], occ_v[rows] = _trace(V, face, keep, world[rows], wo[rows], T, centre)
        free = above & ~(occ_t <= t2)
        state[free] = COUNTED
        p_bl = np.where(above, cos_p / pi, T(0.0)); p_lf = np.where(above, pdf / nl, T(0.0))
        w_l = np.where(above, _power(p_lf, p_bl, T), T(0.0))
        add = np.where(free[:, None], (w_l[:, None] * lrad) * (p_bl / np.where(above, p_lf, T(1.0)))[:, None], T(0.0))
        ill = ill | _cancels(wo, lnrm) | _cancels(wo, n32)
    live = ~dead
    z = lambda a, fill=0: np.where(live.reshape((-1,) + (1,) * (a.ndim - 1)), a, np.asarray(fill, a.dtype))
    out.sub, out.add = z(sub), z(add)
    out.w_b, out.w_l, out.p_b, out.p_l, out.p_bl, out.p_lf = z(w_b), z(w_l), z(p_b), z(p_l), z(p_bl), z(p_lf)
    out.hit_face = z(hf.astype(np.int32), -1); out.front = z(front.astype(np.int32)); out.light_face = z(lface.astype(np.int32), -1)
    out.state = z(state, DEAD)
    out.mis = mis & live; out.ill = ill & live; out.wo = wo; out.t2 = t2; out.le = lrad; out.hit_le = le
    out.hit_t = t; out.hit_edge = np.minimum(np.minimum(hu, hv), hw); out.occ_t = occ_t; out.occ_edge = np.minimum(np.minimum(occ_u, occ_v), T(1.0) - occ_u - occ_v)
    out.lights = lights
    return out


def unsure_rows(scene, centre, P, d, r64, r32, vertex=None, visible=None):
    """The rows the brute force cannot decide (the module docstring's three criteria), from the float64 run r64 and the float32 run r32."""
    V = np.asarray(scene.vertex if vertex is None else vertex, np.float64)
    vis = np.ones(scene.face.shape[0], bool) if visible is None else np.asarray(visible).astype(bool)
    world = np.asarray(P, np.float64) + np.asarray(centre, np.float64); d = np.asarray(d, np.float64)
    hit = r64.hit_face >= 0
    t64 = np.where(hit, r64.hit_t, 0.0)
    t2nd, _, _, _ = _trace(V, scene.face, vis, world + d * (t64 * (1 + 1e-4))[:, None], d, np.float64, centre, t1=0.0)
    first = (r64.hit_face != r32.hit_face) | (hit & (r64.hit_edge < 1e-4)) | (hit & np.isfinite(t2nd) & (t2nd < 2e-4 * np.where(hit, t64, 1.0)))
    reached = (r64.state >= OCCLUDED) | (r32.state >= OCCLUDED)
    blocked = np.isfinite(r64.occ_t) & (r64.occ_t <= r64.t2 * (1 + 2e-4))
    occ = reached & (((r64.state == COUNTED) != (r32.state == COUNTED)) | (blocked & (r64.occ_edge < 1e-4)) | (np.abs(r64.occ_t - r64.t2) <= 2e-4 * r64.t2))
    return (first | occ) & (r64.state != DEAD)


def worst_units(got, ref, keep):
    """The worst difference of the kept rows from the float64 run `ref`, per class, in the error model's units: {"radiance", "weight", "pdf"}.
    `got`: a namespace like ref, or mcpt_probe_bake_direct's (n, 12) array."""
    if isinstance(got, np.ndarray):
        g = SimpleNamespace(sub=got[:, 0:3], add=got[:, 3:6], **{k: got[:, 6 + i] for i, k in enumerate(FLOATS[2:])})
    else:
        g = got
    le = max(float(np.abs(ref.le).max()), float(np.abs(ref.hit_le).max()))
    D = lambda k: np.abs(np.asarray(getattr(g, k), np.float64) - np.asarray(getattr(ref, k), np.float64))[keep]
    out = {"radiance": max(D("sub").max(initial=0), D("add").max(initial=0)) / (EPS24 * le), "weight": max(D("w_b").max(initial=0), D("w_l").max(initial=0)) / EPS24}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["pdf"] = max(float(np.nan_to_num(D(k) / (EPS24 * np.abs(np.asarray(getattr(ref, k), np.float64))[keep]), nan=0.0, posinf=np.inf).max(initial=0)) for k in FLOATS[4:])
    return {k: float(x) for k, x in out.items()}


# ------------------------------------------------------------------------------------------------------------------------ scenes and points
def centred_box(pkg, black=False):
    """open_box moved so that the centre every device coordinate is relative to is exactly 0 (tests/test_bake.py's copy): probe_paths then starts
    from the very origins the stage wrote.  black: every non-emissive material with kd = ks = 0."""
    s = pkg.scenes.open_box(16, 16)
    used = s.vertex[np.unique(s.face[:, :, 0])]
    out = kit.with_arrays(pkg, s, vertex=s.vertex - (0.5 * used.min(0) + 0.5 * used.max(0)))
    if black:
        out.materials = [m if any(m.radiance) else pkg.scenes.Material(m.name) for m in s.materials]
    return out


def family_points(pkg, scene, n, seed=SEED, faces=None):
    """n points on `scene`: every face (or `faces`) at every (u, v) of bake_ref.UV_SET on both sides first, then random interior ones; cut or
    filled to n (tests/test_bake.py's family)."""
    faces = np.arange(scene.face.shape[0]) if faces is None else np.asarray(faces)
    f, u, v, b = [], [], [], []
    for fc in faces:
        for uv in R.UV_SET:
            for back in (0, 1):
                f.append(fc); u.append(uv[0]); v.append(uv[1]); b.append(back)
    rng = np.random.default_rng(seed)
    m = max(0, n - len(f))
    a = rng.random((m, 2)); flip = a.sum(1) > 1; a[flip] = 1 - a[flip]
    f += list(rng.choice(faces, m)); u += list(a[:, 0]); v += list(a[:, 1]); b += list(rng.integers(0, 2, m))
    pts = pkg.bake_points(np.array(f[:n]), np.array(u[:n], F32), np.array(v[:n], F32), np.array(b[:n], np.uint32))
    over = pts["u"].astype(np.float64) + pts["v"].astype(np.float64) > 1.0
    pts["v"][over] = np.nextafter(pts["v"][over], F32(0))
    return pts


def interior_points(pkg, scene, n, seed=SEED):
    """n points well inside their faces (every barycentric >= 0.05), all faces, both sides."""
    rng = np.random.default_rng(seed)
    a = rng.random((n, 2)); flip = a.sum(1) > 1; a[flip] = 1 - a[flip]
    a = 0.05 + 0.85 * a
    return pkg.bake_points(rng.integers(0, scene.face.shape[0], n), a[:, 0].astype(F32), a[:, 1].astype(F32), rng.integers(0, 2, n).astype(np.uint32))


def box_lists(pkg, scene):
    """[(points, sample)] of the device test: per length a list whose first half is the point family and whose second half lies inside the faces,
    at samples 0, 1 and 7."""
    out = []
    for length in LENGTHS:
        half = (length + 1) // 2
        pts = np.concatenate([family_points(pkg, scene, half, SEED + length), interior_points(pkg, scene, length - half, SEED + length)])
        out += [(pts, s) for s in SAMPLES]
    return out


def cpu_rays(scene, centre, pts, sample, seed, first=0):
    """What the stage hands the direct-light kernel, without a device: bake_ref.rays from this module's generator -- (P, N, d as fp32 values,
    dead, xi of block 0xFFFFFFFF)."""
    items = np.arange(first, first + len(pts))
    o, n, d, dead = R.rays(xi=rng_block(items, sample, 0, seed)[:, :2], **R.scene_inputs(scene, centre, pts))
    return o, n, d.astype(F32).astype(np.float64), dead, rng_block(items, sample, DIRECT_BLOCK, seed)[:, :3]


def lamp_rect(scene):
    """(x0, x1, z0, z1, y) of open_box's lamp."""
    lv = scene.vertex[np.unique(scene.face[shade_ref.light_faces(scene)][:, :, 0])]
    return lv[:, 0].min(), lv[:, 0].max(), lv[:, 2].min(), lv[:, 2].max(), lv[0, 1]
