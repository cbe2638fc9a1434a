"""Plain numpy restatements of the first and the last steps of every path -- cast_ray, load_hit_shade and tex_color of csrc/pt_device.h and
tonemap_kernel of csrc/kernels.hip --, the error model each comparison uses and the deliberately awkward inputs of tests/test_endpoints_ref.py
(CPU) and tests/test_endpoints_edges.py (device).  Written from the behaviour documented in pt_device.h, kernels.hip and oracle/mcpt_oracle.cpp.

Every restatement takes the fp32 values the device actually holds (records, barycentrics, uv, film sums) and works in float64 after that, so a
difference from it is the error of the side under test and not an input rounding.

Camera (cast_ref).  ((float)x + xi) / (float)width is replayed in np.float32: both operations are IEEE, the replay is bit-exact.  The rest is
float64 in the operation order of camera_constants (scene_build.cpp) and cast_ray.  The only roundings outside the replay are float64 ones and the
final conversion to fp32, so a component q of the origin or the direction is allowed 2^-24 max(|q|, 2^-126) (1 + 2^-20): half an fp32 ulp plus
float64 slack.  Nothing is measured.

Texture (tex_ref).  fu = tu - floorf(tu) in np.float32, the caps of clamp01(float) (> 0.999f gives the DOUBLE 0.999, < 0 gives 0), (int)(cu * w) in
float64: two IEEE operations and exact integer arithmetic.  No tolerance: the texel is the restatement's for every finite uv.

Hit record (hit_shade_ref).  w = 1 - u - v and the three interpolations in float64 from the fp32 corner records.  Beside each output stands its
absolute-value form (every product and difference replaced by the sum of magnitudes: w -> 1 + |u| + |v|; the normal's form divided by the length
of the unnormalised sum), as tests/trace_ref.py does it, and the allowance is K_HIT 2^-24 times that form.  K_HIT is measured on the CPU by
`hit_shade_replay`, the same expressions in np.float32 with every product-sum evaluated both uncontracted and as an fma chain (-ffp-contract=fast
leaves that open) and the reciprocal square root moved by -1, 0, +1 ulp (v_rsq_f32 is a 1-ulp operation): worst ratio 4.41 (family distinct, a
normal; uv at most 2.09), so K_HIT = 16, the next power of two at or above twice the worst.  `front` must equal the restatement's wherever |n.d|
exceeds K_HIT 2^-24 sum_i (|n_i| + form_i) |d_i|; at or below it the case is `marginal` (an exact zero whose bound is zero too is not: nothing
rounds).  An exactly zero normal sum is normalize(0) on both sides: the restatement's normal is not a number, the device's must not be finite,
and nothing more is compared for that case.

Tonemap (tonemap_ref).  The definition it pins: the mean is sum / count; a NaN mean gives 0, +inf gives 255, negative and -inf give 0, count 0
with sum 0 gives 0 (0 / 0 is NaN).  y = sqrt(clamp(mean, 0, 1)) * float32(255.99) in float64 from the fp32 sum and count, and a level L is
admissible iff some y' with |y' - y| <= K 2^-24 y + 2^-67 has floor(y') = L.  (The second term is derived, not measured: a mean below 2^-126 is
held by fp32 to 2^-150 absolute, not to a relative error, and sqrt(m + e) - sqrt(m) <= sqrt(e) = 2^-75, times 255.99; it moves no level.)  K_T, the K
of the oracle's arithmetic, is measured like K_HIT: the np.float32 chain (IEEE divide, correctly rounded sqrt, IEEE multiply) against float64 on
`tonemap_cases` has the worst ratio 2.29 (family boundary; half an ulp of the mean halved by the root, half an ulp of the root and half an ulp of
the product are at most 1.25 ulp, and an ulp is up to 2^-23 relative: 2.5), so K_T = 8, the next power of two at or above twice the worst.  The
device is given TONEMAP_DEVICE_FACTOR = 4 times that for powf(m, 0.5f) taking the place of the correctly rounded root.  Source of the factor:
shade_ref.DEVICE_FACTOR; the documentation that ships with the ROCm installation states no ulp bound for powf, so nothing larger is claimed.
At 32 * 2^-24 the band around a level boundary is 5e-4 of a level at y = 255.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

F32 = np.float32
EPS24 = 2.0 ** -24
ONE_BELOW = F32(1.0 - EPS24)
K_HIT = 16.0                                                # measured 4.41, see the module docstring
K_T = 8.0                                                   # measured 2.29
Y_FLOOR = 2.0 ** -67                                        # see the module docstring
TONEMAP_DEVICE_FACTOR = 4.0
CAP = F32(0.999)
SCALE_255 = F32(255.99)
SEED = 20262


def _f32(x):
    return np.asarray(x, np.float64).astype(F32)


def _steps(x, k):
    """The fp32 number k representable steps above (below for k < 0) each element of x."""
    x = np.array(x, F32)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def worst_by_family(family, ratio):
    """{family: largest ratio}; NaN ratios count as inf."""
    r = np.where(np.isnan(ratio), np.inf, ratio)
    return {f: float(r[family == f].max()) for f in np.unique(family)}


def print_worst(title, family, ratio, allowed=1.0):
    for f, w in worst_by_family(family, ratio).items():
        print("%-34s %-14s worst ratio %8.3f (allowed %g)" % (title, f, w, allowed))


def next_pow2(x):
    return 2.0 ** math.ceil(math.log2(x))


# ------------------------------------------------------------------------------------------------------------------------ camera
def _len3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def camera_constants(camera):
    """(h, front, right, up) as camera_constants forms them: float64, glm's operation order."""
    eye, lookat, up = (np.array([float(x) for x in v], np.float64) for v in (camera.eye, camera.lookat, camera.up))
    h = math.tan(float(camera.fovy) * 3.14159265358979323846 / 180.0 * 0.5) * 2.0
    fr = lookat - eye
    front = fr * (1.0 / _len3(fr))
    rt = np.array([front[1] * up[2] - up[1] * front[2], front[2] * up[0] - up[2] * front[0], front[0] * up[1] - up[0] * front[1]])
    return h, front, rt * (1.0 / _len3(rt)), up


def cast_ref(camera, centre, width, height, xy, xi):
    """(origin (3,) float32, direction (N, 3) float64) of cast_ray for pixels xy (N, 2) int and offsets xi (N, 2) fp32 on a width x height film
    of a context whose scene centre is `centre`."""
    h, front, right, up = camera_constants(camera)
    xy = np.asarray(xy, np.int32).reshape(-1, 2); xi = np.asarray(xi, F32).reshape(-1, 2)
    fx = (xy[:, 0].astype(F32) + xi[:, 0]) / F32(width)                      # the fp32 replay: bit-exact
    fy = (xy[:, 1].astype(F32) + xi[:, 1]) / F32(height)
    assert fx.dtype == F32 and fy.dtype == F32
    u = (fx.astype(np.float64) - 0.5) * h * float(width) / float(height)
    v = (fy.astype(np.float64) - 0.5) * h
    d = front[None, :] + u[:, None] * right[None, :] + v[:, None] * up[None, :]
    inv = 1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    eye = np.array([float(x) for x in camera.eye], np.float64); centre = np.asarray(centre, np.float64)
    return ((eye - centre) + centre).astype(F32), d * inv[:, None]


def cast_bound(q):
    return EPS24 * np.maximum(np.abs(np.asarray(q, np.float64)), 2.0 ** -126) * (1 + 2.0 ** -20)


def cast_ratio(got6, origin, direction):
    """Per case the worst |difference| / bound over the six outputs of probe_cast_ray."""
    want = np.concatenate([np.broadcast_to(np.asarray(origin, np.float64), direction.shape), direction], 1)
    with np.errstate(invalid="ignore"):
        r = np.abs(np.asarray(got6, np.float64) - want) / cast_bound(want)
    return np.where(np.isnan(r), np.inf, r).max(1)


FILMS = ((1, 1), (3, 2), (37, 21), (1, 257), (257, 1), (4097, 3), (16384, 2))
XI_SET = (0.0, EPS24, 0.5, 1.0 - EPS24)


def pixel_cases(width, height, seed=SEED):
    """(xy int32 (N, 2), xi float32 (N, 2), family) for one film: the four corners and the centre with every xi of XI_SET on both axes, the last column
    with xi_x = 1 - 2^-24, random pixels with xi from XI_SET, random pixels with random xi (k 2^-24)."""
    rng = np.random.default_rng(seed + 7 * width + height)
    xy, xi, fam = [], [], []

    def add(family, p, x):
        p = np.asarray(p, np.int32).reshape(-1, 2); x = np.broadcast_to(np.asarray(x, np.float64), p.shape)
        xy.append(p); xi.append(x.astype(F32)); fam.append(np.full(len(p), family))

    grid = np.array([(a, b) for a in XI_SET for b in XI_SET])
    for p in ((0, 0), (width - 1, 0), (0, height - 1), (width - 1, height - 1), (width // 2, height // 2)):
        add("corners", np.tile(p, (len(grid), 1)), grid)
    rows = np.unique(np.concatenate([np.arange(min(height, 8)), rng.integers(0, height, 24)]))
    for b in XI_SET:
        add("last_column", np.stack([np.full(len(rows), width - 1), rows], 1), np.stack([np.full(len(rows), 1.0 - EPS24), np.full(len(rows), b)], 1))
    m = 64
    add("xi_edges", np.stack([rng.integers(0, width, m), rng.integers(0, height, m)], 1), grid[rng.integers(0, len(grid), m)])
    m = 128
    add("random", np.stack([rng.integers(0, width, m), rng.integers(0, height, m)], 1), rng.integers(0, 1 << 24, (m, 2)) / float(1 << 24))
    return np.concatenate(xy), np.concatenate(xi), np.concatenate(fam)


def camera_cases(scene_camera, centre):
    """[(family, name, dict(eye, lookat, up, fovy))]: the field of view from 0.001 to 179.9 degrees, `up` unit, long, skewed and 1e-3 rad from the view
    direction, an eye 1e6 and 1e9 from the scene, |lookat - eye| of 1e-12 and 1e15, views along each negative axis."""
    e, l, u = (tuple(float(x) for x in v) for v in (scene_camera.eye, scene_camera.lookat, scene_camera.up))
    c = tuple(float(x) for x in centre)
    out = []
    for fovy in (0.001, 1.0, 40.0, 90.0, 170.0, 179.9):
        out.append(("fovy", "fovy %g" % fovy, dict(eye=e, lookat=l, up=u, fovy=fovy)))
    fr = np.subtract(l, e); fr = fr / np.linalg.norm(fr)
    side = np.cross(fr, (0.0, 1.0, 0.0)); upright = np.cross(side, fr); upright /= np.linalg.norm(upright)
    near = tuple(math.cos(1e-3) * fr + math.sin(1e-3) * upright)
    for name, up in (("unit", (0.0, 1.0, 0.0)), ("long", (0.0, 2.5, 0.0)), ("skewed", (0.3, 1.0, 0.2)), ("1e-3 rad from the view", near)):
        out.append(("up", "up " + name, dict(eye=e, lookat=l, up=up, fovy=40.0)))
    for off in (1e6, 1e9):
        out.append(("far_eye", "eye + %g" % off, dict(eye=(e[0] + off, e[1], e[2] + 0.5 * off), lookat=c, up=(0.3, 1.0, 0.2), fovy=40.0)))
    t = np.array([0.1, -0.2, -1.0]); t /= np.linalg.norm(t)
    out.append(("lookat_distance", "|lookat - eye| 1e-12", dict(eye=e, lookat=(e[0], e[1], e[2] - 1e-12), up=u, fovy=40.0)))
    out.append(("lookat_distance", "|lookat - eye| 1e15", dict(eye=e, lookat=tuple(np.add(e, 1e15 * t)), up=(0.3, 1.0, 0.2), fovy=40.0)))
    for ax, up in ((0, (0.0, 1.0, 0.0)), (1, (0.0, 0.0, -1.0)), (2, (0.0, 1.0, 0.0))):
        eye = list(c); eye[ax] += 2.0
        out.append(("axis", "along -%s" % "xyz"[ax], dict(eye=tuple(eye), lookat=c, up=up, fovy=40.0)))
    return out


# ------------------------------------------------------------------------------------------------------------------------ texture
def tex_ref(image_w, image_h, tex_off, uv_f32):
    """(x, y, texel index) of tex_color for fp32 uv (N, 2) on an image_w x image_h image whose first texel is tex_off."""
    uv = np.asarray(uv_f32)
    assert uv.dtype == F32
    uv = uv.reshape(-1, 2)
    if image_w * image_h == 1:
        z = np.zeros(len(uv), np.int64)
        return z, z, z + tex_off
    out = []
    with np.errstate(invalid="ignore"):
        for t, n in ((uv[:, 0], image_w), (uv[:, 1], image_h)):
            f = t - np.floor(t)
            assert f.dtype == F32
            c = np.where(f > CAP, 0.999, np.where(f < F32(0), 0.0, f.astype(np.float64)))
            out.append((c * float(n)).astype(np.int64))
    return out[0], out[1], tex_off + out[1] * image_w + out[0]


TEXTURES = (None, (1, 1), (1, 7), (7, 1), (8, 5), (255, 3), (1000, 3), (3, 1000), (2000, 1), (4096, 2))     # (w, h); None: a constant colour


def texture_materials(pkg, first_index):
    """The materials of the texture scene, `first_index` being the index of the first: every texel's rgb is (x, y, material index), exact in fp32.
    Returns (materials, [(w, h, tex_off relative to the first material's texture)])."""
    S = pkg.scenes
    mats, dims, off = [], [], 0
    for k, wh in enumerate(TEXTURES):
        i = first_index + k
        if wh is None:
            mats.append(S.Material("const%d" % i, kd=(0.0, 0.0, float(i)))); w = h = 1
        else:
            w, h = wh
            img = np.zeros((h, w, 3), F32)
            img[..., 0] = np.arange(w, dtype=F32)[None, :]; img[..., 1] = np.arange(h, dtype=F32)[:, None]; img[..., 2] = F32(i)
            mats.append(S.Material("tex%d" % i, kd=(0.5, 0.5, 0.5), map_kd="t%d.ppm" % i, texture=img))
        dims.append((w, h, off)); off += w * h
    return mats, dims


def texture_scene(pkg):
    """open_box with the texture materials appended (no face uses them: the probe names its material).  (scene, index of the first, dims)."""
    S = pkg.scenes
    base = S.open_box(8, 8)
    first = len(base.materials)
    mats, dims = texture_materials(pkg, first)
    return S.SceneData("texture-edges", base.vertex, base.normal, base.texcoord, base.face, list(base.materials) + mats, base.camera, {}), first, dims


def _axis_values(n, rng):
    """fp32 texture coordinates for an axis of n texels, with a family name each."""
    ks = np.arange(n + 1) if n <= 255 else np.concatenate([[0, 1, n - 1, n], 2 + rng.choice(n - 3, 60, replace=False)])      # every k, or 64 of them
    edge = ks.astype(F32) / F32(n)
    vals = [_steps(edge, s) for s in (-2, -1, 0, 1, 2)]
    fam = ["texel_edges"] * (5 * len(edge))
    cap = [_steps([CAP], s)[0] for s in (-2, -1, 0, 1, 2)] + [ONE_BELOW, F32(1.0), F32(2.0), F32(-1.0), F32(-0.0)]
    den = [F32(2.0 ** -149), F32(-2.0 ** -149), F32(1e-38), F32(-1e-38), F32(-2.0 ** -30)]
    huge = [F32(2.0 ** 23 + 0.5), F32(2.0 ** 24), F32(-2.0 ** 24), F32(1e10), F32(-1e10), F32(3e38), F32(-3e38)]
    uni = rng.uniform(-4, 4, 200).astype(F32)
    vals += [np.array(cap, F32), np.array(den, F32), np.array(huge, F32), uni]
    fam += ["cap"] * len(cap) + ["denormal"] * len(den) + ["huge"] * len(huge) + ["uniform"] * len(uni)
    return np.concatenate(vals).astype(F32), np.array(fam)


def texture_cases(w, h, seed=SEED):
    """(uv float32 (N, 2), family) for a w x h image: every value of the u axis against values of the v axis taken in turn, and the other way round."""
    rng = np.random.default_rng(seed + 31 * w + h)
    uu, fu = _axis_values(w, rng)
    vv, fv = _axis_values(h, rng)
    a = np.stack([uu, vv[rng.integers(0, len(vv), len(uu))]], 1)
    b = np.stack([uu[rng.integers(0, len(uu), len(vv))], vv], 1)
    return np.concatenate([a, b]).astype(F32), np.concatenate([fu, fv])


# ------------------------------------------------------------------------------------------------------------------------ hit record
def corner_records(scene):
    """(n_faces, 3 corners, 5) float32: the normal and the uv of every corner, as the device's tri_shade records hold them."""
    n = scene.normal[scene.face[:, :, 1]]; t = scene.texcoord[scene.face[:, :, 2]]
    return np.concatenate([n, t], 2).astype(F32)


def hit_shade_ref(records, tri, u, v, d):
    """load_hit_shade in float64 for faces `tri` (N,) of `records` at fp32 barycentrics u, v and directions d (N, 3; rounded to fp32 as the probe does).
    Namespace of n (N, 3), tu, tv, front, nd and their absolute-value forms n_abs, tu_abs, tv_abs, nd_abs; length (of the unnormalised sum)."""
    R = np.asarray(records)[np.asarray(tri, np.int64)].astype(np.float64)
    assert np.asarray(u).dtype == F32 and np.asarray(v).dtype == F32
    u = np.asarray(u, np.float64); v = np.asarray(v, np.float64); d = _f32(d).astype(np.float64).reshape(-1, 3)
    w = 1.0 - u - v
    wa = 1.0 + np.abs(u) + np.abs(v)
    B = np.stack([w, u, v], 1)[:, :, None]; Ba = np.stack([wa, np.abs(u), np.abs(v)], 1)[:, :, None]
    raw = (B * R).sum(1); form = (Ba * np.abs(R)).sum(1)                            # (N, 5)
    length = np.sqrt((raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1]) + raw[:, 2] * raw[:, 2])
    with np.errstate(all="ignore"):
        n = raw[:, :3] / length[:, None]; n_abs = form[:, :3] / length[:, None]
        nd = (n * d).sum(1); nd_abs = ((np.abs(n) + n_abs) * np.abs(d)).sum(1)
    return SimpleNamespace(n=n, tu=raw[:, 3], tv=raw[:, 4], front=nd < 0, nd=nd, n_abs=n_abs, tu_abs=form[:, 3], tv_abs=form[:, 4], nd_abs=nd_abs, length=length)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _sum3(x0, y0, x1, y1, x2, y2, contract):
    """x0 y0 + x1 y1 + x2 y2 in fp32: rounded product by product and sum by sum, or as the fma chain contraction makes of it."""
    if contract:
        return _fma(x2, y2, _fma(x1, y1, x0 * y0))
    return (x0 * y0 + x1 * y1) + x2 * y2


def hit_shade_replay(records, tri, u, v, d, contract=False, rsq_ulp=0):
    """load_hit_shade in np.float32, the same expressions: out6 (N, 6) in the probe's layout."""
    R = np.asarray(records, F32)[np.asarray(tri, np.int64)]
    u = np.asarray(u, F32); v = np.asarray(v, F32); d = _f32(d).reshape(-1, 3)
    w = F32(1) - u - v
    with np.errstate(all="ignore"):
        raw = [_sum3(w, R[:, 0, k], u, R[:, 1, k], v, R[:, 2, k], contract) for k in range(5)]
        dot = _sum3(raw[0], raw[0], raw[1], raw[1], raw[2], raw[2], contract)
        r = (1.0 / np.sqrt(dot.astype(np.float64))).astype(F32)
        r = np.where(np.isfinite(r), _steps(r, rsq_ulp), r)
        n = [raw[k] * r for k in range(3)]
        nd = _sum3(n[0], d[:, 0], n[1], d[:, 1], n[2], d[:, 2], contract)
    return np.stack(n + [raw[3], raw[4], (nd < 0).astype(F32)], 1)


def hit_check(ref, out6, K=K_HIT):
    """(ratio (N,), marginal (N,), bad (N,)) of probe_hit_shade's layout against the restatement: ratio is the worst |difference| / (2^-24 form) over the
    normal and the uv (so the case is inside iff ratio <= K); a zero normal sum asks for a non-finite normal and nothing more."""
    out = np.asarray(out6, np.float64)
    zero = ~np.isfinite(ref.n).all(1)
    with np.errstate(all="ignore"):
        want = np.concatenate([ref.n, ref.tu[:, None], ref.tv[:, None]], 1)
        form = np.concatenate([ref.n_abs, ref.tu_abs[:, None], ref.tv_abs[:, None]], 1)
        err = np.abs(out[:, :5] - want)
        r = np.where(err == 0, 0.0, err / (EPS24 * form))
    r = np.where(np.isnan(r), np.inf, r).max(1)
    marginal = (np.abs(ref.nd) <= K * EPS24 * ref.nd_abs) & (ref.nd_abs > 0) & ~zero
    bad = np.where(zero, np.isfinite(out[:, :3]).all(1), (r > K) | (~marginal & ((out[:, 5] != 0) != ref.front)))
    return np.where(zero, 0.0, r), marginal, bad


HIT_TARGET = (F32(0.25), F32(0.25))                       # the barycentrics (u, v) at which the cancelling faces cancel


def hit_mesh(pkg, seed=SEED):
    """About 200 small faces with a corner of its own each, so that a swapped corner or channel changes the answer: (scene, face family (n_faces,)).
      distinct     three different non-unit normals and three different uv, of magnitude 1, 100 or 1e6 (uv0: magnitude 0)
      cancel3/6    normals whose interpolation at HIT_TARGET has length 1e-3 / 1e-6
      equal        one normal on all three corners: (0, 0, 2), where n.d is exact, and a generic one
      zero_corner  a zero normal on one corner
      zero_sum     normals that cancel exactly at HIT_TARGET, and three zero normals
    The last two faces are the light every scene needs."""
    S = pkg.scenes
    rng = np.random.default_rng(seed)
    m = S._Mesh()
    fam = []

    def face(k, family, nrm, uv):
        x, y = (k % 16) * 0.125, (k // 16) * 0.125
        p = np.array([[x, y, 0.0], [x + 0.1, y + 0.01 * rng.uniform(), 0.02 * rng.uniform()], [x + 0.01 * rng.uniform(), y + 0.1, 0.02 * rng.uniform()]])
        i = m.add_vertices(p, np.asarray(nrm, np.float64).reshape(3, 3), np.asarray(uv, np.float64).reshape(3, 2))
        m.add_tri(i, i + 1, i + 2, 1 if family == "light" else 0)
        fam.append(family)

    def normals():
        return rng.normal(size=(3, 3)) * rng.uniform(0.5, 3.0, (3, 1))

    k = 0
    for scale in (1.0, 100.0, 1e6, 1.0, 100.0, 1e6, 0.0):
        for _ in range(20):
            face(k, "distinct" if scale else "uv0", normals(), scale * rng.uniform(-1, 1, (3, 2))); k += 1
    u0, v0 = float(HIT_TARGET[0]), float(HIT_TARGET[1])
    for family, length in (("cancel3", 1e-3), ("cancel6", 1e-6)):
        for _ in range(12 if length == 1e-3 else 4):
            n = normals(); t = rng.normal(size=3); t /= np.linalg.norm(t)
            n[2] = (length * t - (1 - u0 - v0) * n[0] - u0 * n[1]) / v0
            face(k, family, n, rng.uniform(-1, 1, (3, 2))); k += 1
    for _ in range(12):
        face(k, "equal", np.tile([0.0, 0.0, 2.0], (3, 1)), rng.uniform(-1, 1, (3, 2))); k += 1
    for _ in range(12):
        face(k, "equal", np.tile(rng.normal(size=3) * 1.7, (3, 1)), 100.0 * rng.uniform(-1, 1, (3, 2))); k += 1
    for c in range(12):
        n = normals(); n[c % 3] = 0.0
        face(k, "zero_corner", n, rng.uniform(-1, 1, (3, 2))); k += 1
    face(k, "zero_sum", [[1.0, -2.0, 0.5], [-1.0, 2.0, 1.0], [-1.0, 2.0, -2.0]], rng.uniform(-1, 1, (3, 2))); k += 1
    face(k, "zero_sum", np.zeros((3, 3)), rng.uniform(-1, 1, (3, 2))); k += 1
    for _ in range(2):
        face(k, "light", np.tile([0.0, 0.0, 1.0], (3, 1)), rng.uniform(0, 1, (3, 2))); k += 1
    mats = [S.Material("grey", kd=(0.5, 0.5, 0.5)), S.Material("light", kd=(0.5, 0.5, 0.5), radiance=(5.0, 5.0, 5.0))]
    cam = S._qcam((1.0, 1.0, 4.0), (1.0, 1.0, 0.0), (0, 1, 0), 40.0, 8, 8)
    return m.finish("hit-edges", mats, cam, {}), np.array(fam)


def hit_cases(scene, face_family, seed=SEED):
    """dict of tri (int32), u, v (float32), d (float32 (N, 3)), family (of the barycentrics / direction) and face_family, about 10 000 cases:
      corners, edge_mid   the three corners, the three edge midpoints
      sum_one             u + v = 1 exactly, and v one fp32 step to either side
      w_negative          u = 0.5, v = 0.5 + 2^-24: w = -2^-24, which the traversal can produce
      target              HIT_TARGET and its fp32 neighbours (where the cancelling faces cancel)
      interior            random interior points
      nd_0, nd_1e-7, nd_1e-4   an interior point with a direction built to have that |n.d|, either sign (exactly 0 on the faces with n = (0, 0, 1))
    Cancelling faces get few directions: on them the sign of n.d is mostly within rounding."""
    rng = np.random.default_rng(seed + 1)
    rec = corner_records(scene)
    rows = {k: [] for k in ("tri", "u", "v", "d", "family")}

    def unit(n):
        x = rng.normal(size=(n, 3)); return x / np.linalg.norm(x, axis=1, keepdims=True)

    def add(f, family, u, v, d=None):
        u = np.asarray(u, np.float64).reshape(-1).astype(F32); v = np.asarray(v, np.float64).reshape(-1).astype(F32)
        rows["tri"].append(np.full(len(u), f, np.int32)); rows["u"].append(u); rows["v"].append(v)
        rows["d"].append((unit(len(u)) if d is None else np.asarray(d, np.float64).reshape(-1, 3)).astype(F32)); rows["family"].append(np.full(len(u), family))

    for f, ff in enumerate(face_family):
        if ff == "light":
            continue
        few = ff in ("cancel3", "cancel6", "zero_sum")
        add(f, "corners", [0, 1, 0], [0, 0, 1])
        add(f, "edge_mid", [0.5, 0, 0.5], [0, 0.5, 0.5])
        t = HIT_TARGET
        if ff == "zero_sum":                                                     # (one step beside an exact zero fp32 may or may not see a zero: not a case)
            add(f, "target", [t[0]], [t[1]])
            continue
        add(f, "target", [t[0], t[0], t[0], _steps([t[0]], 1)[0], _steps([t[0]], -1)[0]], [t[1], _steps([t[1]], 1)[0], _steps([t[1]], -1)[0], t[1], t[1]])
        if few:
            continue
        uu = rng.integers(1 << 23, 1 << 24, 4) / float(1 << 24)                  # [0.5, 1): 1 - u is an fp32 number
        vv = (1.0 - uu).astype(F32)
        add(f, "sum_one", np.tile(uu, 3), np.concatenate([vv, _steps(vv, 1), _steps(vv, -1)]))
        add(f, "w_negative", [0.5, 0.5 + EPS24], [0.5 + EPS24, 0.5])
        a = rng.uniform(0, 1, (40, 2)); a = np.where((a.sum(1) > 1)[:, None], 1 - a, a)
        add(f, "interior", a[:, 0], a[:, 1])
        if ff in ("distinct", "equal", "zero_corner"):
            a = rng.uniform(0.1, 0.45, (12, 2)).astype(F32)
            r = hit_shade_ref(rec, np.full(12, f), a[:, 0], a[:, 1], np.zeros((12, 3)))
            t = unit(12); t -= (t * r.n).sum(1)[:, None] * r.n; t /= np.linalg.norm(t, axis=1, keepdims=True)
            s = np.array([0.0, 0.0, 1e-7, -1e-7, 1e-4, -1e-4] * 2)
            names = np.array(["nd_0", "nd_0", "nd_1e-7", "nd_1e-7", "nd_1e-4", "nd_1e-4"] * 2)
            d = t + s[:, None] * r.n
            exact = bool(np.all(rec[f, :, :3] == F32([0, 0, 2])))
            pick = (names == "nd_1e-4") | exact | (f % 16 == 0)                    # the inexact 0 and 1e-7 are mostly marginal: on every sixteenth face only
            for nm in np.unique(names[pick]):
                sel = pick & (names == nm)
                add(f, nm, a[sel, 0], a[sel, 1], d[sel])
    case = {k: np.concatenate(a) for k, a in rows.items()}
    case["face_family"] = np.asarray(face_family)[case["tri"]]
    return case


# ------------------------------------------------------------------------------------------------------------------------ tonemap
def tonemap_ref(rgba_f32, K=TONEMAP_DEVICE_FACTOR * K_T):
    """(lo, hi, y) per colour channel of films rgba (..., 4) float32: the admissible levels are lo .. hi (module docstring), y the float64 value of
    sqrt(clamp(mean)) * 255.99f."""
    a = np.asarray(rgba_f32)
    assert a.dtype == F32
    with np.errstate(all="ignore"):
        mean = a[..., :3].astype(np.float64) / a[..., 3:].astype(np.float64)
    m = np.minimum(np.maximum(np.where(np.isnan(mean), 0.0, mean), 0.0), 1.0)
    y = np.sqrt(m) * np.float64(SCALE_255)
    lo = np.maximum(np.floor(y * (1 - K * EPS24) - Y_FLOOR), 0).astype(np.int64); hi = np.minimum(np.floor(y * (1 + K * EPS24) + Y_FLOOR), 255).astype(np.int64)
    return lo, hi, y


def tonemap_ratio(y, y_got):
    """|y_got - y| less the absolute term, in units of 2^-24 y."""
    with np.errstate(all="ignore"):
        e = np.maximum(np.abs(np.asarray(y_got, np.float64) - y) - Y_FLOOR, 0.0)
        return np.where(e == 0, 0.0, e / (EPS24 * y))


def tonemap_replay(rgba_f32):
    """The np.float32 chain: IEEE divide, clamp (NaN to 0), correctly rounded sqrt, IEEE multiply.  (y as float32, level)."""
    a = np.asarray(rgba_f32, F32)
    with np.errstate(all="ignore"):
        mean = a[..., :3] / a[..., 3:]
    m = np.minimum(np.maximum(np.where(np.isnan(mean), F32(0), mean), F32(0)), F32(1))
    y = np.sqrt(m) * SCALE_255
    assert y.dtype == F32
    return y, y.astype(np.int64)


TONEMAP_FILMS = ((1, 1), (3, 2), (37, 21), (255, 1), (1, 257), (64, 5))
COUNTS = (1.0, 3.0, 7.0, 1024.0, 2.0 ** 24)


def tonemap_cases(seed=SEED):
    """(rgba float32 (N, 4) with one case per colour channel, family (N, 3)):
      boundary   for every level k in 1..255 the mean (k / 255.99)^2 and its +-1, +-2, +-8 fp32 neighbours, as sums over each count of COUNTS
      special    count 0 with sum 0, a positive and a negative sum; inf, -inf and NaN sums; negative means
      above_one  means 1 +- 2^-23, 1.5, 1e30
      denormal   denormal sums
      generic    log-uniform means"""
    rng = np.random.default_rng(seed + 2)
    vals, fam = [], []                                                           # (sum, count) per channel case

    def add(family, s, c):
        s = np.asarray(s, np.float64).reshape(-1); c = np.broadcast_to(np.asarray(c, np.float64), s.shape)
        vals.append(np.stack([s, c], 1).astype(F32)); fam.append(np.full(len(s), family))

    k = np.arange(1, 256, dtype=np.float64)
    edge = ((k / np.float64(SCALE_255)) ** 2).astype(F32)
    means = np.concatenate([_steps(edge, s) for s in (-8, -2, -1, 0, 1, 2, 8)])
    for c in COUNTS:
        add("boundary", (means * F32(c)).astype(F32), c)                        # (the fp32 product: the mean the film holds is sum / count, whatever it is)
    add("special", [0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, np.inf, np.nan, -0.25, -1e30, -0.0], [0, 0, 0, 1, 1, 1, 0, 0, 1, 7, 3])
    add("above_one", [1 + 2.0 ** -23, 1 - 2.0 ** -23, 1.5, 1e30, 3 * (1 + 2.0 ** -23)], [1, 1, 1, 1, 3])
    add("denormal", [2.0 ** -149, 3 * 2.0 ** -149, 2.0 ** -127, 1e-39, 2.0 ** -130], [1, 3, 1, 7, 1024])
    m = 3000
    add("generic", np.exp(rng.uniform(np.log(1e-6), np.log(1.2), m)) * rng.choice(COUNTS, m), 0)
    v, f = np.concatenate(vals), np.concatenate(fam)
    g = f == "generic"
    v[g, 1] = rng.choice(COUNTS, g.sum()).astype(F32); v[g, 0] = (np.exp(rng.uniform(np.log(1e-6), np.log(1.2), g.sum())) * v[g, 1]).astype(F32)
    # three cases share a pixel and with it its count: group by count, fill a group up to a multiple of three with a plain mean
    rgba, family = [], []
    key = v[:, 1].view(np.uint32)
    for c in np.unique(key):
        sel = np.flatnonzero(key == c)
        cnt = v[sel[0], 1]
        s = v[sel, 0]; ff = f[sel]
        pad = (-len(s)) % 3
        s = np.concatenate([s, np.full(pad, F32(0.25) * cnt if cnt > 0 else F32(0.25), F32)]); ff = np.concatenate([ff, np.full(pad, "generic")])
        px = np.zeros((len(s) // 3, 4), F32); px[:, :3] = s.reshape(-1, 3); px[:, 3] = cnt
        rgba.append(px); family.append(ff.reshape(-1, 3))
    rgba, family = np.concatenate(rgba), np.concatenate(family)
    order = rng.permutation(len(rgba))
    return rgba[order], family[order]


def tonemap_films(rgba, family, width, height):
    """Every case as (h, w, 4) films of width x height with their (h, w, 3) families: as many films as the cases need (the last one wraps around)."""
    n = width * height
    for start in range(0, len(rgba), n):
        idx = np.arange(start, start + n) % len(rgba)
        yield rgba[idx].reshape(height, width, 4), family[idx].reshape(height, width, 3)
