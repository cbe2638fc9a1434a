"""The fp64 restatement of the trace kernels' triangle test (tri_test / tri_accept_closest / tri_accept_any, csrc/pt_device.h) with an error model, the
answers it ADMITS for a ray, and the scenes, hard poses and ray families of tests/test_trace_ref.py (CPU), tests/test_trace_edges.py and
tests/test_refit_hard.py (GPU).  Plain numpy.

Records.  The restatement starts from what the device holds, formed as kit.brute_force_trace(..., np.float32) forms it: first corner and ray origin less
the fp64 centre of the used vertices, edges from the world coordinates, direction, all rounded to fp32.  Moeller-Trumbore is evaluated on those fp32
values in fp64, so input rounding is out of the picture: what remains between this and any fp32 kernel is the arithmetic of tri_test.

Error model.  Beside each of a, t, u, v stands its absolute-value form: the same expression with every product and every difference replaced by the
sum of the magnitudes; for the quotients (|num|_abs + |x| |a|_abs) / |a|.  The bound of a quantity is K 2^-24 times that form.  K = 8 is measured by
tests/test_trace_ref.py (an fp32 restatement of tri_test's fma chains with the reciprocal off by +-1 ulp: tri_test32), not assumed.

Classification.  Under either acceptance rule a triangle is SURE (every inequality holds by more than its bound), REJ (one fails by more than its
bound) or DOUBT.  Closest hit: T* = the smallest t + bound over the SURE triangles; face k is admissible iff it is SURE or DOUBT and t_k - bound_k <=
T*; a miss is admissible iff no triangle is SURE; the reported t, u, v lie within face k's bounds.  Any hit: "blocked" is required if a triangle is
SURE, forbidden if none is SURE or DOUBT.  Every ray has an admissible set; none is excluded.
"""
from __future__ import annotations

import dataclasses
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F32 = np.float32
EPS = 2.0 ** -24
K = 8.0                                                      # measured: test_trace_ref.py::test_k_is_measured (worst ratios in DESIGN.md)
A_CLOSEST, A_ANY, T_MIN, T_MAX = float(F32(1e-5)), float(F32(1e-6)), float(F32(1e-4)), float(F32(3.0e38))
REJ, DOUBT, SURE = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------------------ the triangle test
def _xyz(a):
    return a[..., 0], a[..., 1], a[..., 2]


def _cross(a, b, A, B):
    return ((a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]),
            (A[1] * B[2] + A[2] * B[1], A[2] * B[0] + A[0] * B[2], A[0] * B[1] + A[1] * B[0]))


def _dot(a, b, A, B):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2], A[0] * B[0] + A[1] * B[1] + A[2] * B[2]


def mt64(v0, e1, e2, o, d, k=K):
    """Moeller-Trumbore in fp64 on (broadcastable) fp32 records: {a, t, u, v, w = 1 - u - v} and the bounds {ba, bt, bu, bv, bw}."""
    v0, e1, e2, o, d = (_xyz(np.asarray(x, np.float64)) for x in (v0, e1, e2, o, d))
    ab = lambda x: tuple(np.abs(c) for c in x)
    h, H = _cross(d, e2, ab(d), ab(e2))
    a, A = _dot(e1, h, ab(e1), H)
    s = tuple(p - q for p, q in zip(o, v0)); S = tuple(np.abs(p) + np.abs(q) for p, q in zip(o, v0))
    q, Q = _cross(s, e1, S, ab(e1))
    nu, NU = _dot(s, h, S, H); nv, NV = _dot(d, q, ab(d), Q); nt, NT = _dot(e2, q, ab(e2), Q)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ia = 1.0 / a; aa = np.abs(ia)
        u, v, t = nu * ia, nv * ia, nt * ia
        f = k * EPS
        bu, bv, bt = f * (NU + np.abs(u) * A) * aa, f * (NV + np.abs(v) * A) * aa, f * (NT + np.abs(t) * A) * aa
        # fl(fl(1 - u) - v) and fl(u + v) each add at most two roundings of magnitude <= 1 + |u| + |v|
        bw = bu + bv + 2.0 * EPS * (1.0 + np.abs(u) + np.abs(v))
        return dict(a=a, t=t, u=u, v=v, w=1.0 - u - v, ba=f * A, bt=bt, bu=bu, bv=bv, bw=bw)


def classify(m, t2, any_rule):
    """REJ / DOUBT / SURE of mt64's result under tri_accept_closest (t1 = 1e-4f, t < 3e38f) or tri_accept_any (t <= t2)."""
    thr = A_ANY if any_rule else A_CLOSEST
    with np.errstate(invalid="ignore"):
        aa = np.abs(m["a"])
        sure = (aa - m["ba"] > thr) & (m["t"] - m["bt"] > T_MIN) & (m["t"] + m["bt"] < t2) & (m["u"] - m["bu"] > 0) & (m["v"] - m["bv"] > 0) & (m["w"] - m["bw"] > 0)
        rej = (aa + m["ba"] < thr) | (m["t"] + m["bt"] < T_MIN) | (m["t"] - m["bt"] > t2) | (m["u"] + m["bu"] < 0) | (m["v"] + m["bv"] < 0) | (m["w"] + m["bw"] < 0)
    return np.where(sure, SURE, np.where(rej, REJ, DOUBT)).astype(np.int8)


def _r(x):
    return np.asarray(x, np.float64).astype(F32)


def _fma(a, b, c):
    """fp32 fma: the fp64 multiply-add (the product of two fp32 values is exact in fp64) rounded once to fp32."""
    return _r(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def _mul(a, b):
    return _r(a.astype(np.float64) * b.astype(np.float64))


def tri_test32(v0, e1, e2, o, d, rcp_ulps=0):
    """tri_test of pt_device.h restated in fp32, fma chain for fma chain; the reciprocal is the correctly rounded one moved by `rcp_ulps` fp32 steps
    (v_rcp_f32 is good to 1 ulp).  (a, t, u, v) as fp32."""
    v0, e1, e2, o, d = (_xyz(np.asarray(x, F32)) for x in (v0, e1, e2, o, d))
    hx = _fma(d[1], e2[2], -_mul(e2[1], d[2])); hy = _fma(d[2], e2[0], -_mul(e2[2], d[0])); hz = _fma(d[0], e2[1], -_mul(e2[0], d[1]))
    a = _fma(e1[2], hz, _fma(e1[1], hy, _mul(e1[0], hx)))
    sx, sy, sz = (_r(p.astype(np.float64) - q.astype(np.float64)) for p, q in zip(o, v0))
    qx = _fma(sy, e1[2], -_mul(e1[1], sz)); qy = _fma(sz, e1[0], -_mul(e1[2], sx)); qz = _fma(sx, e1[1], -_mul(e1[0], sy))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = _r(1.0 / a.astype(np.float64))
        step = np.broadcast_to(np.asarray(rcp_ulps), inv.shape)
        inv = np.where(step > 0, np.nextafter(inv, F32(np.inf)), np.where(step < 0, np.nextafter(inv, F32(-np.inf)), inv)).astype(F32)
        u = _mul(_fma(sz, hz, _fma(sy, hy, _mul(sx, hx))), inv)
        v = _mul(_fma(d[2], qz, _fma(d[1], qy, _mul(d[0], qx))), inv)
        t = _mul(_fma(e2[2], qz, _fma(e2[1], qy, _mul(e2[0], qx))), inv)
    return a, t, u, v


def k_trial(n=1_000_000, seed=1):
    """The measurement behind K: `n` random (triangle, ray) pairs -- scales 1e-3, 1 and 1e3, an offset of 100 on a third, triangle sizes 1e-4 .. 3
    of the scale, a third of the directions with a zeroed component, the reciprocal off by -1, 0 or +1 ulp -- and the worst
    |x32 - x64| / (2^-24 abs-form) of a, t, u, v over the pairs whose |a| is at least the smaller acceptance threshold (1e-6)."""
    rng = np.random.default_rng(seed)
    scale = np.array([1e-3, 1.0, 1e3])[rng.integers(0, 3, n)][:, None]
    off = np.where(rng.integers(0, 3, (n, 1)) == 0, 100.0, 0.0) * rng.uniform(-1, 1, (n, 3))
    size = 10.0 ** rng.uniform(-4, np.log10(3.0), (n, 1))
    c = rng.uniform(-1, 1, (n, 3))
    p = ((c[:, None, :] + size[:, None, :] * rng.normal(size=(n, 3, 3))) * scale[:, None, :] + off[:, None, :])
    w = rng.dirichlet((1, 1, 1), n)
    tgt = np.einsum("nk,nkd->nd", w, p) + 0.2 * size * scale * rng.normal(size=(n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    z = rng.integers(0, 3, n) == 0
    d[z, rng.integers(0, 3, z.sum())] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = tgt - d * scale * rng.uniform(0.01, 3.0, (n, 1))
    v0, e1, e2, o, d = _r(p[:, 0]), _r(p[:, 1] - p[:, 0]), _r(p[:, 2] - p[:, 0]), _r(o), _r(d)
    m = mt64(v0, e1, e2, o, d, k=1.0)
    a, t, u, v = tri_test32(v0, e1, e2, o, d, rng.integers(-1, 2, n))
    ok = np.abs(m["a"]) >= A_ANY
    with np.errstate(invalid="ignore", divide="ignore"):
        return {x: float(np.max((np.abs(g.astype(np.float64) - m[x]) / m["b" + x])[ok])) for x, g in (("a", a), ("t", t), ("u", u), ("v", v))}


# ------------------------------------------------------------------------------------------------------------------------ records and the restatement
def centre_of(scene):
    used = scene.vertex[scene.face[:, :, 0]].astype(np.float64).reshape(-1, 3)
    return 0.5 * used.min(0) + 0.5 * used.max(0)


def records(scene, origin, direction, centre=None):
    """(v0, e1, e2, o, d) as fp32, the way scene_build.cpp / refit.hip and the probes form them.  centre: that of the scene the context was created
    with, where `scene` is a later pose of it (mcpt_update_vertices keeps the centre)."""
    p = scene.vertex[scene.face[:, :, 0]].astype(np.float64)
    ctr = centre_of(scene) if centre is None else np.asarray(centre, np.float64)
    return (_r(p[:, 0] - ctr), _r(p[:, 1] - p[:, 0]), _r(p[:, 2] - p[:, 0]),
            _r(np.asarray(origin, np.float64).reshape(-1, 3) - ctr), _r(np.asarray(direction, np.float64).reshape(-1, 3)))


def clamp_t2(t2):
    """The limit a probe hands its kernel: float(t2), 3e38f above 3e38."""
    t2 = np.asarray(t2, np.float64)
    with np.errstate(over="ignore"):
        return np.where(t2 > 3.0e38, F32(3.0e38), t2.astype(F32)).astype(F32)


_SPARSE = ("ray", "face", "sc", "sa", "a", "t", "u", "v", "ba", "bt", "bu", "bv")


class Restatement:
    """What restate() found: per ray T*, the counts of SURE triangles under either rule and of admissible answers; per (ray, triangle) that is not REJ
    under both rules, its class under either rule, its fp64 a, t, u, v and their bounds."""

    def __init__(self, n, n_faces, t_star, sparse):
        self.n, self.n_faces, self.t_star = n, n_faces, t_star
        for k in _SPARSE: setattr(self, k, sparse[k])
        self.key = self.ray.astype(np.int64) * n_faces + self.face                      # sorted: rays in order, faces in order within a ray
        assert np.all(np.diff(self.key) > 0)
        self.sure_closest = np.bincount(self.ray[self.sc == SURE], minlength=n)
        self.sure_any = np.bincount(self.ray[self.sa == SURE], minlength=n)
        self.open_any = np.bincount(self.ray[self.sa != REJ], minlength=n)
        with np.errstate(invalid="ignore"):
            self.adm = (self.sc != REJ) & ~(self.t - self.bt > t_star[self.ray])
        self.miss_ok = self.sure_closest == 0
        self.n_admissible = np.bincount(self.ray[self.adm], minlength=n) + self.miss_ok
        self.forced_any = (self.sure_any > 0) | (self.open_any == 0)

    def admissible(self, i):
        """The admissible closest-hit answers of ray i: face indices, -1 for a miss."""
        return sorted(self.face[(self.ray == i) & self.adm].tolist()) + ([-1] if self.miss_ok[i] else [])

    def single(self):
        """Per ray: its one admissible closest-hit answer (-1: a miss), or -2 where it has several."""
        out = np.full(self.n, -2, np.int64)
        one = self.n_admissible == 1
        out[one & self.miss_ok] = -1
        m = self.adm & one[self.ray]
        out[self.ray[m]] = self.face[m]
        return out

    def check_closest(self, face, t, u, v):
        """A kernel's closest-hit answers -> (bad: per ray, the answer is not admissible; ratio: the worst |reported - fp64| / bound of t, u, v where the
        face is admissible (infinite beyond the bound), 0 elsewhere).  A value beyond its bound makes the ray bad."""
        face = np.asarray(face, np.int64); hit = face >= 0
        if self.key.size == 0:                                                       # no triangle that could be hit: only a miss is admissible
            return hit | ~self.miss_ok, np.zeros(self.n)
        rep = np.arange(self.n, dtype=np.int64) * self.n_faces + np.where(hit, face, 0)
        j = np.minimum(np.searchsorted(self.key, rep), self.key.size - 1)
        ok_face = hit & (self.key[j] == rep) & self.adm[j]
        ratio = np.zeros(self.n)
        with np.errstate(invalid="ignore", divide="ignore"):
            for got, x, b in ((t, self.t, self.bt), (u, self.u, self.bu), (v, self.v, self.bv)):
                err = np.abs(np.asarray(got, np.float64) - x[j]); bound = b[j]
                r = np.where(err == 0, 0.0, np.where(err <= bound, err / bound, np.inf))
                ratio = np.maximum(ratio, np.where(ok_face, np.nan_to_num(r, nan=0.0, posinf=np.inf), 0.0))   # a NaN bound (a == 0) forgives nothing it could check
        bad = np.where(hit, ~ok_face | ~(ratio <= 1.0), ~self.miss_ok)
        return bad, ratio

    def check_any(self, blocked):
        """A kernel's any-hit verdicts -> bad per ray: not blocked where a triangle is SURE, blocked where none is SURE or DOUBT."""
        blocked = np.asarray(blocked) != 0
        return np.where(blocked, self.open_any == 0, self.sure_any > 0)


def restate(scene, origin, direction, t2=None, centre=None, pairs_per_chunk=30_000):
    """The Restatement of every ray against EVERY triangle of `scene`; t2: the any-hit limits as the caller hands them to a probe (default: none).
    Chunks of rays small enough to stay in cache, a few of them at a time (numpy releases the interpreter lock inside its loops)."""
    v0, e1, e2, o, d = records(scene, origin, direction, centre)
    n, nf = o.shape[0], v0.shape[0]
    t2 = np.full(n, T_MAX) if t2 is None else clamp_t2(t2).astype(np.float64)
    chunk = max(1, pairs_per_chunk // nf)

    def work(b):
        m = mt64(v0[None], e1[None], e2[None], o[b:b + chunk, None, :], d[b:b + chunk, None, :])
        sc = classify(m, T_MAX, False); sa = classify(m, t2[b:b + chunk, None], True)
        with np.errstate(invalid="ignore"):
            ts = np.where(sc == SURE, m["t"] + m["bt"], np.inf).min(1)
        r, f = np.nonzero((sc != REJ) | (sa != REJ))
        part = {"ray": r + b, "face": f, "sc": sc[r, f], "sa": sa[r, f]}
        part.update({k: np.broadcast_to(m[k], sc.shape)[r, f] for k in _SPARSE[4:]})
        return ts, part

    with ThreadPoolExecutor(max(1, min(8, (os.cpu_count() or 1)))) as pool:
        done = list(pool.map(work, range(0, n, chunk)))
    t_star = np.concatenate([ts for ts, _ in done]) if done else np.zeros(0)
    empty = {k: np.zeros(0, np.int64 if k in ("ray", "face") else np.int8 if k in ("sc", "sa") else np.float64) for k in _SPARSE}
    return Restatement(n, nf, t_star, {k: np.concatenate([p[k] for _, p in done] + [empty[k]]) for k in _SPARSE})


def joined(a, b):
    """The Restatement of a's rays followed by b's."""
    sparse = {k: np.concatenate([getattr(a, k), getattr(b, k) + (a.n if k == "ray" else 0)]) for k in _SPARSE}
    return Restatement(a.n + b.n, a.n_faces, np.concatenate([a.t_star, b.t_star]), sparse)


def describe(rs, rays, i, face):
    """The words of a failure message: family, ray, reported face, admissible set."""
    return "family %s, ray %d: origin %r direction %r reported face %d, admissible %r" % (
        rays["family"][i], i, rays["origin"][i].tolist(), rays["direction"][i].tolist(), int(face), rs.admissible(i))


# ------------------------------------------------------------------------------------------------------------------------ scenes
GRID = 16                                                    # wall cells per side of room16: 6 x 16 x 16 x 2 = 3 072 triangles


def _materials(S):
    return [S.Material("grey", kd=(0.6, 0.6, 0.6)), S.Material("lamp", kd=(0.0, 0.0, 0.0), radiance=(5.0, 5.0, 5.0))]


def room(pkg, scale=1.0, offset=(0.0, 0.0, 0.0), grid=GRID, name="room16"):
    """The closed unit cube, each wall a grid x grid lattice of quads on the k / grid lattice (the ceiling is the light), scaled by the power of two
    `scale` and moved by `offset`: every vertex is exact in fp32, and stays so less the centre."""
    S = pkg.scenes; m = S._Mesh()
    for a in range(3):
        for side in (0.0, 1.0):
            o = np.zeros(3); o[a] = side
            du = np.zeros(3); du[(a + 1) % 3] = 1.0
            dv = np.zeros(3); dv[(a + 2) % 3] = 1.0
            nrm = np.zeros(3); nrm[a] = 1.0 - 2.0 * side
            m.add_grid(o, du, dv, grid, grid, nrm, 1 if (a == 1 and side == 1.0) else 0)
    base = m.finish(name, _materials(S), S._qcam((0.5, 0.5, 0.9), (0.5, 0.5, 0.0), (0, 1, 0), 40.0, 16, 16))
    assert np.array_equal(base.vertex * grid, np.rint(base.vertex * grid))             # on the lattice, exactly
    off = np.asarray(offset, np.float64)
    v = base.vertex * scale + off
    c = base.camera
    cam = S.Camera(tuple(np.asarray(c.eye) * scale + off), tuple(np.asarray(c.lookat) * scale + off), c.up, c.fovy, c.width, c.height)
    scene = S.SceneData(name, v, base.normal, base.texcoord, base.face, base.materials, cam, {"scale": float(scale), "offset": tuple(off), "grid": grid})
    ctr = centre_of(scene)
    assert np.array_equal(v, v.astype(F32)) and np.array_equal(v - ctr, (v - ctr).astype(F32))
    return scene


def _triangles(pkg, name, tri, offset=(0.0, 0.0, 0.0)):
    """(n, 3, 3) triangles, own vertices each, through scenes._Mesh; triangle 0 is the light; vertices exact in fp32."""
    S = pkg.scenes; m = S._Mesh()
    tri = (np.asarray(tri, np.float64) + np.asarray(offset, np.float64)).astype(F32).astype(np.float64)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]); nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    base = m.add_vertices(tri.reshape(-1, 3), np.repeat(nrm, 3, axis=0), np.zeros((3 * tri.shape[0], 2)))
    f = np.arange(3 * tri.shape[0], dtype=np.int64).reshape(-1, 3) + base
    m.f.append(np.concatenate([f, (np.arange(tri.shape[0]) == 0).astype(np.int64)[:, None]], 1))
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0); c = 0.5 * (lo + hi); r = float(np.linalg.norm(hi - lo)) + 1.0
    scene = m.finish(name, _materials(S), S.Camera(tuple(c + np.array([0.3, 0.5, 1.0]) * 1.5 * r), tuple(c), (0.0, 1.0, 0.0), 40.0, 16, 16))
    scene = S.SceneData(name, tri.reshape(-1, 3), scene.normal, scene.texcoord, scene.face, scene.materials, scene.camera, {"offset": tuple(offset)})
    assert np.array_equal(scene.vertex, scene.vertex.astype(F32))
    return scene


def soup(pkg, offset=(0.0, 0.0, 0.0), n=1500, seed=7, name="soup"):
    """`n` random triangles, sizes log-uniform 1e-4 .. 1, centres in a unit cube."""
    rng = np.random.default_rng(seed)
    size = 10.0 ** rng.uniform(-4, 0, (n, 1, 1))
    tri = rng.uniform(0, 1, (n, 1, 3)) + size * rng.uniform(-0.5, 0.5, (n, 3, 3))
    return _triangles(pkg, name, tri, offset)


SCENES = {
    "room16": lambda pkg: room(pkg),
    "room16-small": lambda pkg: room(pkg, scale=2.0 ** -6, name="room16-small"),
    "room16-large": lambda pkg: room(pkg, scale=2.0 ** 6, name="room16-large"),
    "room16-moved": lambda pkg: room(pkg, offset=(1024.0, -2048.0, 512.0), name="room16-moved"),
    "soup": lambda pkg: soup(pkg),
    "soup-moved": lambda pkg: soup(pkg, offset=(5e3, -3.0, 0.25), name="soup-moved"),
    "one": lambda pkg: _triangles(pkg, "one", [[[0, 0, 0], [1, 0, 0], [0, 1, 0]]]),
    "two": lambda pkg: _triangles(pkg, "two", [[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 0, 0], [1, 1, 0], [0, 1, 0]]]),
}
ROOMS = ("room16", "room16-small", "room16-large", "room16-moved")


def displaced(scene):
    """room16 with the wall interiors moved smoothly (the rim of every wall, and so the bounding box and the centre, stay): the pose of the refit test."""
    s = scene.meta["scale"]; off = np.asarray(scene.meta["offset"])
    x = (scene.vertex - off) / s
    rim = ((x == 0) | (x == 1)).sum(1) >= 2
    bump = 0.04 * np.sin(np.pi * x[:, [1, 2, 0]]) * np.sin(np.pi * x[:, [2, 0, 1]])     # zero on the rim, along the wall's own axis
    wall = (x == 0) | (x == 1)
    y = x + np.where(wall & ~rim[:, None], np.where(x == 0, 1.0, -1.0) * bump, 0.0)
    return dataclasses.replace(scene, vertex=(y * s + off).astype(F32).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------------ hard poses
# Each pose: creation scene -> posed vertices (fp64, before the rounding to fp32 values that posed() applies).  c is the creation centre, the one
# the context keeps.  The magnitudes keep every intermediate of tri_test inside fp32 range, which is what the error model assumes.
FAR = np.array([64.0, -128.0, 32.0])
STRETCH = np.array([2.0 ** 12, 1.0, 2.0 ** -12])
FOLD = 3.0                    # (were a pose to miss the condition test_trace_ref.py sets for it, its magnitude is what gets halved, not the condition)


def _used(scene):
    return np.unique(scene.face[:, :, 0])


def _scramble(scene, c):
    v = scene.vertex.copy(); used = _used(scene)
    v[used] = scene.vertex[np.random.default_rng(11).permutation(used)]
    return v


def _mirror(scene, c):
    v = scene.vertex.copy(); v[:, 0] = 2.0 * c[0] - v[:, 0]
    return v


def _fold(scene, c):
    v = scene.vertex.copy()
    v[:, 1] += FOLD * np.sin(40.0 * v[:, 0]); v[:, 2] += FOLD * np.cos(31.0 * v[:, 1])      # (z from the folded y)
    return v


def _flatten(axes):
    def pose(scene, c):
        v = scene.vertex.copy(); v[:, axes] = c[list(axes)]
        return v
    return pose


def _third_degenerate(scene, c):
    f = scene.face[::3, :, 0]
    assert np.unique(scene.face[:, :, 0]).size == 3 * scene.face.shape[0]              # the triangles own their vertices
    v = scene.vertex.copy(); v[f[:, 1]] = v[f[:, 0]]; v[f[:, 2]] = v[f[:, 0]]
    return v


POSES = {
    "scramble": _scramble,                                              # the used vertices permuted among their own positions: every triangle spans the scene
    "stretch": lambda s, c: (s.vertex - c) * STRETCH + c,               # extents 2^24 apart between x and z
    "far": lambda s, c: s.vertex + FAR,                                 # far from the creation centre, the step of a frame stays small
    "mirror": _mirror,                                                  # x reflected about the centre: every winding flips
    "fold": _fold,
    "plane": _flatten((2,)),                                            # flat on z
    "line": _flatten((1, 2)),
    "point": _flatten((0, 1, 2)),                                       # every triangle degenerate, the light's area 0
    "third-degenerate": _third_degenerate,                              # every third triangle collapsed onto its first corner (soup only)
}
COLLAPSED = ("plane", "line", "point")                                  # rays of the creation scene: _soup_rays divides by their zero areas
POSE_SCENES = {p: (("soup",) if p == "third-degenerate" else ("soup", "room16")) + (("one", "two") if p in ("far", "mirror") else ()) for p in POSES}
POSE_CASES = [(s, p) for p in POSES for s in POSE_SCENES[p]]


def posed(scene, pose):
    """`scene` in pose POSES[pose]: the vertices rounded to fp32 values, everything else kept."""
    return dataclasses.replace(scene, vertex=np.asarray(POSES[pose](scene, centre_of(scene)), np.float64).astype(F32).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------------ rays
NEAR_AXIS = [F32(x) for x in (1e-38, 1e-31, 1e-30, 1e-29, 1e-20, 1e-8)] + [np.nextafter(F32(1e-30), F32(1)), np.nextafter(F32(1e-30), F32(0)), F32(1.0000001e-30)]
START_NEAR = [F32(0), F32(0.5e-4), np.nextafter(F32(1e-4), F32(0)), F32(1e-4), np.nextafter(F32(1e-4), F32(1)), F32(2e-4), F32(1e-3)]
ULPS_OFF = (1, 2, 10, 100)
N_FAMILY = 500
N_T2_SOURCE = 50                                             # rays of every family that the t2 family copies, four times each
T2_KINDS = ("t", "t-", "t+", "t(1-2^-20)", "t(1+2^-20)", "t/2", "3e38", ">3e38")


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _signed_zero(rng, shape):
    return np.where(rng.integers(0, 2, shape) == 0, 0.0, -0.0)


def _axis_dirs(rng, n):
    """+-e_i with every combination of +0.0 and -0.0 in the two zero components; (directions, axis)."""
    ax = rng.integers(0, 3, n)
    d = _signed_zero(rng, (n, 3))
    d[np.arange(n), ax] = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)
    return d, ax


def _near_axis_dirs(rng, n):
    ax = rng.integers(0, 3, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    d = np.zeros((n, 3))
    d[np.arange(n), (ax + 1) % 3] = np.cos(ang); d[np.arange(n), (ax + 2) % 3] = np.sin(ang)
    val = np.array(NEAR_AXIS, np.float64)[np.arange(n) % len(NEAR_AXIS)]
    d[np.arange(n), ax] = val * np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)
    return d


def _aim(o, tgt):
    d = tgt - o
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _ulp_steps(x, k):
    """fp32 x moved by k fp32 steps (k an integer array, either sign)."""
    x = np.ascontiguousarray(x, F32)
    i = x.view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7fffffff), i) + k                                       # sign-magnitude -> ordered integers
    i = np.where(i < 0, (-i) | 0x80000000, i)
    return i.astype(np.uint32).view(F32)


def _room_families(rng, n=N_FAMILY, grid=GRID):
    """The families of a room, in the coordinates of the unit cube: a list of (family, origins, directions)."""
    out = []
    interior = lambda k: rng.uniform(0.05, 0.95, (k, 3))
    lattice = lambda k: rng.integers(1, grid, k) / grid
    # axis_on_planes comes FIRST and twice the size: whole waves of same-octant rays
    d, ax = _axis_dirs(rng, 2 * n); o = interior(2 * n)
    both = rng.integers(0, 2, 2 * n) == 0
    o[np.arange(2 * n), (ax + 1) % 3] = lattice(2 * n)
    o[both, (ax[both] + 2) % 3] = lattice(int(both.sum()))
    order = np.lexsort((d[np.arange(2 * n), ax], ax))                                   # runs of one axis and sign
    out.append(("axis_on_planes", o[order], d[order]))
    d, ax = _axis_dirs(rng, n)
    out.append(("axis", interior(n), d))
    # in_wall: origin on a wall, direction in that wall's plane
    a = rng.integers(0, 3, n); o = interior(n); o[np.arange(n), a] = rng.integers(0, 2, n).astype(np.float64)
    snap = rng.integers(0, 3, n) == 0; o[snap, (a[snap] + 1) % 3] = lattice(int(snap.sum()))
    ang = rng.uniform(0, 2 * np.pi, n); d = np.zeros((n, 3))
    d[np.arange(n), (a + 1) % 3] = np.cos(ang); d[np.arange(n), (a + 2) % 3] = np.sin(ang); d[np.arange(n), a] = _signed_zero(rng, n)
    axial = rng.integers(0, 4, n) == 0                                                  # a quarter run along a lattice direction as well
    d[axial] = 0.0; d[axial, (a[axial] + 1) % 3] = np.where(rng.integers(0, 2, int(axial.sum())) == 0, 1.0, -1.0)
    out.append(("in_wall", o, d))
    out.append(("near_axis", interior(n), _near_axis_dirs(rng, n)))
    # start_near: is filled in by rays() in the scene's own fp32 coordinates (the distances are absolute)
    out.append(("start_near", None, None))
    # edges: generic origins aimed at lattice vertices, edge midpoints (axis-parallel and diagonal edges) and points a few fp32 steps off an edge
    a = rng.integers(0, 3, n); tgt = np.zeros((n, 3)); tgt[np.arange(n), a] = rng.integers(0, 2, n).astype(np.float64)
    kind = np.arange(n) % 4
    i, j = rng.integers(0, grid, n), rng.integers(0, grid, n)
    p = np.where(kind == 0, i, np.where(kind == 1, i + 0.5, np.where(kind == 2, i + 0.5, i + rng.uniform(0.1, 0.9, n)))) / grid
    q = np.where(kind == 0, j, np.where(kind == 1, j, np.where(kind == 2, j + 0.5, j))) / grid
    tgt[np.arange(n), (a + 1) % 3] = p; tgt[np.arange(n), (a + 2) % 3] = q
    out.append(("edges", interior(n), ("aim", tgt, np.where(kind == 3, (a + 2) % 3, -1))))           # kind 3: off the lattice line q, across it
    # corners: aimed at the cube's 8 corners, and along its 12 edges (origin on the edge's line, inside the cube or on its end)
    h = n // 2
    corner = rng.integers(0, 2, (h, 3)).astype(np.float64)
    o2 = np.zeros((n - h, 3)); a = rng.integers(0, 3, n - h)
    o2[np.arange(n - h), (a + 1) % 3] = rng.integers(0, 2, n - h); o2[np.arange(n - h), (a + 2) % 3] = rng.integers(0, 2, n - h)
    o2[np.arange(n - h), a] = np.where(rng.integers(0, 3, n - h) == 0, rng.integers(0, grid + 1, n - h) / grid, rng.uniform(0, 1, n - h))
    d2 = _signed_zero(rng, (n - h, 3)); d2[np.arange(n - h), a] = np.where(rng.integers(0, 2, n - h) == 0, 1.0, -1.0)
    out.append(("corners", interior(h), ("aim", corner, np.full(h, -1))))
    out.append(("corners", o2, d2))
    out.append(("generic", interior(n), _unit(rng, n)))
    return out


def _room_rays(scene, rng):
    s = scene.meta["scale"]; g = scene.meta["grid"]; ctr = centre_of(scene)
    local = lambda x: _r((np.asarray(x, np.float64) - 0.5) * s)                         # unit-cube coordinates -> the device's fp32 coordinates
    O, D, F = [], [], []
    for fam, o, d in _room_families(rng, grid=g):
        if fam == "start_near":
            n = N_FAMILY
            a = rng.integers(0, 3, n); side = rng.integers(0, 2, n).astype(np.float64)
            p = rng.uniform(0.05, 0.95, (n, 3)); p[np.arange(n), a] = side
            d = _unit(rng, n)
            toward = np.arange(n) % 3 != 0                                              # a third points away from the wall it starts near
            da = np.abs(d[np.arange(n), a]) * np.where(side == 1, 1.0, -1.0) * np.where(toward, 1.0, -1.0)
            d[np.arange(n), a] = np.where(np.abs(da) < 0.05, np.sign(da) * 0.05, da)
            d = _r(d / np.linalg.norm(d, axis=1, keepdims=True))
            tau = np.array(START_NEAR, np.float64)[(np.arange(n) // 3) % len(START_NEAR)]
            pl = local(p).astype(np.float64)
            o = _r(pl - np.where(toward, 1.0, -1.0)[:, None] * tau[:, None] * d.astype(np.float64))
        else:
            o = local(o)
            if isinstance(d, tuple):
                _, tgt, across = d                                                  # across: the coordinate to move off its lattice line, or -1
                tl = local(tgt); m = tl.shape[0]; off = across >= 0; c = np.maximum(across, 0)
                k = np.where(off, np.array(ULPS_OFF)[rng.integers(0, 4, m)] * np.where(rng.integers(0, 2, m) == 0, 1, -1), 0)
                tl[np.arange(m), c] = _ulp_steps(tl[np.arange(m), c], k)
                d = _aim(o.astype(np.float64), tl.astype(np.float64))
            d = _r(d)
        O.append(o); D.append(d); F += [fam] * o.shape[0]
    return np.concatenate(O).astype(np.float64) + ctr, np.concatenate(D).astype(np.float64), np.array(F)


def _soup_rays(scene, rng):
    n = N_FAMILY
    p = scene.vertex[scene.face[:, :, 0]]
    nt = p.shape[0]
    ctr = centre_of(scene); lo, hi = p.reshape(-1, 3).min(0), p.reshape(-1, 3).max(0)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cr = np.cross(e1, e2); area2 = np.linalg.norm(cr, axis=1); nrm = cr / np.maximum(area2, 1e-300)[:, None]
    longest = np.maximum(np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)), np.linalg.norm(e2 - e1, axis=1))
    thin = area2 / longest ** 2                                                         # altitude over the longest edge
    cen = p.mean(1)
    inside = lambda k: rng.uniform(lo, hi, (k, 3))
    O, D, F = [], [], []
    def add(fam, o, d):
        O.append(o); D.append(d); F.extend([fam] * o.shape[0])
    d, _ = _axis_dirs(rng, n); add("axis", inside(n), d)
    add("near_axis", inside(n), _near_axis_dirs(rng, n))
    add("generic", inside(n), _unit(rng, n))
    # edges: aimed at a triangle's corner, an edge midpoint, or a point a few fp32 steps off an edge
    k = rng.integers(0, nt, n); kind = np.arange(n) % 3; c = rng.integers(0, 3, n)
    a_, b_ = p[k, c], p[k, (c + 1) % 3]
    tgt = np.where((kind == 0)[:, None], a_, np.where((kind == 1)[:, None], 0.5 * (a_ + b_), a_ + rng.uniform(0.1, 0.9, (n, 1)) * (b_ - a_)))
    steps = np.where(kind == 2, np.array(ULPS_OFF)[rng.integers(0, 4, n)] * np.where(rng.integers(0, 2, n) == 0, 1, -1), 0)
    tl = _r(tgt - ctr); ax = rng.integers(0, 3, n)
    tl[np.arange(n), ax] = _ulp_steps(tl[np.arange(n), ax], steps)
    d = _unit(rng, n); add("edges", tl.astype(np.float64) + ctr - d * rng.uniform(0.05, 0.5, (n, 1)), d)
    # start_near: origins the absolute distances of START_NEAR from a triangle of size >= 0.05, along the ray; a third point away
    big = np.nonzero(longest >= 0.05)[0] if (longest >= 0.05).any() else np.arange(nt)
    k = big[rng.integers(0, big.size, n)]; w = rng.dirichlet((1, 1, 1), n) * 0.7 + 0.1
    tgt = np.einsum("nk,nkd->nd", w, p[k]); d = _unit(rng, n)
    cs = np.einsum("nd,nd->n", d, nrm[k]); d = np.where((np.abs(cs) < 0.2)[:, None], nrm[k] * np.where(cs < 0, -1.0, 1.0)[:, None], d)   # no grazing starts: that is `grazing`'s business
    toward = np.arange(n) % 3 != 0
    tau = np.array(START_NEAR, np.float64)[(np.arange(n) // 3) % len(START_NEAR)]
    add("start_near", tgt - np.where(toward, 1.0, -1.0)[:, None] * tau[:, None] * d, d)
    # slivers: into the thinnest tenth, at the centroid
    thinnest = np.argsort(thin)[:max(1, nt // 10)]
    k = thinnest[rng.integers(0, thinnest.size, n)]; d = _unit(rng, n)
    add("slivers", cen[k] - d * rng.uniform(0.05, 0.5, (n, 1)), d)
    # det: |a| = |e1 x e2| |cos| log-uniform over 1e-7 .. 1e-4; grazing: |cos| log-uniform over 1e-6 .. 1e-3; both at the centroid of a large triangle
    large = np.nonzero(area2 >= 1e-3)[0] if (area2 >= 1e-3).any() else np.arange(nt)
    for fam, pick in (("det", lambda kk: 10.0 ** rng.uniform(-7, -4, n) / area2[kk]), ("grazing", lambda kk: 10.0 ** rng.uniform(-6, -3, n))):
        k = large[rng.integers(0, large.size, n)]
        cos = np.minimum(pick(k), 1.0) * np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)
        tang = np.cross(nrm[k], _unit(rng, n)); tang /= np.linalg.norm(tang, axis=1, keepdims=True)
        d = tang * np.sqrt(1.0 - cos ** 2)[:, None] + nrm[k] * cos[:, None]
        add(fam, cen[k] - d * (longest[k] * rng.uniform(0.3, 0.6, n))[:, None], d)
    o = np.concatenate(O); d = np.concatenate(D)
    return _r(o - ctr).astype(np.float64) + ctr, _r(d).astype(np.float64), np.array(F)


_cases = {}


def case(pkg, name):
    """(scene, rays, Restatement) of SCENES[name], computed once per session and never changed.  rays: origin (n, 3) and direction (n, 3) as fp64 holding
    fp32 values (the origin less the scene's centre is one), t2 (n,) the any-hit limit as handed to a probe (1e300: none), family (n,) and, for the
    rays of family t2, t2_kind and source (the ray it copies)."""
    if name in _cases:
        return _cases[name]
    scene = SCENES[name](pkg)
    rng = np.random.default_rng(1000 + sorted(SCENES).index(name))
    o, d, fam = (_room_rays if name in ROOMS else _soup_rays)(scene, rng)
    _cases[name] = (scene,) + with_t2_family(scene, o, d, fam)
    return _cases[name]


def with_t2_family(scene, o, d, fam, centre=None):
    """(rays, Restatement) of the base rays (o, d, fam) against `scene` followed by their t2 family.  centre: as in records()."""
    assert np.isfinite(o).all() and np.isfinite(d).all() and (np.abs(_r(d)) > 0).any(1).all()
    # the t2 family: copies of rays of every family, the limit around the fp32 hit distance of the nearest triangle of the fp64 restatement (1 where
    # there is none).  The five limits within 2^-20 of t leave the verdict open by construction (the bound of t is at least 2^-20 t), the other three
    # force it: each source ray gets one of the five and all of the three.
    base = restate(scene, o, d, centre=centre)
    src = np.concatenate([np.nonzero(fam == f)[0][:N_T2_SOURCE] for f in np.unique(fam)])
    v0, e1, e2, ol, dl = records(scene, o[src], d[src], centre)
    near = np.full(src.size, -1)
    cand = (base.sc != REJ) | (base.sa != REJ)
    for j, i in enumerate(src):
        m = np.nonzero((base.ray == i) & cand & (base.t > 0))[0]
        if m.size: near[j] = base.face[m[np.argmin(base.t[m])]]
    k = np.maximum(near, 0)
    t32 = tri_test32(v0[k], e1[k], e2[k], ol, dl)[1]
    t32 = np.where((near >= 0) & np.isfinite(t32) & (t32 > 0), t32, F32(1.0)).astype(F32)
    t64 = t32.astype(np.float64)
    limits = {"t": t64, "t-": np.nextafter(t32, F32(0)).astype(np.float64), "t+": np.nextafter(t32, F32(np.inf)).astype(np.float64),
              "t(1-2^-20)": t64 * (1 - 2.0 ** -20), "t(1+2^-20)": t64 * (1 + 2.0 ** -20), "t/2": t64 / 2, "3e38": np.full(src.size, 3.0e38),
              ">3e38": np.full(src.size, 1e300)}
    j = np.arange(src.size)
    kinds = np.concatenate([np.array(T2_KINDS[:5])[j % 5]] + [np.full(src.size, kk) for kk in T2_KINDS[5:]])
    src2 = np.tile(src, 4)
    t2 = np.array([limits[kk][jj] for kk, jj in zip(kinds, np.tile(j, 4))])
    nb = o.shape[0]
    rays = {"origin": np.concatenate([o, o[src2]]), "direction": np.concatenate([d, d[src2]]), "t2": np.concatenate([np.full(nb, 1e300), t2]),
            "family": np.concatenate([fam, np.array(["t2"] * src2.size)]), "t2_kind": np.concatenate([np.array([""] * nb, dtype=kinds.dtype), kinds]),
            "source": np.concatenate([np.arange(nb), src2])}
    rs = joined(base, restate(scene, o[src2], d[src2], t2, centre=centre))
    for a in rays.values(): a.setflags(write=False)
    return rays, rs


_pose_cases = {}


def pose_case(pkg, name, pose):
    """(creation scene, posed scene, rays, Restatement) of SCENES[name] moved into POSES[pose] by an update of a live context, once per session.
    The rays are _soup_rays of the posed scene (of the creation scene for the COLLAPSED poses) and their t2 family; the context keeps the CREATION
    centre, so the origins are fp32 values less that centre and the restatement forms its records about it."""
    if (name, pose) not in _pose_cases:
        scene = case(pkg, name)[0]
        moved = posed(scene, pose)
        ctr = centre_of(scene)
        with np.errstate(invalid="ignore", divide="ignore"):                           # (a degenerate triangle's altitude over its longest edge is 0 / 0)
            o, d, fam = _soup_rays(scene if pose in COLLAPSED else moved, np.random.default_rng(7))
        o = _r(o - ctr).astype(np.float64) + ctr
        _pose_cases[(name, pose)] = (scene, moved) + with_t2_family(moved, o, d, fam, centre=ctr)
    return _pose_cases[(name, pose)]


def family_table(rs, rays, ratio=None):
    """Per family: rays, share with a single admissible closest-hit answer, share with at most 8, share with a forced any-hit verdict and (given the
    ratios check_closest returned, in units of the bound) the worst error / bound."""
    rows = []
    for f in dict.fromkeys(rays["family"].tolist()):
        m = rays["family"] == f
        rows.append((f, int(m.sum()), float((rs.n_admissible[m] == 1).mean()), float((rs.n_admissible[m] <= 8).mean()), float(rs.forced_any[m].mean()),
                     None if ratio is None else float(ratio[m].max())))
    return rows


def print_table(title, rows):
    print("\n%s\n%-16s %6s %8s %8s %8s %s" % (title, "family", "rays", "single", "<= 8", "forced", "worst error / bound"))
    for f, n, one, few, forced, worst in rows:
        print("%-16s %6d %8.3f %8.3f %8.3f %s" % (f, n, one, few, forced, "" if worst is None else "%.3f" % worst))
