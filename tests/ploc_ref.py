"""A plain restatement of the device tree builder (csrc/bvh_gpu.hip: gpu_build_ploc) in numpy, fp32 where the kernels use fp32, and the scene
makers its tests share.  The steps, in the kernels' order: morton_kernel's 63-bit codes from the host's `lo` / `inv_ext`; a stable sort;
rounds of ploc_nn_kernel (nearest neighbour within +-16 positions by half_area of the merged box), ploc_merge_kernel (mutual pairs merge at
the lower position) and the compaction; then the host emission rule (subtrees of <= MCPT_LEAF_MAX = 2 triangles become leaves).

half_area is x*y + y*z + z*x with every product and sum rounded to fp32.  The device compiles it with contraction allowed, so the two agree
bit for bit only where the arithmetic is exact: the integer-lattice makers below (coincident, strip, grid, lattice_soup) are built so that every
coordinate, extent and merged area is an integer (or half-integer) below 2^24.  `shells` is not exact; it is asked for depth bands only.

What the restatement found (`tie="lower"`, the rule the kernel had: among equal merged areas the lower index wins).  That rule makes only the
FIRST pair of a run of equal areas mutual -- cluster i picks i - 16, which picks its own lower neighbour -- so a run merges one pair per round
and the tree is a chain: coincident(300) took 299 rounds to depth 298, coincident(5000) 4999 rounds (past the builder's 4096-round cap: the
context was refused), a strip of unit quads n/4 rounds.  `tie="pair"` is the kernel's rule now: among equal areas the even-odd partner i ^ 1,
else the lower index; tests/test_ploc_ref.py pins the figures of both.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
RADIUS = 16                     # PLOC_RADIUS
LEAF_MAX = 2                    # MCPT_LEAF_MAX
MAX_ROUNDS = 4096               # gpu_build_ploc gives up after this many


# ------------------------------------------------------------------------------------------------------------------------ the builder
def scene_boxes(scene) -> np.ndarray:
    """(n, 6) fp32 {lo xyz, hi xyz} per face, as build_host_scene hands them to the custom builder: vertices less the fp64 centre of the used
    vertices' bounding box, rounded outward."""
    p = scene.vertex[scene.face[:, :, 0]].astype(np.float64)                       # (n, 3 corners, 3)
    used = p.reshape(-1, 3)
    ctr = 0.5 * used.min(0) + 0.5 * used.max(0)
    x = p - ctr
    lo, hi = x.min(1), x.max(1)
    flo = lo.astype(F32); fhi = hi.astype(F32)
    flo = np.where(flo.astype(np.float64) > lo, np.nextafter(flo, F32(-np.inf)), flo)
    fhi = np.where(fhi.astype(np.float64) < hi, np.nextafter(fhi, F32(np.inf)), fhi)
    return np.concatenate([flo, fhi], 1).astype(F32)


def _expand21(v):
    v = v & np.uint64(0x1fffff)
    for sh, m in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(sh))) & np.uint64(m)
    return v


def morton_codes(boxes) -> np.ndarray:
    """morton_kernel: 21 bits per axis of the box centre inside the bounds of the centres (the host's lo / inv_ext, fp32)."""
    b = np.asarray(boxes, F32)
    c = F32(0.5) * (b[:, :3] + b[:, 3:])
    lo, hi = c.min(0), c.max(0)
    with np.errstate(divide="ignore"):
        inv = np.where(hi > lo, F32(1.0) / (hi - lo), F32(0.0)).astype(F32)
    s = F32(2097152.0)
    q = np.minimum(np.maximum((c - lo) * inv * s, F32(0.0)), s - F32(1.0)).astype(np.uint64)
    return (_expand21(q[:, 0]) << np.uint64(2)) | (_expand21(q[:, 1]) << np.uint64(1)) | _expand21(q[:, 2])


def _nearest(lo, hi, tie):
    """ploc_nn_kernel on clusters (lo, hi): nn[i]."""
    nc = lo.shape[0]
    pad_lo = np.full((nc + 2 * RADIUS, 3), np.nan, F32); pad_hi = pad_lo.copy()
    pad_lo[RADIUS:RADIUS + nc] = lo; pad_hi[RADIUS:RADIUS + nc] = hi
    wl = np.lib.stride_tricks.sliding_window_view(pad_lo, 2 * RADIUS + 1, axis=0)  # (nc, 3, 33)
    wh = np.lib.stride_tricks.sliding_window_view(pad_hi, 2 * RADIUS + 1, axis=0)
    e = np.maximum(hi[:, :, None], wh) - np.minimum(lo[:, :, None], wl)            # fmaxf / fminf; fp32 differences
    x, y, z = e[:, 0], e[:, 1], e[:, 2]
    a = (x * y + y * z) + z * x                                                    # fp32, product by product
    g = np.arange(nc)[:, None] + np.arange(-RADIUS, RADIUS + 1)[None, :]
    a = np.where((g < 0) | (g >= nc) | (g == np.arange(nc)[:, None]) | ~(a < F32(3.4e38)), F32(np.inf), a)
    k = np.argmin(a, 1)                                                            # the first minimum = the lowest index
    rows = np.arange(nc)
    if tie == "pair":
        kp = (rows ^ 1) - rows + RADIUS                                            # column of the partner i ^ 1
        k = np.where(a[rows, kp] == a[rows, k], kp, k)
    else:
        assert tie == "lower"
    best = a[rows, k]
    return np.where(np.isfinite(best), rows + k - RADIUS, rows)


def build(boxes, tie="pair", max_rounds=None):
    """The device builder on (n, 6) fp32 boxes.  A dict: rounds, gave_up (more than MAX_ROUNDS rounds or a round without a merge: what
    gpu_build_ploc reports as such; the figures below are then of the clustering carried to its end when max_rounds allows), n_nodes (inner
    nodes emitted), depth (inner levels), max_leaf."""
    b = np.asarray(boxes, F32); n = b.shape[0]
    assert n > LEAF_MAX
    order = np.argsort(morton_codes(b), kind="stable")
    lo, hi = b[order, :3].copy(), b[order, 3:].copy()
    ref = -1 - np.arange(n, dtype=np.int64)                                        # < 0: a triangle; >= 0: an inner node
    left, right = [], []
    rounds, stuck = 0, False
    limit = 10 * n if max_rounds is None else max_rounds
    while lo.shape[0] > 1 and rounds < limit:
        nc = lo.shape[0]
        nn = _nearest(lo, hi, tie)
        rows = np.arange(nc)
        mutual = (nn != rows) & (nn[nn] == rows)
        low = np.flatnonzero(mutual & (rows < nn)); up = nn[low]
        if low.size == 0:
            stuck = True; break
        base = len(left)
        left.extend(ref[low].tolist()); right.extend(ref[up].tolist())
        lo[low] = np.minimum(lo[low], lo[up]); hi[low] = np.maximum(hi[low], hi[up])
        ref = ref.copy(); ref[low] = base + np.arange(low.size)
        keep = np.ones(nc, bool); keep[up] = False
        lo, hi, ref = lo[keep], hi[keep], ref[keep]
        rounds += 1
    out = {"rounds": rounds, "gave_up": bool(stuck or rounds > MAX_ROUNDS or lo.shape[0] > 1), "n_nodes": None, "depth": None, "max_leaf": None}
    if lo.shape[0] > 1:
        return out
    ni = len(left)
    assert ni == n - 1
    size = [0] * ni
    for k in range(ni):                                                            # children are made before their parents
        size[k] = (1 if left[k] < 0 else size[left[k]]) + (1 if right[k] < 0 else size[right[k]])
    depth = [0] * ni; depth[ni - 1] = 1                                            # the last merge is the root
    n_nodes = 0; deepest = 0; max_leaf = 1
    for k in range(ni - 1, -1, -1):
        if size[k] <= LEAF_MAX:
            max_leaf = max(max_leaf, size[k]); continue
        n_nodes += 1; deepest = max(deepest, depth[k])
        for c in (left[k], right[k]):
            if c >= 0: depth[c] = depth[k] + 1
    out.update(n_nodes=n_nodes, depth=deepest, max_leaf=max_leaf)
    return out


def predict(scene, tie="pair"):
    """`build` on a scene, stopped where the device stops: rounds capped just past MAX_ROUNDS."""
    return build(scene_boxes(scene), tie, max_rounds=MAX_ROUNDS + 1)


# ------------------------------------------------------------------------------------------------------------------------ scenes
def _scene(pkg, name, tri, emissive=0):
    """A SceneData of the (n, 3, 3) triangles `tri`, own vertices each, flat normals; triangle `emissive` is the light (mcpt_create wants one),
    the camera looks at the whole set from outside its bounding box."""
    S = pkg.scenes
    tri = np.asarray(tri, np.float64); n = tri.shape[0]
    v = tri.reshape(-1, 3)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    f = np.zeros((n, 3, 4), np.int32)
    for k in range(3):
        f[:, k, 0] = 3 * np.arange(n) + k; f[:, k, 1] = np.arange(n)
    f[emissive, :, 3] = 1
    mats = [S.Material("grey", kd=(0.6, 0.6, 0.6)), S.Material("lamp", kd=(0.0, 0.0, 0.0), radiance=(5.0, 5.0, 5.0))]
    lo, hi = v.min(0), v.max(0); c = 0.5 * (lo + hi); r = float(np.linalg.norm(hi - lo)) + 1.0
    cam = S.Camera(tuple(c + np.array([0.3, 0.5, 1.0]) * 1.5 * r), tuple(c), (0.0, 1.0, 0.0), 40.0, 16, 16)
    return S.SceneData(name, v, nrm, np.zeros((1, 2)), f, mats, cam, {})


def coincident(pkg, n):
    """n copies of one triangle."""
    return _scene(pkg, "coincident-%d" % n, np.tile(np.array([[[0.0, 0.0, 0.0], [2.0, 0.0, 1.0], [0.0, 2.0, 1.0]]]), (n, 1, 1)))


def _quads(ix, iy):
    """Two triangles per unit quad [ix, ix + 1] x [iy, iy + 1] of the plane z = 0, quad by quad."""
    ix = np.asarray(ix, np.float64).ravel(); iy = np.asarray(iy, np.float64).ravel(); z = np.zeros_like(ix)
    p00 = np.stack([ix, iy, z], -1); p10 = np.stack([ix + 1, iy, z], -1); p11 = np.stack([ix + 1, iy + 1, z], -1); p01 = np.stack([ix, iy + 1, z], -1)
    return np.stack([np.stack([p00, p10, p11], 1), np.stack([p00, p11, p01], 1)], 1).reshape(-1, 3, 3)


def strip(pkg, n_quads):
    """n_quads unit quads in a row (2 n_quads triangles) on the integer lattice: every box, extent and area exact in fp32."""
    return _scene(pkg, "strip-%d" % n_quads, _quads(np.arange(n_quads), np.zeros(n_quads)))


def grid(pkg, k):
    """k x k unit quads, row by row."""
    iy, ix = np.mgrid[0:k, 0:k]
    return _scene(pkg, "grid-%d" % k, _quads(ix, iy))


def lattice_soup(pkg, n, seed=1):
    """n triangles with integer vertices in [0, 255]^3 and bounding boxes of 1 .. 4 units a side: merged areas are integers below 2^24."""
    rng = np.random.default_rng(seed)
    e = rng.integers(1, 5, (n, 3)).astype(np.float64)
    p = np.floor(rng.uniform(0, 1, (n, 3)) * (256 - e))                             # box [p, p + e] inside [0, 255]
    third = np.stack([e[:, 0], np.zeros(n), rng.integers(0, 5, n) % (e[:, 2] + 1)], -1)   # never on the diagonal p .. p + e: no degenerate triangle
    tri = np.stack([p, p + e, p + third], 1)
    assert tri.min() >= 0 and tri.max() <= 255
    return _scene(pkg, "soup-%d" % n, tri)


def shells(pkg, n, ratio, smallest=None):
    """n copies of one tilted triangle, lifted along its normal by 0.05 x its size (so the copies share no plane) and scaled by
    smallest * ratio^k about the centre of its bounding box.  The box of a shell and any smaller one is the shell's own, so every merge order is
    a chain: depth n - 2 under any tie rule.  All boxes share their centre -- it is the scene's centre too, so a small shell's fp32 coordinates
    are as precise as a large one's -- and with it their Morton code: the sorted order is the order of sizes.  The largest shell is the light.
    The sizes start at 0.1, or lower where the largest would pass 1e12: the fp32 triangle test multiplies three lengths, which overflows from about
    7e12 on.  (At the other end its |det| >= 1e-5 rule never accepts a triangle below about 4e-3: the smallest shells of such a set are in the tree
    but cannot be hit, in fp64 either.)"""
    if smallest is None:
        smallest = min(0.1, 1e12 / ratio ** (n - 1))
    base = np.array([[1.0, 0.1, 0.0], [0.0, 1.0, 0.2], [0.1, 0.0, 1.0]])               # cuts the corners of its box: the box centre is well off its plane
    nrm = np.cross(base[1] - base[0], base[2] - base[0]); nrm /= np.linalg.norm(nrm)
    t0 = base + 0.05 * nrm
    t0 = t0 - 0.5 * (t0.min(0) + t0.max(0))
    assert abs(float(nrm @ t0[0])) > 0.2                                           # the centre of scaling is well off the plane
    s = smallest * ratio ** np.arange(n, dtype=np.float64)
    return _scene(pkg, "shells-%d" % n, s[:, None, None] * t0[None], emissive=n - 1)


# ------------------------------------------------------------------------------------------------------------------------ rays
def interior_rays(scene, n, seed, miss_share=0.2, reach=(0.5, 3.0)):
    """n rays for hit comparisons, and their fp64 brute-force answer: (origins, unit directions, t, face).  Candidates: (1 - miss_share) aimed at
    points inside random triangles from reach[0] .. reach[1] triangle sizes away on either side, the rest from the same kind of origin in a random
    direction.  Kept, by the fp64 brute force alone: the rays that miss everything, and the rays whose closest hit has barycentrics >= 0.05 from
    every edge, meets its triangle at |cos| >= 0.2 and lies at least 0.05 of that triangle's size away -- off edges, grazing angles and origins all but
    on a (large) triangle's plane, where fp32 coordinates cannot give t to the relative tolerance the GPU suite asks."""
    from tests import kit
    rng = np.random.default_rng(seed)
    p = scene.vertex[scene.face[:, :, 0]].astype(np.float64)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tri_size = np.linalg.norm(p.max(1) - p.min(1), axis=1)
    O, D, T_, F_ = [], [], [], []
    have = 0
    for _ in range(80):                                                               # candidates by the quarter set, as many as it takes
        m = max(1, n // 4)
        k = rng.integers(0, p.shape[0], m)
        w = rng.dirichlet((1.0, 1.0, 1.0), m) * 0.85 + 0.05                          # each >= 0.05, sum 1
        tgt = np.einsum("nk,nkd->nd", w, p[k])
        d = rng.normal(size=(m, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        o = tgt - d * tri_size[k][:, None] * rng.uniform(reach[0], reach[1], (m, 1))
        miss = rng.uniform(size=m) < miss_share
        r = rng.normal(size=(m, 3)); r /= np.linalg.norm(r, axis=1, keepdims=True)
        d[miss] = r[miss]
        t, f, u, v = kit.brute_force_trace(scene, o, d, np.float64)
        cos = np.abs(np.einsum("nd,nd->n", nrm[np.maximum(f, 0)], d))
        keep = (f < 0) | ((np.minimum(np.minimum(u, v), 1.0 - u - v) >= 0.05) & (cos >= 0.2) & (t >= 0.05 * tri_size[np.maximum(f, 0)]))
        O.append(o[keep]); D.append(d[keep]); T_.append(t[keep]); F_.append(f[keep]); have += int(keep.sum())
        if have >= n: break
    assert have >= n, (have, n)
    return tuple(np.concatenate(x)[:n] for x in (O, D, T_, F_))


def awkward(pkg, n=3000, seed=11):
    """The scene of test_device_builder_on_awkward_geometry: scenes.open_box plus n triangles with huge coordinate offsets, tiny and huge ones side
    by side, flat boxes and 400 copies of one triangle.  (scene, centres of the n triangles, the generator, for the test's rays)."""
    rng = np.random.RandomState(seed)
    base = pkg.scenes.open_box(8, 8)
    centres = rng.uniform(-1, 1, (n, 3)) * np.array([1e3, 1.0, 1e-3]) + np.array([5e4, -3.0, 0.25])
    size = 10.0 ** rng.uniform(-5, 1, (n, 1, 1))
    tri = centres[:, None, :] + size * rng.normal(size=(n, 3, 3))
    tri[::7, :, 1] = tri[::7, :1, 1]
    tri[1000:1400] = tri[1000]                                                    # 400 copies of one triangle
    v = np.concatenate([base.vertex, tri.reshape(-1, 3)])
    nrm = np.concatenate([base.normal, np.tile([[0.0, 1.0, 0.0]], (3 * n, 1))])
    tc = np.concatenate([base.texcoord, np.zeros((3 * n, 2))])
    off = base.vertex.shape[0]
    f = np.zeros((n, 3, 4), np.int32)
    for k in range(3):
        f[:, k, 0] = f[:, k, 1] = f[:, k, 2] = off + 3 * np.arange(n) + k
    scene = pkg.scenes.SceneData("stress", v, nrm, tc, np.concatenate([base.face, f]), base.materials, base.camera)
    return scene, centres, rng


# ------------------------------------------------------------------------------------------------------------------------ shared cases
# the scenes whose hits the GPU suite compares between a device-built and a host-built context and against the fp64 brute force
HIT_SCENES = {
    "coincident-5000": lambda pkg: coincident(pkg, 5000),
    "strip-9000": lambda pkg: strip(pkg, 9000),
    "grid-64": lambda pkg: grid(pkg, 64),
    "soup-4099": lambda pkg: lattice_soup(pkg, 4099),
    "shells-40": lambda pkg: shells(pkg, 40, 1.5),
    "shells-150": lambda pkg: shells(pkg, 150, 1.2),
    "shells-300": lambda pkg: shells(pkg, 300, 1.15),
    "shells-5000": lambda pkg: shells(pkg, 5000, 1.005),
}
N_RAYS = 2000
N_RAYS_OF = {"shells-5000": 600}          # (where a ray in eight passes interior_rays' selection and every candidate costs 5000 triangle tests)
_cases = {}


def hit_case(pkg, name):
    """(scene, origins, directions, fp64 brute-force t, fp64 brute-force face) of HIT_SCENES[name]: N_RAYS
    rays (N_RAYS_OF[name] where given) of interior_rays, computed once per session and never changed."""
    if name not in _cases:
        scene = HIT_SCENES[name](pkg)
        o, d, t, f = interior_rays(scene, N_RAYS_OF.get(name, N_RAYS), seed=len(name) + scene.face.shape[0], reach=(5.0, 20.0) if name.startswith("soup") else (0.5, 3.0))
        for a in (o, d, t, f):
            a.setflags(write=False)
        _cases[name] = (scene, o, d, t, f)
    return _cases[name]
