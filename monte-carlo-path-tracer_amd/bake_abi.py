"""ctypes mirror of include/mcpt.h's surface-baking section: mcpt_bake_point, mcpt_bake_info, the constants, and the two makers
of bake-point lists -- lightmap_points (mcpt_lightmap_points: host only, no device) and vertex_bake_points.  Re-exported by the package, whose
Renderer mixes BakeMethods in; tests/test_bake_ref.py holds the structs' sizes and offsets to the header (BakeInfo keeps the header's
`reserved` array whole and reads `direct_mode`, the name the header gives its first word, through a property: tests/test_bake_direct_ref.py)."""
import ctypes as C

import numpy as np

BAKE_BACK_SIDE = 1
BAKE_IRRADIANCE = 0
BAKE_DIFFUSE = 1
BAKE_MAX_POINTS = 0x3ffffff
BAKE_DIRECT_OFF = 0
BAKE_DIRECT_MIS = 1
# probe_bake_direct's state column
BAKE_DIRECT_STATE_DEAD, BAKE_DIRECT_STATE_NO_PDF, BAKE_DIRECT_STATE_BELOW, BAKE_DIRECT_STATE_OCCLUDED, BAKE_DIRECT_STATE_COUNTED = range(5)

# numpy's view of a list of mcpt_bake_point
POINT_DTYPE = np.dtype([("face", np.uint32), ("u", np.float32), ("v", np.float32), ("flags", np.uint32)])


class BakePoint(C.Structure):
    _fields_ = [("face", C.c_uint32), ("u", C.c_float), ("v", C.c_float), ("flags", C.c_uint32)]


class BakeInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_points", C.c_uint32), ("n_dead", C.c_uint32), ("bakes", C.c_uint32), ("passes", C.c_uint64),
                ("last_stage_ms", C.c_double), ("device_bytes", C.c_uint64), ("reserved", C.c_uint32 * 4)]

    @property
    def direct_mode(self) -> int:
        """BAKE_DIRECT_*: the header's name for reserved[0]'s word."""
        return int(self.reserved[0])

    def as_dict(self):
        return dict({k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}, direct_mode=self.direct_mode)


def bake_points(face, u, v, flags=0) -> np.ndarray:
    """A POINT_DTYPE array from per-point faces, barycentrics and flags (scalars broadcast)."""
    face = np.asarray(face).reshape(-1)
    p = np.zeros(face.shape[0], POINT_DTYPE)
    p["face"] = face; p["u"] = np.asarray(u, np.float32); p["v"] = np.asarray(v, np.float32); p["flags"] = np.asarray(flags, np.uint32)
    return p


def _as_points(points) -> np.ndarray:
    p = np.ascontiguousarray(points)
    if p.dtype != POINT_DTYPE:
        raise ValueError("bake points: need an array of bake_abi.POINT_DTYPE (bake_points() makes one)")
    return p.reshape(-1)


def lightmap_points(scene, width: int, height: int):
    """The texel-to-surface map of a width x height lightmap over `scene`'s texcoords (mcpt_lightmap_points; no device is touched):
    (POINT_DTYPE array, (n,) uint32 texel = j * width + i), in texel order; texels that no face covers are absent."""
    from . import DescHolder, MCPT_OK, McptError, load_library
    lib = load_library()
    holder = DescHolder(scene)
    n = C.c_uint32(0)
    lib.mcpt_lightmap_points(C.byref(holder.desc), int(width), int(height), 0, None, None, C.byref(n))      # the count: the capacity protocol
    pts = np.zeros(max(1, n.value), POINT_DTYPE); tex = np.zeros(max(1, n.value), np.uint32)
    st = lib.mcpt_lightmap_points(C.byref(holder.desc), int(width), int(height), pts.shape[0], pts.ctypes.data_as(C.c_void_p), tex.ctypes.data_as(C.c_void_p), C.byref(n))
    if st != MCPT_OK:
        raise McptError("mcpt status %d: %s" % (st, (lib.mcpt_last_error() or b"").decode()))
    return pts[:n.value].copy(), tex[:n.value].copy()


def vertex_bake_points(scene):
    """One point per face corner, for per-vertex baking: (POINT_DTYPE array of 3 n_face points -- corner k of face f is point 3 f + k --,
    (3 n_face,) int64 vertex index of each).  A vertex's value is the average of its points' (np.add.at over the second array)."""
    nf = scene.face.shape[0]
    p = np.zeros(3 * nf, POINT_DTYPE)
    p["face"] = np.repeat(np.arange(nf, dtype=np.uint32), 3)
    p["u"] = np.tile(np.array([0.0, 1.0, 0.0], np.float32), nf); p["v"] = np.tile(np.array([0.0, 0.0, 1.0], np.float32), nf)
    return p, scene.face[:, :, 0].astype(np.int64).reshape(-1)


class BakeMethods:
    """Renderer's surface-baking methods."""

    def set_bake_points(self, points):
        """The points mcpt_bake starts rays from (a POINT_DTYPE array; None or an empty one drops them).  Zeroes the bake film.  Synchronous."""
        p = np.zeros(0, POINT_DTYPE) if points is None else _as_points(points)
        self._check(self.lib.mcpt_set_bake_points(self.ctx, p.ctypes.data_as(C.c_void_p) if p.size else None, p.shape[0]))
        self._n_bake = int(p.shape[0])

    def bake(self, spp: int, seed: int = 0, first_sample: int = 0):
        """`spp` samples added to every point's bake-film record: per sample the ray kernel, then the wavefront pipeline.  Asynchronous."""
        self._check(self.lib.mcpt_bake(self.ctx, spp, seed, first_sample))

    def clear_bake(self):
        self._check(self.lib.mcpt_clear_bake(self.ctx))

    def read_bake(self, mode: int = BAKE_IRRADIANCE) -> np.ndarray:
        """(n, 4) float32: {irradiance (BAKE_IRRADIANCE) or outgoing diffuse radiance (BAKE_DIFFUSE), samples} per point."""
        out = np.zeros((getattr(self, "_n_bake", 0), 4), np.float32)
        self._check(self.lib.mcpt_read_bake(self.ctx, int(mode), out.ctypes.data_as(C.c_void_p)))
        return out

    def read_bake_film(self) -> np.ndarray:
        """(n, 4) float32: the raw {sum L, count} per point."""
        out = np.zeros((getattr(self, "_n_bake", 0), 4), np.float32)
        self._check(self.lib.mcpt_read_bake_film(self.ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    def bake_info(self) -> BakeInfo:
        i = BakeInfo()
        self._check(self.lib.mcpt_get_bake_info(self.ctx, C.byref(i)))
        return i

    def set_bake_direct(self, mode: int):
        """BAKE_DIRECT_OFF (the default) or BAKE_DIRECT_MIS: next-event estimation at the bake point, MIS-weighted against the cosine ray.  Holds
        for the passes enqueued after it; survives set_bake_points, clear_bake and rebuild."""
        self._check(self.lib.mcpt_set_bake_direct(self.ctx, int(mode)))

    def probe_bake_direct(self, sample: int = 0, seed: int = 0, first: int = 0, n=None):
        """The direct-light kernel's two terms for points first .. first + n - 1 (n None: to the end of the list) of sample `sample`, whatever the
        mode: ((n, 12) float32 sub[3], add[3], w_b, w_l, p_b, p_l, p_bl, p_lf; (n, 4) int32 first-hit face or -1, front, light face, state)."""
        n = getattr(self, "_n_bake", 0) - int(first) if n is None else int(n)
        f = np.zeros((max(n, 0), 12), np.float32); k = np.zeros((max(n, 0), 4), np.int32)
        self._check(self.lib.mcpt_probe_bake_direct(self.ctx, sample, seed, int(first), max(n, 0) if n >= 0 else 0xffffffff, f.ctypes.data_as(C.c_void_p),
                                                    k.ctypes.data_as(C.c_void_p)))
        return f, k

    def probe_bake_rays(self, sample: int = 0, seed: int = 0, first: int = 0, n=None):
        """The stage's rays for points first .. first + n - 1 (n None: to the end of the list) of sample `sample`: ((n, 3) float64 origins in
        DEVICE coordinates, (n, 3) float64 directions holding fp32 values, (n, 3) float64 unit normals, (n,) uint8 dead)."""
        n = getattr(self, "_n_bake", 0) - int(first) if n is None else int(n)
        o = np.zeros((max(n, 0), 3), np.float64); d = np.zeros_like(o); nn = np.zeros_like(o); dead = np.zeros(max(n, 0), np.uint8)
        self._check(self.lib.mcpt_probe_bake_rays(self.ctx, sample, seed, int(first), max(n, 0) if n >= 0 else 0xffffffff, o.ctypes.data_as(C.c_void_p),
                                                  d.ctypes.data_as(C.c_void_p), nn.ctypes.data_as(C.c_void_p), dead.ctypes.data_as(C.c_void_p)))
        return o, d, nn, dead
