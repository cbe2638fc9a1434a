"""ctypes mirror of include/mcpt.h's light-probe section: mcpt_sh_info, the constants, Renderer's probe methods and the two
host-only helpers -- sh_grid (mcpt_sh_grid: the cell centres of a box) and sh_eval (mcpt_sh_eval: a probe's coefficients for a normal).
Re-exported by the package, whose Renderer mixes ShProbeMethods in; tests/test_shprobe_ref.py holds the struct's size and offsets to the header."""
import ctypes as C

import numpy as np

SH_RADIANCE = 0
SH_IRRADIANCE = 1
SH_DIRECTIONS = 64
SH_MAX_PROBES = 1048575
SH_COEFFS = 27                                               # 9 coefficients x 3 channels, channel-major


class ShInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_probes", C.c_uint32), ("bakes", C.c_uint32), ("reserved0", C.c_uint32), ("passes", C.c_uint64),
                ("last_stage_ms", C.c_double), ("device_bytes", C.c_uint64), ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


def _raise(lib, st):
    from . import McptError
    raise McptError("mcpt status %d: %s" % (st, (lib.mcpt_last_error() or b"").decode()))


def sh_grid(lo, hi, nx: int, ny: int, nz: int) -> np.ndarray:
    """(nx ny nz, 3) float64: the centres of the cells of the box [lo, hi], x fastest (mcpt_sh_grid; no device is touched)."""
    from . import MCPT_OK, load_library
    lib = load_library()
    lo = np.ascontiguousarray(lo, np.float64).reshape(3); hi = np.ascontiguousarray(hi, np.float64).reshape(3)
    n = C.c_uint32(0)
    lib.mcpt_sh_grid(lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), int(nx), int(ny), int(nz), 0, None, C.byref(n))       # the count: the capacity protocol
    out = np.zeros((max(1, n.value), 3), np.float64)
    st = lib.mcpt_sh_grid(lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), int(nx), int(ny), int(nz), out.shape[0], out.ctypes.data_as(C.c_void_p), C.byref(n))
    if st != MCPT_OK:
        _raise(lib, st)
    return out[:n.value].copy()


def sh_eval(coeffs, normal) -> np.ndarray:
    """(n, 3) float64: sum_k coeffs[c, k] Y_k(normal / |normal|) per channel for coefficients (n, 27) or (n, 3, 9) float32 and normals (n, 3) (one
    normal broadcasts); 0 for a zero normal.  With read_sh(SH_IRRADIANCE)'s coefficients this is the irradiance for that normal."""
    from . import MCPT_OK, load_library
    lib = load_library()
    c = np.ascontiguousarray(coeffs, np.float32).reshape(-1, SH_COEFFS)
    nrm = np.ascontiguousarray(np.broadcast_to(np.asarray(normal, np.float64).reshape(-1, 3), (c.shape[0], 3)))
    out = np.zeros((c.shape[0], 3), np.float64)
    for i in range(c.shape[0]):
        st = lib.mcpt_sh_eval(c[i].ctypes.data_as(C.c_void_p), nrm[i].ctypes.data_as(C.c_void_p), out[i].ctypes.data_as(C.c_void_p))
        if st != MCPT_OK:
            _raise(lib, st)
    return out


class ShProbeMethods:
    """Renderer's light-probe methods."""

    def set_sh_probes(self, positions):
        """The probes bake_sh starts rays from: (n, 3) WORLD positions (None or an empty array drops them).  Zeroes the accumulators.  Synchronous."""
        p = np.zeros((0, 3), np.float64) if positions is None else np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
        self._check(self.lib.mcpt_set_sh_probes(self.ctx, p.ctypes.data_as(C.c_void_p) if p.size else None, p.shape[0]))
        self._n_sh = int(p.shape[0])

    def bake_sh(self, passes: int, seed: int = 0, first_sample: int = 0):
        """`passes` passes of 64 rays per probe added to every probe's accumulators: per pass the ray kernel, the first-hit kernel, the wavefront
        pipeline and the projection kernel.  Asynchronous."""
        self._check(self.lib.mcpt_bake_sh(self.ctx, passes, seed, first_sample))

    def clear_sh(self):
        self._check(self.lib.mcpt_clear_sh(self.ctx))

    def read_sh(self, mode: int = SH_RADIANCE) -> np.ndarray:
        """(n, 3, 9) float32: per probe and channel the coefficients k = l (l + 1) + m of the incident radiance (SH_RADIANCE) or of the
        irradiance as a function of the normal (SH_IRRADIANCE: sh_eval's input)."""
        out = np.zeros((getattr(self, "_n_sh", 0), 3, 9), np.float32)
        self._check(self.lib.mcpt_read_sh(self.ctx, int(mode), out.ctypes.data_as(C.c_void_p)))
        return out

    def read_sh_film(self):
        """((n, 3, 9) float32 raw accumulators, (n, 3) uint32 {rays, hits from behind, misses})."""
        n = getattr(self, "_n_sh", 0)
        acc = np.zeros((n, 3, 9), np.float32); counts = np.zeros((n, 3), np.uint32)
        self._check(self.lib.mcpt_read_sh_film(self.ctx, acc.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)))
        return acc, counts

    def sh_info(self) -> ShInfo:
        i = ShInfo()
        self._check(self.lib.mcpt_get_sh_info(self.ctx, C.byref(i)))
        return i

    def probe_sh_rays(self, sample: int = 0, seed: int = 0, first_item: int = 0, n_items=None):
        """The stage's rays for items first_item .. first_item + n_items - 1 (n_items None: to the end; item i = probe i >> 6, slot i & 63) of sample
        `sample`: ((n, 3) float64 origins in DEVICE coordinates, (n, 3) float64 directions holding fp32 values)."""
        n = SH_DIRECTIONS * getattr(self, "_n_sh", 0) - int(first_item) if n_items is None else int(n_items)
        o = np.zeros((max(n, 0), 3), np.float64); d = np.zeros_like(o)
        self._check(self.lib.mcpt_probe_sh_rays(self.ctx, sample, seed, int(first_item), max(n, 0) if n >= 0 else 0xffffffff, o.ctypes.data_as(C.c_void_p),
                                                d.ctypes.data_as(C.c_void_p)))
        return o, d

    def read_sh_pass(self):
        """The last pass as it was left: ((64 n, 4) float32 scratch film {L, 1}, (64 n,) uint8 class: 0 miss, 1 front, 2 back).  Synchronises."""
        n = SH_DIRECTIONS * getattr(self, "_n_sh", 0)
        film = np.zeros((n, 4), np.float32); cls = np.zeros(n, np.uint8)
        self._check(self.lib.mcpt_read_sh_pass(self.ctx, film.ctypes.data_as(C.c_void_p), cls.ctypes.data_as(C.c_void_p)))
        return film, cls
