"""ctypes mirrors of include/mcpt.h's tree-rebuild section: mcpt_rebuild_opts, mcpt_rebuild_info and the MCPT_REBUILD_* builder
constants.  Re-exported by the package; tests/test_rebuild.py holds their sizes and offsets to the header."""
import ctypes as C

REBUILD_SAME, REBUILD_HOST, REBUILD_DEVICE = 0, 1, 2


class RebuildOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("builder", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class RebuildInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("rebuilds", C.c_uint32), ("last_ms", C.c_double), ("last_build_ms", C.c_double),
                ("last_device_ms", C.c_double), ("area_ratio_before", C.c_double), ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
