"""ctypes mirror of include/mcpt.h's keyframe section: mcpt_keyframe_opts and mcpt_keyframe_info, and the interpolation and
wrap constants.  Re-exported by the package; tests/test_keyframes.py holds the structs' sizes and offsets to the header."""
import ctypes as C

KEYFRAMES_LINEAR = 0
KEYFRAMES_CATMULL_ROM = 1
KEYFRAMES_CLAMP = 0
KEYFRAMES_LOOP = 1
KEYFRAMES_MAX = 65536


class KeyframeOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("interpolation", C.c_uint32), ("wrap", C.c_uint32), ("reserved0", C.c_uint32),
                ("start_time", C.c_double), ("frame_time", C.c_double), ("reserved", C.c_uint32 * 4)]


class KeyframeInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_frames", C.c_uint32), ("interpolation", C.c_uint32), ("wrap", C.c_uint32),
                ("updates", C.c_uint32), ("last_frame", C.c_uint32), ("last_u", C.c_double), ("last_time", C.c_double), ("last_ms", C.c_double),
                ("device_bytes", C.c_uint64), ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}
