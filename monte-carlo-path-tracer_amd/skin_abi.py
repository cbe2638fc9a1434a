"""ctypes mirror of include/mcpt.h's skinning sections: mcpt_skin_info, MCPT_SKIN_INFLUENCES and the skinning modes.
Re-exported by the package; tests/test_skin.py holds the struct's size and offsets to the header, tests/test_skin_dq.py the modes' values."""
import ctypes as C

SKIN_INFLUENCES = 4
SKIN_LINEAR, SKIN_DUAL_QUATERNION = 0, 1                 # mcpt_set_skin_mode


class SkinInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_bones", C.c_uint32), ("updates", C.c_uint32), ("reserved0", C.c_uint32), ("last_ms", C.c_double),
                ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}
