"""ctypes mirror of include/mcpt.h's face-visibility section: mcpt_visibility_info, and the mask that hides the faces of a set of
materials.  Re-exported by the package; tests/test_visibility.py holds the struct's size and offsets to the header."""
import ctypes as C

import numpy as np


class VisibilityInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("set", C.c_uint32), ("n_hidden", C.c_uint32), ("n_hidden_emitters", C.c_uint32),
                ("updates", C.c_uint32), ("reserved0", C.c_uint32), ("last_ms", C.c_double), ("device_bytes", C.c_uint64),
                ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


def visibility_from_materials(scene, hidden_materials):
    """One byte per face (a uint8 array, for Renderer.set_face_visibility): 0 for the faces whose material -- corner 0's -- is one of
    `hidden_materials` (indices into scene.materials), 1 for the rest.  Raises ValueError for an index the scene does not have."""
    hidden = np.unique(np.ascontiguousarray(list(hidden_materials), np.int64).reshape(-1))
    if hidden.size and (hidden.min() < 0 or hidden.max() >= len(scene.materials)):
        raise ValueError("visibility_from_materials: material index out of range")
    return (~np.isin(scene.face[:, 0, 3], hidden)).astype(np.uint8)
