"""ctypes mirror of include/mcpt.h's auto-normals section: mcpt_normals_opts and mcpt_normals_info, and the mask of the normal
records that a set of faces uses.  Re-exported by the package; tests/test_normals.py holds the structs' sizes and offsets to the header."""
import ctypes as C

import numpy as np

NORMALS_OFF = 0
NORMALS_AREA = 1


class NormalsOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class NormalsInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_uint32), ("records", C.c_uint32), ("max_valence", C.c_uint32), ("entries", C.c_uint64),
                ("updates", C.c_uint32), ("reserved0", C.c_uint32), ("last_ms", C.c_double), ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


def normal_mask_from_faces(scene, face_mask):
    """uint8 (n_normal): 1 for every normal record that a face chosen by `face_mask` (bool per face) names in any corner."""
    face_mask = np.asarray(face_mask, bool).reshape(-1)
    if face_mask.shape[0] != scene.face.shape[0]:
        raise ValueError("face_mask has %d entries for %d faces" % (face_mask.shape[0], scene.face.shape[0]))
    mask = np.zeros(scene.normal.shape[0], np.uint8)
    mask[np.unique(scene.face[face_mask][:, :, 1])] = 1
    return mask
