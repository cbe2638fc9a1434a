"""ctypes mirror of include/mcpt.h's parts-update section: mcpt_scene_update and mcpt_parts_info, the owner ids, route bits and the
flag, and the owners a set of faces gives its records.  Re-exported by the package; tests/test_parts.py holds the structs' sizes and offsets to
the header."""
import ctypes as C

import numpy as np

OWNER_NONE = 0
OWNER_GROUPS = 1
OWNER_SKIN = 2
OWNER_MORPH = 3
OWNER_KEYFRAMES = 4
ROUTE_GROUPS = 1 << OWNER_GROUPS
ROUTE_SKIN = 1 << OWNER_SKIN
ROUTE_MORPH = 1 << OWNER_MORPH
ROUTE_KEYFRAMES = 1 << OWNER_KEYFRAMES
PARTS_MORPH_THEN_SKIN = 0x1


class SceneUpdate(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("routes", C.c_uint32), ("flags", C.c_uint32), ("reserved0", C.c_uint32),
                ("group_m3x4", C.c_void_p), ("n_groups", C.c_uint32), ("reserved1", C.c_uint32),
                ("bone_m3x4", C.c_void_p), ("n_bones", C.c_uint32), ("reserved2", C.c_uint32),
                ("morph_weight", C.c_void_p), ("n_targets", C.c_uint32), ("reserved3", C.c_uint32),
                ("time", C.c_double), ("reserved", C.c_uint32 * 4)]


class PartsInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("set", C.c_uint32), ("updates", C.c_uint32), ("last_routes", C.c_uint32),
                ("vertex_records", C.c_uint32 * 5), ("normal_records", C.c_uint32 * 5), ("last_ms", C.c_double), ("device_bytes", C.c_uint64),
                ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        out = {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}
        out["vertex_records"] = list(self.vertex_records); out["normal_records"] = list(self.normal_records)
        return out


def owners_from_faces(scene, face_owner):
    """Per-vertex and per-normal owner ids (two uint8 arrays, for Renderer.set_vertex_owners) from one owner id per face, the twin of
    groups_from_faces: a vertex or normal takes the owner of the faces that use it, one no face uses is OWNER_NONE.  Raises ValueError naming the
    record when faces of two owners share a vertex or a normal -- the caller duplicates it then."""
    fo = np.ascontiguousarray(face_owner, np.int64).reshape(-1)
    if fo.shape[0] != scene.face.shape[0] or (fo.size and (fo.min() < OWNER_NONE or fo.max() > OWNER_KEYFRAMES)):
        raise ValueError("owners_from_faces: need one owner id in [0, 4] per face")
    out = []
    for what, col, n in (("vertex", 0, scene.vertex.shape[0]), ("normal", 1, scene.normal.shape[0])):
        idx = scene.face[:, :, col].astype(np.int64).reshape(-1); o = np.repeat(fo, 3)
        lo = np.full(n, np.iinfo(np.int64).max, np.int64); hi = np.full(n, -1, np.int64)
        np.minimum.at(lo, idx, o); np.maximum.at(hi, idx, o)
        shared = np.flatnonzero((hi >= 0) & (lo != hi))
        if shared.size:
            raise ValueError("owners_from_faces: %s %d is used by faces of owners %d and %d" % (what, shared[0], lo[shared[0]], hi[shared[0]]))
        out.append(np.where(hi >= 0, hi, OWNER_NONE).astype(np.uint8))
    return out[0], out[1]
