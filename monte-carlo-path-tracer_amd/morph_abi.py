"""ctypes mirror of include/mcpt.h's morph-target section: mcpt_morph_targets and mcpt_morph_info, and the flattening of a list
of targets into the arrays mcpt_morph_targets points to.  Re-exported by the package; tests/test_morph.py holds the structs' sizes and offsets
to the header."""
import ctypes as C

import numpy as np

MORPH_MAX_TARGETS = 65536


class MorphTargets(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_targets", C.c_uint32), ("target_offset", C.POINTER(C.c_uint32)), ("index", C.POINTER(C.c_uint32)),
                ("delta", C.POINTER(C.c_double)), ("reserved", C.c_uint32 * 4)]


class MorphInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_targets", C.c_uint32), ("updates", C.c_uint32), ("reserved0", C.c_uint32),
                ("vertex_entries", C.c_uint64), ("normal_entries", C.c_uint64), ("last_ms", C.c_double), ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


def flatten_targets(targets):
    """A list of (index array, (n, 3) delta array) pairs, one per target, as (target_offset uint32 (n_targets + 1), index uint32 (total),
    delta float64 (total, 3)).  The entries are taken as they come -- nothing is sorted, merged or checked beyond the shapes: the library's
    rules (strictly ascending indices inside a target, finite deltas) are the library's to refuse.  Raises ValueError when a pair's lengths
    differ or an index does not fit 32 bits."""
    offset = np.zeros(len(targets) + 1, np.uint32)
    idx, dlt = [], []
    for k, (i, d) in enumerate(targets):
        i = np.asarray(i).reshape(-1)
        d = np.ascontiguousarray(d, np.float64).reshape(-1, 3)
        if i.shape[0] != d.shape[0]:
            raise ValueError("target %d: %d indices and %d deltas" % (k, i.shape[0], d.shape[0]))
        if i.size and (np.asarray(i, np.int64).min() < 0 or np.asarray(i, np.int64).max() >= 2 ** 32):
            raise ValueError("target %d: an index does not fit 32 bits" % k)
        idx.append(i.astype(np.uint32)); dlt.append(d)
        offset[k + 1] = offset[k] + i.shape[0]
    index = np.concatenate(idx) if idx else np.zeros(0, np.uint32)
    delta = np.concatenate(dlt) if dlt else np.zeros((0, 3), np.float64)
    return offset, np.ascontiguousarray(index, np.uint32), np.ascontiguousarray(delta, np.float64)


def targets_struct(targets):
    """(MorphTargets, the arrays it points to -- keep them alive as long as the struct is used)."""
    offset, index, delta = flatten_targets(targets)
    t = MorphTargets()
    t.struct_size = C.sizeof(MorphTargets); t.n_targets = len(targets)
    t.target_offset = offset.ctypes.data_as(C.POINTER(C.c_uint32))
    t.index = index.ctypes.data_as(C.POINTER(C.c_uint32)) if index.size else None
    t.delta = delta.ctypes.data_as(C.POINTER(C.c_double)) if delta.size else None
    return t, (offset, index, delta)
