"""numpy restatement of automatic normals: the host's per-record face lists (nr_per_record of csrc/normals.hip) and the pass
(nr_normals_kernel).  Every step is one correctly rounded fp64 operation in the kernel's association and order, so the arrays are the
device's bit for bit.  numpy never fuses a product into a sum: each ufunc call below rounds once."""
from __future__ import annotations

import numpy as np


def _cross(v0, v1, v2):
    """cross(v1 - v0, v2 - v0) per row, the kernel's expressions."""
    a = v1 - v0; b = v2 - v0
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)


def per_record(face, n_normal, vertex, normal, mask=None):
    """(offset uint32 (n_normal + 1), entry uint32 (total, 4): v0, v1, v2, flip).  face: (n_face, 3, >= 2) with [..., 0] the vertex and
    [..., 1] the normal index of a corner.  A record gets one entry per face that names it in any corner, by ascending face index; a record
    that `mask` (n_normal, != 0 = recompute; None = all) leaves out gets none.  flip = ((g.x n.x + g.y n.y) + g.z n.z) < 0 at the reference
    pose `vertex` / `normal`."""
    face = np.asarray(face); fv = face[:, :, 0].astype(np.int64); fn = face[:, :, 1].astype(np.int64)
    nf = fv.shape[0]
    f_id = np.repeat(np.arange(nf), 3); rec = fn.reshape(-1)
    key = np.unique(rec * max(nf, 1) + f_id)                                 # sorted by record, then face; one per (record, face)
    pair = np.stack([key // max(nf, 1), key % max(nf, 1)], -1)
    if mask is not None:
        pair = pair[np.asarray(mask).reshape(-1)[pair[:, 0]] != 0]
    offset = np.zeros(n_normal + 1, np.uint32)
    offset[1:] = np.cumsum(np.bincount(pair[:, 0], minlength=n_normal))
    f = pair[:, 1]
    vertex = np.asarray(vertex, np.float64); normal = np.asarray(normal, np.float64)
    g = _cross(vertex[fv[f, 0]], vertex[fv[f, 1]], vertex[fv[f, 2]])
    n = normal[pair[:, 0]]
    with np.errstate(invalid="ignore", over="ignore"):
        dot = (g[:, 0] * n[:, 0] + g[:, 1] * n[:, 1]) + g[:, 2] * n[:, 2]
    entry = np.concatenate([fv[f], (dot < 0)[:, None].astype(np.int64)], 1).astype(np.uint32).reshape(-1, 4)
    return offset, entry


def apply(offset, entry, vertex, normal):
    """The pass: a copy of `normal` with every record that has entries, and a sum of finite length > 0, replaced by s / len."""
    vertex = np.asarray(vertex, np.float64); out = np.array(normal, np.float64)
    off = offset.astype(np.int64); count = np.diff(off)
    e = entry.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = _cross(vertex[e[:, 0]], vertex[e[:, 1]], vertex[e[:, 2]])
        sigma = np.where(e[:, 3] != 0, -1.0, 1.0)[:, None]
        s = np.zeros((count.shape[0], 3))
        for k in range(int(count.max()) if count.size else 0):               # the k-th entry of every record that has one: stored order per record
            r = np.flatnonzero(count > k)
            s[r] = s[r] + sigma[off[r] + k] * c[off[r] + k]
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        write = (count > 0) & (length > 0) & np.isfinite(length)
        out[write] = s[write] / length[write][:, None]
    return out


def auto_normals(face, vertex, normal, mask=None, ref_vertex=None, ref_normal=None):
    """The normals after the pass for the current `vertex` / `normal`, with the lists taken at the reference pose (default: the same arrays)."""
    offset, entry = per_record(face, np.asarray(normal).shape[0], vertex if ref_vertex is None else ref_vertex, normal if ref_normal is None else ref_normal, mask)
    return apply(offset, entry, vertex, normal)


def mean_angle_deg(a, b):
    """Mean and max angle in degrees between the rows of two arrays of unit vectors."""
    d = np.clip((a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)), -1.0, 1.0)
    ang = np.degrees(np.arccos(d))
    return float(ang.mean()), float(ang.max())
