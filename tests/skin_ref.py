"""numpy restatement of csrc/skin.hip: the two kernels, mcpt_set_vertex_skin's checks and mcpt_update_skin's validation.

Every product, sum, difference, quotient and root below is ONE numpy operation on fp64 arrays -- correctly rounded, never fused -- in the
association the kernels use, so the arrays are the device's bit for bit.  All four influence slots are accumulated, a slot of weight 0 included:
0 * m is +0 or -0 by m's sign, and leaving the term out would change the sign of a zero.  The cofactor formulas, the normalisation rule and the
helpers are tests/transform_ref.py's.
"""
from __future__ import annotations

import numpy as np

from tests import transform_ref as T

INFLUENCES = 4
MAX_COORD = T.MAX_COORD
SLACK = 1.0 + 2.0 ** -16                                                     # covers a weight sum of up to 1 + 1e-6 and the blend's rounding
SUM_TOLERANCE = 1e-6


def _records(bone, weight):
    b = np.ascontiguousarray(bone, np.int64).reshape(-1, INFLUENCES); w = np.ascontiguousarray(weight, np.float64).reshape(-1, INFLUENCES)
    assert b.shape == w.shape
    return b, w


def blend(bone, weight, m):
    """(n, 3, 4) per record B = ((w0 M0 + w1 M1) + w2 M2) + w3 M3, entrywise."""
    b, w = _records(bone, weight)
    a = np.ascontiguousarray(m, np.float64).reshape(-1, 3, 4)
    t = [w[:, k, None, None] * a[b[:, k]] for k in range(INFLUENCES)]
    return ((t[0] + t[1]) + t[2]) + t[3]


def skin_vertices(rest, bone, weight, m):
    """sk_vertices_kernel: per row ((B0 x + B1 y) + B2 z) + B3 of the record's blended matrix."""
    B = blend(bone, weight, m)
    p = np.ascontiguousarray(rest, np.float64).reshape(-1, 3)
    return T.transform_vertices(p, np.arange(p.shape[0]), B)


def skin_normals(rest, bone, weight, m):
    """sk_normals_kernel: C = cof(A_B) of the record's blended matrix, v = (C0 x + C1 y) + C2 z per row; v / |v| where |v| is finite and > 0, else v."""
    with np.errstate(all="ignore"):
        B = blend(bone, weight, m)
    p = np.ascontiguousarray(rest, np.float64).reshape(-1, 3)
    return T.transform_normals(p, np.arange(p.shape[0]), B)


def weight_sums(weight):
    w = np.ascontiguousarray(weight, np.float64).reshape(-1, INFLUENCES)
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def accepts_skin(bone, weight, n_bones):
    """mcpt_set_vertex_skin's checks of one array of records: every id < n_bones (zero-weight slots included), every weight finite and in
    [0, 1], |S - 1| <= 1e-6 for S = ((w0 + w1) + w2) + w3."""
    b, w = _records(bone, weight)
    if (b < 0).any() or (b >= n_bones).any():
        return False
    with np.errstate(all="ignore"):
        if not ((w >= 0.0) & (w <= 1.0)).all():                              # (a NaN fails both)
            return False
        return bool((np.abs(weight_sums(w) - 1.0) <= SUM_TOLERANCE).all())


def bone_radius(vertex, bone, weight, used, n_bones):
    """R_b: the largest |coordinate| among the vertices that a face uses and that give the bone a weight > 0; 0 for a bone without any."""
    b, w = _records(bone, weight)
    r = np.zeros(n_bones, np.float64)
    far = np.abs(np.ascontiguousarray(vertex, np.float64).reshape(-1, 3)).max(axis=1)
    u = np.asarray(used, bool)
    for k in range(INFLUENCES):
        on = u & (w[:, k] > 0.0)
        np.maximum.at(r, b[on, k], far[on])
    return r


def reach(m, radius):
    """(n, 3) per bone and row (1 + 2^-16) (((|a0| + |a1|) + |a2|) R_b + |t|)."""
    return SLACK * T.reach(m, radius)


def accepts(m, radius):
    """mcpt_update_skin's checks of the matrices themselves: finite entries, det A finite and non-zero per bone, and per row the conservative
    reach with its slack factor <= 1e18."""
    a = np.ascontiguousarray(m, np.float64).reshape(-1, 3, 4)
    if a.shape[0] != len(radius) or not np.isfinite(a).all():
        return False
    with np.errstate(all="ignore"):
        det = T.determinants(a)
        if not (np.isfinite(det) & (det != 0.0)).all():
            return False
        far = reach(a, radius)
    return bool((far <= MAX_COORD).all())


def single(group):
    """The influence records of one bone of weight 1 per record: (ids, weights), the other slots bone 0 with weight 0."""
    g = np.asarray(group, np.int64).reshape(-1)
    b = np.zeros((g.shape[0], INFLUENCES), np.uint32); w = np.zeros((g.shape[0], INFLUENCES), np.float64)
    b[:, 0] = g; w[:, 0] = 1.0
    return b, w
