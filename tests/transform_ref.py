"""numpy restatement of csrc/transform.hip: the two kernels, the host-side cofactors and mcpt_update_transforms' validation.

Every product, sum, difference, quotient and root below is ONE numpy operation on fp64 arrays -- correctly rounded, never fused -- in the
association the kernels use, so the arrays are the device's bit for bit.
"""
from __future__ import annotations

import numpy as np

MAX_COORD = 1e18


def cofactors(m):
    """(n, 3, 3) cofactor matrices of the A of (n, 3, 4) matrices [A | t]: every entry p*q - r*s, two products and one subtraction."""
    a = np.ascontiguousarray(m, np.float64).reshape(-1, 3, 4)
    a00, a01, a02 = a[:, 0, 0], a[:, 0, 1], a[:, 0, 2]
    a10, a11, a12 = a[:, 1, 0], a[:, 1, 1], a[:, 1, 2]
    a20, a21, a22 = a[:, 2, 0], a[:, 2, 1], a[:, 2, 2]
    c = np.empty((a.shape[0], 3, 3), np.float64)
    c[:, 0, 0] = a11 * a22 - a12 * a21; c[:, 0, 1] = a12 * a20 - a10 * a22; c[:, 0, 2] = a10 * a21 - a11 * a20
    c[:, 1, 0] = a02 * a21 - a01 * a22; c[:, 1, 1] = a00 * a22 - a02 * a20; c[:, 1, 2] = a01 * a20 - a00 * a21
    c[:, 2, 0] = a01 * a12 - a02 * a11; c[:, 2, 1] = a02 * a10 - a00 * a12; c[:, 2, 2] = a00 * a11 - a01 * a10
    return c


def determinants(m):
    """det A = (a00 c00 + a01 c01) + a02 c02 per matrix, from the cofactors above."""
    a = np.ascontiguousarray(m, np.float64).reshape(-1, 3, 4); c = cofactors(a)
    return (a[:, 0, 0] * c[:, 0, 0] + a[:, 0, 1] * c[:, 0, 1]) + a[:, 0, 2] * c[:, 0, 2]


def transform_vertices(rest, group, m):
    """xf_vertices_kernel: per row ((a0 x + a1 y) + a2 z) + t of the vertex's group."""
    a = np.ascontiguousarray(m, np.float64).reshape(-1, 3, 4)[np.asarray(group, np.int64)]
    p = np.ascontiguousarray(rest, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    for r in range(3):
        out[:, r] = ((a[:, r, 0] * x + a[:, r, 1] * y) + a[:, r, 2] * z) + a[:, r, 3]
    return out


def transform_normals(rest, group, m):
    """xf_normals_kernel: c = cof(A) n per row (c0 x + c1 y) + c2 z; c / |c| where |c| is finite and > 0, else c."""
    c = cofactors(m)[np.asarray(group, np.int64)]
    p = np.ascontiguousarray(rest, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    v = np.empty_like(p)
    with np.errstate(all="ignore"):
        for r in range(3):
            v[:, r] = (c[:, r, 0] * x + c[:, r, 1] * y) + c[:, r, 2] * z
        ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        unit = np.isfinite(ln) & (ln > 0.0)
        out = v.copy()
        out[unit] = v[unit] / ln[unit][:, None]
    return out


def group_radius(vertex, vertex_group, used, n_groups):
    """R_g: the largest |coordinate| among the group's vertices that a face uses; 0 for a group without any."""
    r = np.zeros(n_groups, np.float64)
    v = np.abs(np.ascontiguousarray(vertex, np.float64).reshape(-1, 3)).max(axis=1)
    u = np.asarray(used, bool)
    np.maximum.at(r, np.asarray(vertex_group, np.int64)[u], v[u])
    return r


def used_vertices(scene):
    u = np.zeros(scene.vertex.shape[0], bool)
    u[np.unique(scene.face[:, :, 0])] = True
    return u


def reach(m, radius):
    """(n, 3) per row ((|a0| + |a1|) + |a2|) R_g + |t|: how far the row can carry a coordinate of its group."""
    b = np.abs(np.ascontiguousarray(m, np.float64).reshape(-1, 3, 4))
    return ((b[:, :, 0] + b[:, :, 1]) + b[:, :, 2]) * np.asarray(radius, np.float64)[:, None] + b[:, :, 3]


def accepts(m, radius):
    """mcpt_update_transforms' checks of the matrices themselves: finite entries, det A finite and non-zero, and per row the conservative reach
    ((|a0| + |a1|) + |a2|) R_g + |t| <= 1e18."""
    a = np.ascontiguousarray(m, np.float64).reshape(-1, 3, 4)
    if a.shape[0] != len(radius) or not np.isfinite(a).all():
        return False
    with np.errstate(all="ignore"):
        det = determinants(a)
        if not (np.isfinite(det) & (det != 0.0)).all():
            return False
        far = reach(a, radius)
    return bool((far <= MAX_COORD).all())


def identity(n):
    m = np.zeros((n, 3, 4), np.float64)
    m[:, 0, 0] = m[:, 1, 1] = m[:, 2, 2] = 1.0
    return m


def about(a3x3, pivot, shift=(0.0, 0.0, 0.0)):
    """The 3x4 matrix of x -> A (x - pivot) + pivot + shift."""
    a = np.asarray(a3x3, np.float64); p = np.asarray(pivot, np.float64)
    return np.concatenate([a, (p - a @ p + np.asarray(shift, np.float64))[:, None]], axis=1)


def rotation(axis, degrees):
    k = np.asarray(axis, np.float64); k = k / np.linalg.norm(k)
    t = np.radians(degrees); K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)
