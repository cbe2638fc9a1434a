"""numpy restatement of dual-quaternion skinning: the host functions sk_bone_gram, sk_bone_rigid, sk_dq_reach and sk_bone_dualquat
of csrc/skin.hip, the two kernels sk_dq_vertices_kernel and sk_dq_normals_kernel, and mcpt_update_skin's validation in that mode.

Every product, sum, difference, quotient and root below is ONE numpy operation on fp64 arrays -- correctly rounded, never fused -- in the
association §21 fixes, so the arrays are the device's bit for bit.  All four influence slots are accumulated, a slot of weight 0 included, as in
tests/skin_ref.py.  The records, the weight checks, R_b and the determinant are tests/skin_ref.py's and tests/transform_ref.py's.
"""
from __future__ import annotations

import numpy as np

from tests import skin_ref as S, transform_ref as T

LINEAR, DUAL_QUATERNION = 0, 1
RECORD = 8                                                                   # doubles per bone: w x y z dw dx dy dz
MAX_COORD = T.MAX_COORD
SLACK = S.SLACK
RIGID_TOLERANCE = 1e-6
MIN_NORM2 = 2.0 ** -8                                                        # a blended rotation part shorter than 1/16 is degenerate


def _m(m):
    return np.ascontiguousarray(m, np.float64).reshape(-1, 3, 4)


# ------------------------------------------------------------------------------------------------------------------------ host
def gram(m):
    """(n, 6) the entries (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) of A^T A, each (a0i a0j + a1i a1j) + a2i a2j."""
    a = _m(m)
    out = np.empty((a.shape[0], 6), np.float64)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        out[:, k] = (a[:, 0, i] * a[:, 0, j] + a[:, 1, i] * a[:, 1, j]) + a[:, 2, i] * a[:, 2, j]
    return out


def rigid(m):
    """(n,) bool: det A > 0 (transform_ref's determinant) and every entry of A^T A within 1e-6 of the identity's."""
    with np.errstate(all="ignore"):
        det = T.determinants(m)
        off = np.abs(gram(m) - np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]))
        return (det > 0.0) & (off <= RIGID_TOLERANCE).all(1)                 # (a NaN fails both)


def reach(m, radius):
    """(n,) per bone (1 + 2^-16) (2 R_b + 16 ((|tx| + |ty|) + |tz|))."""
    b = np.abs(_m(m))
    return SLACK * (2.0 * np.asarray(radius, np.float64) + 16.0 * ((b[:, 0, 3] + b[:, 1, 3]) + b[:, 2, 3]))


def shepperd_branch(m):
    """(n,) which of {trace, a00, a11, a22} is the largest; the first wins a tie."""
    a = _m(m)
    cand = np.stack([(a[:, 0, 0] + a[:, 1, 1]) + a[:, 2, 2], a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], 1)
    return np.argmax(cand, 1)                                                # (argmax: the first of equal maxima)


def raw_quaternion(m):
    """(n, 4) w x y z by Shepperd's method, before the normalisation and the sign rule."""
    a = _m(m)
    a00, a01, a02 = a[:, 0, 0], a[:, 0, 1], a[:, 0, 2]
    a10, a11, a12 = a[:, 1, 0], a[:, 1, 1], a[:, 1, 2]
    a20, a21, a22 = a[:, 2, 0], a[:, 2, 1], a[:, 2, 2]
    pick = shepperd_branch(a)
    q = np.empty((a.shape[0], 4), np.float64)
    with np.errstate(all="ignore"):
        s = 2.0 * np.sqrt(1.0 + ((a00 + a11) + a22))
        b = np.stack([0.25 * s, (a21 - a12) / s, (a02 - a20) / s, (a10 - a01) / s], 1); q[pick == 0] = b[pick == 0]
        s = 2.0 * np.sqrt(1.0 + ((a00 - a11) - a22))
        b = np.stack([(a21 - a12) / s, 0.25 * s, (a01 + a10) / s, (a02 + a20) / s], 1); q[pick == 1] = b[pick == 1]
        s = 2.0 * np.sqrt(1.0 + ((a11 - a00) - a22))
        b = np.stack([(a02 - a20) / s, (a01 + a10) / s, 0.25 * s, (a12 + a21) / s], 1); q[pick == 2] = b[pick == 2]
        s = 2.0 * np.sqrt(1.0 + ((a22 - a00) - a11))
        b = np.stack([(a10 - a01) / s, (a02 + a20) / s, (a12 + a21) / s, 0.25 * s], 1); q[pick == 3] = b[pick == 3]
    return q


def dualquats(m):
    """sk_bone_dualquat: (n, 8) w x y z dw dx dy dz -- the raw quaternion divided by its length, negated when w < 0; the dual part 1/2 (0, t) q."""
    a = _m(m)
    q = raw_quaternion(a)
    with np.errstate(all="ignore"):
        ln = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        q = q / ln[:, None]
        q = np.where((q[:, 0] < 0.0)[:, None], -q, q)
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        tx, ty, tz = a[:, 0, 3], a[:, 1, 3], a[:, 2, 3]
        out = np.empty((a.shape[0], RECORD), np.float64)
        out[:, :4] = q
        out[:, 4] = -0.5 * ((tx * x + ty * y) + tz * z)
        out[:, 5] = 0.5 * ((w * tx + ty * z) - tz * y)
        out[:, 6] = 0.5 * ((w * ty + tz * x) - tx * z)
        out[:, 7] = 0.5 * ((w * tz + tx * y) - ty * x)
    return out


def accepts_dq(m, radius):
    """mcpt_update_skin's checks of the matrices in dual-quaternion mode: finite entries, det A finite and non-zero (the checks both modes
    share), every bone rigid, and per bone the reach <= 1e18."""
    a = _m(m)
    if a.shape[0] != len(radius) or not np.isfinite(a).all():
        return False
    with np.errstate(all="ignore"):
        det = T.determinants(a)
        if not (np.isfinite(det) & (det != 0.0)).all() or not rigid(a).all():
            return False
        return bool((reach(a, radius) <= MAX_COORD).all())


# ------------------------------------------------------------------------------------------------------------------------ device
def signed_weights(bone, weight, table):
    """(n, 4) the weights as the blend takes them: slot 0 as it is, slot k negated when its rotation quaternion's dot product with slot 0's is < 0."""
    b, w = S._records(bone, weight)
    q = np.ascontiguousarray(table, np.float64).reshape(-1, RECORD)[:, :4]
    q0 = q[b[:, 0]]
    out = w.copy()
    for k in range(1, S.INFLUENCES):
        qk = q[b[:, k]]
        dot = ((q0[:, 0] * qk[:, 0] + q0[:, 1] * qk[:, 1]) + q0[:, 2] * qk[:, 2]) + q0[:, 3] * qk[:, 3]
        out[:, k] = w[:, k] * np.where(dot < 0.0, -1.0, 1.0)
    return out


def blend(bone, weight, table):
    """(n, 8) per record ((w0 q0 + (w1 s1) q1) + (w2 s2) q2) + (w3 s3) q3, componentwise."""
    b, _ = S._records(bone, weight)
    q = np.ascontiguousarray(table, np.float64).reshape(-1, RECORD)
    ws = signed_weights(bone, weight, q)
    with np.errstate(all="ignore"):
        t = [ws[:, k, None] * q[b[:, k]] for k in range(S.INFLUENCES)]
        return ((t[0] + t[1]) + t[2]) + t[3]


def norm2(bq):
    return ((bq[:, 0] * bq[:, 0] + bq[:, 1] * bq[:, 1]) + bq[:, 2] * bq[:, 2]) + bq[:, 3] * bq[:, 3]


def regular(n2):
    with np.errstate(all="ignore"):
        return (n2 >= MIN_NORM2) & (n2 < np.inf)                             # (a NaN fails both)


def rotation_of(r):
    """(n, 3, 3) the rotation matrix of unit quaternions w x y z: the usual nine formulas."""
    w, x, y, z = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    R = np.empty((r.shape[0], 3, 3), np.float64)
    R[:, 0, 0] = 1.0 - 2.0 * (y * y + z * z); R[:, 0, 1] = 2.0 * (x * y - w * z); R[:, 0, 2] = 2.0 * (x * z + w * y)
    R[:, 1, 0] = 2.0 * (x * y + w * z); R[:, 1, 1] = 1.0 - 2.0 * (x * x + z * z); R[:, 1, 2] = 2.0 * (y * z - w * x)
    R[:, 2, 0] = 2.0 * (x * z - w * y); R[:, 2, 1] = 2.0 * (y * z + w * x); R[:, 2, 2] = 1.0 - 2.0 * (x * x + y * y)
    return R


def skin_vertices_from_table(rest, bone, weight, table):
    """sk_dq_vertices_kernel on a table of dual quaternions."""
    p = np.ascontiguousarray(rest, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        bq = blend(bone, weight, table)
        n2 = norm2(bq); ok = regular(n2)
        n = np.sqrt(n2)
        r = bq[:, :4] / n[:, None]; d = bq[:, 4:] / n[:, None]
        R = rotation_of(r)
        rw, rx, ry, rz = r[:, 0], r[:, 1], r[:, 2], r[:, 3]; dw, dx, dy, dz = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
        t = [2.0 * (((rw * dx - dw * rx) + ry * dz) - rz * dy), 2.0 * (((rw * dy - dw * ry) + rz * dx) - rx * dz), 2.0 * (((rw * dz - dw * rz) + rx * dy) - ry * dx)]
        out = np.empty_like(p)
        for a in range(3):
            out[:, a] = ((R[:, a, 0] * x + R[:, a, 1] * y) + R[:, a, 2] * z) + t[a]
    out[~ok] = p[~ok]                                                        # a degenerate blend: the rest pose's record, bit for bit
    return out


def skin_normals_from_table(rest, bone, weight, table):
    """sk_dq_normals_kernel on a table of dual quaternions: only the rotation parts are read."""
    p = np.ascontiguousarray(rest, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        bq = blend(bone, weight, table)
        n2 = norm2(bq); ok = regular(n2)
        R = rotation_of(bq[:, :4] / np.sqrt(n2)[:, None])
        v = np.empty_like(p)
        for a in range(3):
            v[:, a] = (R[:, a, 0] * x + R[:, a, 1] * y) + R[:, a, 2] * z
        ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        unit = np.isfinite(ln) & (ln > 0.0)
        out = v.copy()
        out[unit] = v[unit] / ln[unit][:, None]
    out[~ok] = p[~ok]                                                        # copied, NOT normalised
    return out


def skin_vertices(rest, bone, weight, m):
    """What mcpt_update_skin writes to the vertices in dual-quaternion mode, from the caller's 3x4 matrices."""
    return skin_vertices_from_table(rest, bone, weight, dualquats(m))


def skin_normals(rest, bone, weight, m):
    return skin_normals_from_table(rest, bone, weight, dualquats(m))
