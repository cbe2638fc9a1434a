"""numpy restatement of csrc/morph.hip: the two kernels, the per-record conversion, mcpt_set_vertex_morph's checks and
mcpt_update_morph's validation.

Every product, sum, quotient and root below is ONE numpy operation on fp64 arrays -- correctly rounded, never fused.  The kernels sum a record's
entries in stored order, ascending target id; here the targets are applied one after the other, ascending, each to the records it names:
`p[idx_k] = p[idx_k] + w[k] * delta_k`.  Per record that is exactly the stored order (indices are strictly ascending inside a target, so no
record is named twice by one fancy-indexed assignment); morph_by_records walks the per-record lists explicitly and the tests hold the two to the
same bytes.  Every entry is accumulated, one whose weight is 0 included: 0 * d is +0 or -0 by d's sign and -0 + +0 is +0, so leaving the term
out would change the sign of a zero.  The normalisation rule is tests/transform_ref.py's.
"""
from __future__ import annotations

import numpy as np

from tests import skin_ref as S, transform_ref as T

MAX_COORD = T.MAX_COORD
MAX_TARGETS = 65536
SLACK = 1.0 + 2.0 ** -16


def _targets(targets):
    return [(np.asarray(i, np.int64).reshape(-1), np.ascontiguousarray(d, np.float64).reshape(-1, 3)) for i, d in targets]


def accepts_targets(targets, n_records, n_targets=None):
    """mcpt_set_vertex_morph's checks of one set of targets (offsets that start at 0 and do not decrease hold by construction of a list):
    n_targets in [1, 65536] (and equal to the other set's), every index < n_records and strictly ascending inside its target, every delta
    component finite with |d| <= 1e18."""
    if not 1 <= len(targets) <= MAX_TARGETS or (n_targets is not None and len(targets) != n_targets):
        return False
    for i, d in _targets(targets):
        if i.shape[0] != d.shape[0]:
            return False
        if i.size and (i.min() < 0 or i.max() >= n_records or (np.diff(i) <= 0).any()):
            return False
        with np.errstate(all="ignore"):
            if not (np.abs(d) <= MAX_COORD).all():                           # (a NaN fails)
                return False
    return True


def per_record(targets, n_records):
    """mo_per_record: (offset (n_records + 1), target id per entry, delta per entry); record i owns entries [offset[i], offset[i + 1]), ordered by
    ascending target id."""
    t = _targets(targets)
    index = np.concatenate([i for i, _ in t]) if t else np.zeros(0, np.int64)
    target = np.concatenate([np.full(i.shape[0], k, np.int64) for k, (i, _) in enumerate(t)]) if t else np.zeros(0, np.int64)
    delta = np.concatenate([d for _, d in t]) if t else np.zeros((0, 3))
    order = np.lexsort((target, index))                                      # by record, then by target
    offset = np.zeros(n_records + 1, np.int64)
    np.add.at(offset, index + 1, 1)
    return np.cumsum(offset).astype(np.uint32), target[order].astype(np.uint32), delta[order]


def _normalised(v, touched):
    """§16's rule on the touched records: v / |v| with |v| = sqrt((x x + y y) + z z) where that is finite and > 0, else v."""
    out = v.copy()
    with np.errstate(all="ignore"):
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        length = np.sqrt((x * x + y * y) + z * z)
        unit = touched & (length > 0.0) & np.isfinite(length)
        out[unit] = v[unit] / length[unit, None]
    return out


def morph_vertices(rest, targets, weight):
    """mo_vertices_kernel: rest + the weighted entries, target after target."""
    p = np.array(rest, np.float64).reshape(-1, 3)
    w = np.ascontiguousarray(weight, np.float64).reshape(-1)
    t = _targets(targets)
    assert len(t) == w.shape[0]
    with np.errstate(all="ignore"):
        for k, (i, d) in enumerate(t):
            p[i] = p[i] + w[k] * d
    return p


def morph_normals(rest, targets, weight):
    """mo_normals_kernel: the same sum; records with >= 1 entry are then normalised, the others stay the rest pose's bits."""
    r = np.ascontiguousarray(rest, np.float64).reshape(-1, 3)
    if targets is None:
        return r.copy()
    touched = np.zeros(r.shape[0], bool)
    for i, _ in _targets(targets):
        touched[i] = True
    return _normalised(morph_vertices(r, targets, weight), touched)


def morph_by_records(rest, targets, weight, normalise=False):
    """The kernels' own walk: per record its list in stored order.  Slow; for the tests that hold morph_vertices / morph_normals to it."""
    p = np.array(rest, np.float64).reshape(-1, 3)
    w = np.ascontiguousarray(weight, np.float64).reshape(-1)
    offset, target, delta = per_record(targets, p.shape[0])
    touched = np.zeros(p.shape[0], bool)
    for i in range(p.shape[0]):
        for e in range(int(offset[i]), int(offset[i + 1])):
            p[i] = p[i] + w[target[e]] * delta[e]
            touched[i] = True
    return _normalised(p, touched) if normalise else p


def rest_radius(vertex, used):
    """R: the largest |coordinate| among the vertices that a face uses; 0 without any."""
    v = np.abs(np.ascontiguousarray(vertex, np.float64).reshape(-1, 3))[np.asarray(used, bool)]
    return float(v.max()) if v.size else 0.0


def target_delta(targets, used):
    """D_k: per target the largest |delta component| among its entries whose vertex a face uses; 0 without any."""
    u = np.asarray(used, bool)
    out = np.zeros(len(targets), np.float64)
    for k, (i, d) in enumerate(_targets(targets)):
        a = np.abs(d[u[i]])
        out[k] = a.max() if a.size else 0.0
    return out


def reach(radius, weight, delta):
    """E = (1 + 2^-16) (R + sum_k |w_k| D_k), the sum sequential in k starting from R."""
    s = np.float64(radius)
    with np.errstate(all="ignore"):
        for w, d in zip(np.ascontiguousarray(weight, np.float64).reshape(-1), np.ascontiguousarray(delta, np.float64).reshape(-1)):
            s = s + np.abs(w) * d
        return np.float64(SLACK) * s


def accepts(weight, radius, delta, bones=None, n_bones=None):
    """mcpt_update_morph's checks: n_targets, every weight finite with |w| <= 1e18, the reach <= 1e18; with bones, mcpt_update_skin's checks of
    the matrices with the reach as EVERY bone's radius."""
    w = np.ascontiguousarray(weight, np.float64).reshape(-1)
    if w.shape[0] != len(delta):
        return False
    with np.errstate(all="ignore"):
        if not (np.abs(w) <= MAX_COORD).all():
            return False
        e = reach(radius, w, delta)
        if not e <= MAX_COORD:
            return False
    if bones is None:
        return True
    m = np.ascontiguousarray(bones, np.float64).reshape(-1, 3, 4)
    if n_bones is not None and m.shape[0] != n_bones:
        return False
    return S.accepts(m, np.full(m.shape[0], e))


def morph_then_skin(rest_vertex, rest_normal, vertex_targets, normal_targets, weight, skin, bones):
    """mcpt_update_morph with bones: skin_ref's kernels applied to the morphed arrays, with the skin's own influences."""
    vb, vw, nb, nw = skin
    return (S.skin_vertices(morph_vertices(rest_vertex, vertex_targets, weight), vb, vw, bones),
            S.skin_normals(morph_normals(rest_normal, normal_targets, weight), nb, nw, bones))
