"""numpy restatement of keyframe playback (csrc/keyframes.hip): the time's segment, taps and weights, the reach, both kernels and the
set-up checks, in the order of operations the library fixes.  Python floats are IEEE doubles, math.fmod and every +, -, *, / and sqrt are
correctly rounded, so the device and the host must agree with this file bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

LINEAR, CATMULL_ROM = 0, 1
CLAMP, LOOP = 0, 1
MAX_FRAMES = 65536
MAX_COORD = 1e18


def segment(time, start_time, frame_time, n_frames, wrap):
    """(k, u) of a finite time: kf_segment's first three steps."""
    K = float(n_frames)
    x = (float(time) - float(start_time)) / float(frame_time)
    if wrap == CLAMP:
        if x <= 0.0:
            x = 0.0
        elif x >= K - 1.0:
            x = K - 1.0
    else:
        x = math.fmod(x, K) if math.isfinite(x) else math.nan
        if x < 0.0:
            x = x + K
        if not (x < K):
            x = 0.0
    k = math.floor(x)
    return int(k), x - float(k)


def taps(k, n_frames, interpolation, wrap):
    """The 2 or 4 frame indices that segment k blends."""
    first = k if interpolation == LINEAR else k - 1
    out = []
    for i in range(first, first + (2 if interpolation == LINEAR else 4)):
        out.append(min(max(i, 0), n_frames - 1) if wrap == CLAMP else (i + n_frames) % n_frames)
    return out


def weights(u, interpolation):
    """The 2 or 4 weights of u, never renormalised."""
    u = float(u)
    if interpolation == LINEAR:
        return [1.0 - u, u]
    u2 = u * u; u3 = u2 * u
    return [0.5 * ((2.0 * u2 - u3) - u), 0.5 * ((3.0 * u3 - 5.0 * u2) + 2.0), 0.5 * ((4.0 * u2 - 3.0 * u3) + u), 0.5 * (u3 - u2)]


def reach(radius, interpolation):
    """(1 + 2^-16) (c R)."""
    return (1.0 + 2.0 ** -16) * ((1.0 if interpolation == LINEAR else 1.25) * float(radius))


def radius(vertex_frames, used):
    """R: the largest |coordinate| among the vertices that a face uses (`used`: boolean per vertex), over all frames; 0 without any."""
    v = np.abs(np.asarray(vertex_frames, np.float64)[:, np.asarray(used, bool)])
    return float(v.max()) if v.size else 0.0


def _mix(frames, tap, w):
    f = np.asarray(frames, np.float64)
    s = w[0] * f[tap[0]] + w[1] * f[tap[1]]
    for t in range(2, len(tap)):
        s = s + w[t] * f[tap[t]]
    return s


def play_vertices(vertex_frames, time, start_time=0.0, frame_time=1.0, interpolation=LINEAR, wrap=CLAMP):
    """kf_vertices_kernel, or the copy of frame k when u == 0: the (n, 3) vertices at `time`."""
    f = np.asarray(vertex_frames, np.float64)
    k, u = segment(time, start_time, frame_time, f.shape[0], wrap)
    if u == 0.0:
        return f[k].copy()
    return _mix(f, taps(k, f.shape[0], interpolation, wrap), weights(u, interpolation))


def play_normals(normal_frames, time, start_time=0.0, frame_time=1.0, interpolation=LINEAR, wrap=CLAMP):
    """kf_normals_kernel, or the copy of frame k (as given, not normalised) when u == 0."""
    f = np.asarray(normal_frames, np.float64)
    k, u = segment(time, start_time, frame_time, f.shape[0], wrap)
    if u == 0.0:
        return f[k].copy()
    s = _mix(f, taps(k, f.shape[0], interpolation, wrap), weights(u, interpolation))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        unit = (length > 0.0) & (length < np.inf)
        return np.where(unit[:, None], s / np.where(unit, length, 1.0)[:, None], s)


def accepts(vertex_frames, normal_frames, used, n_vertex, n_normal, start_time=0.0, frame_time=1.0, interpolation=LINEAR, wrap=CLAMP):
    """mcpt_set_vertex_keyframes' rules for arrays of shape (n_frames, n, 3)."""
    v = np.asarray(vertex_frames, np.float64)
    if v.ndim != 3 or v.shape[1] != n_vertex or (normal_frames is not None and np.asarray(normal_frames).shape[1:] != (n_normal, 3)):
        return False
    if interpolation not in (LINEAR, CATMULL_ROM) or wrap not in (CLAMP, LOOP) or not 2 <= v.shape[0] <= MAX_FRAMES:
        return False
    if not math.isfinite(start_time) or not (math.isfinite(frame_time) and frame_time > 0.0):
        return False
    if not np.all(np.abs(v[:, np.asarray(used, bool)]) <= MAX_COORD):
        return False
    if normal_frames is not None and not np.isfinite(np.asarray(normal_frames, np.float64)).all():
        return False
    return reach(radius(v, used), interpolation) <= MAX_COORD
