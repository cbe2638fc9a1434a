"""Baked vertex animation from device-resident keyframes: mcpt_set_vertex_keyframes, mcpt_update_keyframes (csrc/keyframes.hip in
front of the refit), mcpt_update_keyframes_reproject, mcpt_get_keyframe_info and their public surfaces.

The reference throughout is tests/keyframes_ref.py (numpy and Python floats, the library's order of operations): fp64 multiply, add, divide,
sqrt and fmod are correctly rounded on both sides, so everything is compared BIT FOR BIT, without a tolerance -- directly, through
mcpt_probe_vertices, and downstream through §16's oracle: a second context of the same scene moved with mcpt_update_vertices to the restated
arrays.
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import deform_kit as K, keyframes_ref as F, kit, morph_ref as M, skin_ref as S, transform_ref as T
from tests.deform_kit import CENTRE, FLAGS, H, INVALID, M_HIGH, M_LAMP, M_LOW, N_BONES, SPHERE, UNSUPPORTED, W
from tests.kit import bits, render_film

NEW_SYMBOLS = ["mcpt_set_vertex_keyframes", "mcpt_update_keyframes", "mcpt_update_keyframes_reproject", "mcpt_get_keyframe_info"]
N_FRAMES = 5
START, FRAME_TIME = 0.0, 0.25                                               # x = time / 0.25 and time = 0.25 x are exact: a test names u itself
MODES = [F.LINEAR, F.CATMULL_ROM]
WRAPS = [F.CLAMP, F.LOOP]
BEND = K.mats(low=M_LOW, high=M_HIGH, lamp=M_LAMP)
LIFT = np.array([0.0, 0.1, 0.0])                                             # the sphere stands on the floor: lifted, every displaced frame stays inside the room


def _time(x):
    return START + FRAME_TIME * x


def _below_one(k):
    """The largest u < 1 that segment k can name: x = the double just below k + 1 (u = 1 - 2^-52 k for k = 1, 2 and 4; 1 - 2^-53 for k = 0)."""
    return math.nextafter(k + 1.0, 0.0) - k


@functools.lru_cache(maxsize=None)
def _frames(pkg, small):
    """Five frames over S-cornell (or S-cornell-small): the sphere's vertices lifted off the floor and displaced by a different smooth offset per
    frame, walls and lamp fixed (so the room's bounding box, and the centre every device coordinate is relative to, stay); the sphere's normals tilted per frame --
    unit length in frames 0, 1, 2 and 4, left at length 1.03 in frame 3 (normal frames are used as given).  Frame 2 carries negative zeros: every
    coordinate and normal component that is 0 there.  (vertex frames (5, nv, 3), normal frames (5, nn, 3).)"""
    s = K.scene(pkg, small); sphere, _ = K.parts(pkg, small)
    ni = np.unique(s.face[s.face[:, 0, 3] == SPHERE][:, :, 1])
    vf = np.repeat(s.vertex[None], N_FRAMES, 0); nf = np.repeat(s.normal[None], N_FRAMES, 0)
    p = s.vertex[sphere]; q = s.normal[ni]
    for k in range(N_FRAMES):
        a = 0.012 * (k + 1)
        vf[k][sphere] = p + LIFT + a * np.stack([np.sin(9.0 * p[:, 1] + k), np.sin(7.0 * p[:, 2] + 2 * k), np.sin(8.0 * p[:, 0] - k)], 1)
        n = q + 0.2 * np.stack([np.sin(5.0 * q[:, 1] + k), np.cos(6.0 * q[:, 0] - k), np.sin(4.0 * q[:, 2] + 3 * k)], 1)
        nf[k][ni] = n / np.linalg.norm(n, axis=1, keepdims=True) * (1.03 if k == 3 else 1.0)
    vf[2][vf[2] == 0.0] = -0.0; nf[2][nf[2] == 0.0] = -0.0
    return vf, nf


def _want(pkg, small, time, mode, wrap, normals=True, frames=None, start=START, frame_time=FRAME_TIME, rest_normal=None):
    """The arrays the time gives, by the restatement; without normal frames the normals captured at set-up (`rest_normal`, or the scene's)."""
    vf, nf = _frames(pkg, small) if frames is None else frames
    v = F.play_vertices(vf, time, start, frame_time, mode, wrap)
    if normals:
        return v, F.play_normals(nf, time, start, frame_time, mode, wrap)
    return v, K.scene(pkg, small).normal if rest_normal is None else rest_normal


def _set(pkg, R, small, mode, wrap, normals=True):
    vf, nf = _frames(pkg, small)
    R.set_vertex_keyframes(vf, nf if normals else None, START, FRAME_TIME, mode, wrap)


def _pair(pkg, small, mode=F.LINEAR, wrap=F.CLAMP, normals=True, extra=0):
    return K.pair(pkg, lambda R: _set(pkg, R, small, mode, wrap, normals), extra=extra, max_depth=6, scene=K.scene(pkg, small))


def _check_against_oracle(pkg, R, O, small, time, mode, wrap, normals=True, film=True, **kw):
    """update_keyframes on R, update_vertices with the restated arrays on O: the device arrays directly, then everything downstream."""
    v, n = _want(pkg, small, time, mode, wrap, normals, **kw)
    R.update_keyframes(time); O.update_vertices(v, n)
    K.assert_arrays(R, v, n)
    a, b = K.state(pkg, R, film, arrays=True), K.state(pkg, O, film, arrays=True)
    K.assert_same(a, b)
    return a


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_library_exports_the_keyframe_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, ("set_vertex_keyframes", "update_keyframes", "update_keyframes_reproject", "keyframe_info"))
    assert set(pkg.KeyframeInfo().as_dict()) == {"struct_size", "n_frames", "interpolation", "wrap", "updates", "last_frame", "last_u", "last_time", "last_ms", "device_bytes"}
    assert (pkg.KEYFRAMES_LINEAR, pkg.KEYFRAMES_CATMULL_ROM, pkg.KEYFRAMES_CLAMP, pkg.KEYFRAMES_LOOP) == (F.LINEAR, F.CATMULL_ROM, F.CLAMP, F.LOOP) == (0, 1, 0, 1)
    assert pkg.KEYFRAMES_MAX == F.MAX_FRAMES == 65536


def test_null_context_is_an_invalid_argument_for_the_keyframe_calls(pkg):
    lib = pkg.load_library()
    cam = pkg.CameraC(); info = pkg.KeyframeInfo()
    o = pkg.ReprojectOpts(); o.struct_size = C.sizeof(pkg.ReprojectOpts)
    v = np.zeros((2, 4, 3)); vp = v.ctypes.data_as(C.c_void_p)
    assert lib.mcpt_set_vertex_keyframes(None, vp, 4, vp, 4, 2, None) == INVALID and lib.mcpt_set_vertex_keyframes(None, vp, 4, None, 4, 2, None) == INVALID
    assert lib.mcpt_update_keyframes(None, 0.5) == INVALID
    assert lib.mcpt_update_keyframes_reproject(None, 0.5, None, None) == INVALID and lib.mcpt_update_keyframes_reproject(None, 0.5, C.byref(cam), C.byref(o)) == INVALID
    assert lib.mcpt_get_keyframe_info(None, C.byref(info)) == INVALID


def test_keyframe_structs_have_the_headers_layout(pkg, tmp_path):
    """sizeof and every offsetof of mcpt_keyframe_opts and mcpt_keyframe_info as a C compiler sees include/mcpt.h, against the ctypes classes, and
    the header's macros against the package's constants."""
    macros = ("MCPT_KEYFRAMES_LINEAR", "MCPT_KEYFRAMES_CATMULL_ROM", "MCPT_KEYFRAMES_CLAMP", "MCPT_KEYFRAMES_LOOP", "MCPT_KEYFRAMES_MAX")
    for cls, name, size in ((pkg.KeyframeOpts, "mcpt_keyframe_opts", 48), (pkg.KeyframeInfo, "mcpt_keyframe_info", 72)):
        c, py, values = K.c_layout(cls, name, tmp_path, macros)
        assert c == py and c[0] == size
        assert values == [pkg.KEYFRAMES_LINEAR, pkg.KEYFRAMES_CATMULL_ROM, pkg.KEYFRAMES_CLAMP, pkg.KEYFRAMES_LOOP, pkg.KEYFRAMES_MAX] == [0, 1, 0, 1, 65536]


def test_restatement_weights_and_segments():
    assert F.weights(0.5, F.CATMULL_ROM) == [-1.0 / 16, 9.0 / 16, 9.0 / 16, -1.0 / 16] and sum(abs(w) for w in F.weights(0.5, F.CATMULL_ROM)) == 1.25
    assert F.weights(0.0, F.CATMULL_ROM) == [0.0, 1.0, 0.0, 0.0] and F.weights(0.0, F.LINEAR) == [1.0, 0.0] and F.weights(0.25, F.LINEAR) == [0.75, 0.25]
    # a partition of unity, never more than 1.25 in absolute sum -- up to rounding: a weight is 0.5 times at most 4 rounded operations on values
    # <= 5, each off by <= 2^-53 * 8, so <= 1.8e-15 per weight once halved; 4 weights and their 3 additions: 8e-15 bounds the sum's error
    for u in np.random.default_rng(5).uniform(0, 1, 200):
        w = F.weights(u, F.CATMULL_ROM)
        assert abs(sum(w) - 1.0) <= 8e-15 and sum(abs(x) for x in w) <= 1.25 + 8e-15
    # LOOP: t, t + period and t - period name the same segment
    period = 4 * 0.25
    assert F.segment(0.375, 0.0, 0.25, 4, F.LOOP) == F.segment(0.375 + period, 0.0, 0.25, 4, F.LOOP) == F.segment(0.375 - period, 0.0, 0.25, 4, F.LOOP) == (1, 0.5)
    assert F.segment(0.875, 0.0, 0.25, 4, F.LOOP) == (3, 0.5) and F.taps(3, 4, F.LINEAR, F.LOOP) == [3, 0] and F.taps(3, 4, F.CATMULL_ROM, F.LOOP) == [2, 3, 0, 1]
    assert F.taps(0, 4, F.CATMULL_ROM, F.LOOP) == [3, 0, 1, 2] and F.taps(0, 4, F.CATMULL_ROM, F.CLAMP) == [0, 0, 1, 2] and F.taps(2, 4, F.CATMULL_ROM, F.CLAMP) == [1, 2, 3, 3]
    assert F.taps(2, 4, F.LINEAR, F.CLAMP) == [2, 3] and F.taps(3, 4, F.LINEAR, F.CLAMP) == [3, 3]
    # a negative x so small that x + K rounds to K, and an x that overflows: both play frame 0
    assert F.segment(-1e-300, 0.0, 0.25, 4, F.LOOP) == (0, 0.0) and F.segment(1e300, 0.0, 1e-300, 4, F.LOOP) == (0, 0.0) and F.segment(-0.0, 0.0, 0.25, 4, F.LOOP)[0] == 0
    # CLAMP pins every time at or before the first frame to (0, 0) and every time at or after the last to (K - 1, 0)
    for start, ft, n in ((0.0, 0.25, 4), (-3.5, 2.0, 7), (1e6, 1e-3, 65536)):
        last = start + ft * (n - 1)
        for t in (start, math.nextafter(start, -math.inf), start - 1.0, -1e300, -1e308):
            assert F.segment(t, start, ft, n, F.CLAMP) == (0, 0.0) and not math.copysign(1.0, F.segment(t, start, ft, n, F.CLAMP)[1]) < 0
        for t in (last, last + ft, math.nextafter(last, math.inf) + ft, 1e300, 1e308):
            assert F.segment(t, start, ft, n, F.CLAMP) == (n - 1, 0.0)
    k, u = F.segment(_time(_below_one(3) + 3), START, FRAME_TIME, N_FRAMES, F.CLAMP)
    assert (k, u) == (3, 1.0 - 2.0 ** -51) and _below_one(1) == 1.0 - 2.0 ** -52 and _below_one(2) == 1.0 - 2 * 2.0 ** -52 and _below_one(4) == 1.0 - 4 * 2.0 ** -52
    # the reach: the slack on c R
    assert F.reach(0.5, F.LINEAR) == (1.0 + 2.0 ** -16) * 0.5 and F.reach(0.5, F.CATMULL_ROM) == (1.0 + 2.0 ** -16) * 0.625
    assert F.reach(1e18, F.LINEAR) > 1e18 and F.reach(1e18 / (1.0 + 2.0 ** -15), F.LINEAR) <= 1e18 and F.reach(0.8e18, F.CATMULL_ROM) > 1e18 and F.reach(0.79e18, F.CATMULL_ROM) <= 1e18


def test_restatement_of_the_kernels_and_the_fixture(pkg):
    for small, records in ((True, 349), (False, 1249)):
        s = K.scene(pkg, small); vf, nf = _frames(pkg, small); sphere, lamp = K.parts(pkg, small)
        ni = np.unique(s.face[s.face[:, 0, 3] == SPHERE][:, :, 1])
        assert s.vertex.shape[0] == s.normal.shape[0] == records and vf.shape == nf.shape == (N_FRAMES, records, 3) and (3 * records) % 2 == 1
        assert np.signbit(vf[2][vf[2] == 0.0]).all() and (vf[2] == 0.0).sum() > 0 and np.signbit(nf[2][nf[2] == 0.0]).all() and not np.signbit(vf[1][vf[1] == 0.0]).any()
        assert np.array_equal(vf[:, ~sphere], np.repeat(s.vertex[None, ~sphere], N_FRAMES, 0))                        # the walls and the lamp stay
        assert vf[:, sphere].min() > 0.005 and vf[:, sphere].max() < 0.995                                         # inside the room
        assert all(not np.array_equal(vf[a], vf[b]) for a in range(N_FRAMES) for b in range(a))
        assert abs(np.linalg.norm(nf[3][ni], axis=1) - 1.03).max() < 1e-12 and abs(np.linalg.norm(nf[1][ni], axis=1) - 1.0).max() < 1e-12
        used = T.used_vertices(s)
        assert F.accepts(vf, nf, used, records, records) and F.accepts(vf, None, used, records, records, interpolation=F.CATMULL_ROM, wrap=F.LOOP)
        for mode in MODES:
            # on a keyframe: the frame itself, as given -- negative zeros and the normals' length included
            for k in range(N_FRAMES):
                assert np.array_equal(bits(F.play_vertices(vf, _time(k), START, FRAME_TIME, mode, F.LOOP)), bits(vf[k]))
                assert np.array_equal(bits(F.play_normals(nf, _time(k), START, FRAME_TIME, mode, F.CLAMP)), bits(nf[k]))
            # in between: one rounding per operation in the stated order; normals come out unit length
            v = F.play_vertices(vf, _time(1.25), START, FRAME_TIME, mode, F.CLAMP); n = F.play_normals(nf, _time(1.25), START, FRAME_TIME, mode, F.CLAMP)
            w = F.weights(0.25, mode); tap = F.taps(1, N_FRAMES, mode, F.CLAMP)
            i = int(np.flatnonzero(sphere)[7])
            want = w[0] * vf[tap[0]][i] + w[1] * vf[tap[1]][i]
            if mode == F.CATMULL_ROM:
                want = (want + w[2] * vf[tap[2]][i]) + w[3] * vf[tap[3]][i]
            assert np.array_equal(bits(v[i]), bits(want)) and abs(np.linalg.norm(n[ni], axis=1) - 1.0).max() <= 4 * np.finfo(np.float64).eps
        # LOOP's last segment blends frame K - 1 into frame 0; CLAMP holds the last frame there
        mid = F.play_vertices(vf, _time(4.5), START, FRAME_TIME, F.LINEAR, F.LOOP)
        assert np.array_equal(bits(mid), bits(0.5 * vf[4] + 0.5 * vf[0])) and np.array_equal(bits(F.play_vertices(vf, _time(4.5), START, FRAME_TIME, F.LINEAR, F.CLAMP)), bits(vf[4]))
    # a zero sum is left as it is, and so is one whose length overflows
    flat = F.play_normals(np.array([[[0.0, 1.0, 0.0]], [[0.0, -1.0, 0.0]]]), 0.5)
    assert np.array_equal(flat, np.zeros((1, 3)))
    big = F.play_normals(np.array([[[1e200, 0.0, 0.0]], [[1e200, 1e200, 0.0]]]), 0.5)
    assert np.array_equal(big, np.array([[1e200, 0.5e200, 0.0]]))


def test_restatement_refusals(pkg):
    s = K.scene(pkg, True); vf, nf = _frames(pkg, True); n = s.vertex.shape[0]
    used = T.used_vertices(s)
    assert (~used).sum() == 2
    ok = lambda v=vf, nr=nf, **kw: F.accepts(v, nr, used, n, n, **kw)
    assert ok() and not ok(vf[:1], nf[:1]) and ok(vf[:2], nf[:2]) and not ok(vf[:, :-1]) and not ok(nr=nf[:, :-1])
    assert not ok(interpolation=2) and not ok(wrap=2)
    for x in (math.nan, math.inf, -math.inf):
        assert not ok(start_time=x) and not ok(frame_time=x)
    assert not ok(frame_time=0.0) and not ok(frame_time=-0.25) and ok(frame_time=5e-324) and ok(start_time=-1e308)

    def edit(a, k, i, c, x):
        a = a.copy(); a[k, i, c] = x
        return a

    iu = int(np.flatnonzero(used)[11]); idle = int(np.flatnonzero(~used)[0])
    for x, fine in ((math.nan, False), (math.inf, False), (-math.inf, False), (1.0000001e18, False), (-0.99e18, True)):
        assert ok(edit(vf, 3, iu, 1, x)) == fine and ok(edit(vf, 3, idle, 1, x))                                     # a vertex no face uses is not judged
        assert ok(nr=edit(nf, 4, 5, 2, x)) == (math.isfinite(x))
    assert not ok(edit(vf, 0, iu, 0, 1e18)) and not ok(edit(vf, 0, iu, 0, 0.9e18), interpolation=F.CATMULL_ROM) and ok(edit(vf, 0, iu, 0, 0.9e18))     # the reach alone


def _host_check_cases():
    """(time, start_time, frame_time, R, n_frames, interpolation, wrap): a few thousand random ones and the edge times."""
    rng = np.random.default_rng(11)
    cases = []
    for _ in range(3000):
        n = int(rng.choice([2, 3, 4, 5, 7, 100, 65535, 65536])); start = float(rng.normal() * 10.0 ** rng.integers(-3, 4)); ft = float(10.0 ** rng.uniform(-4, 3))
        time = start + ft * float(rng.uniform(-2.5 * n, 3.5 * n))
        cases.append((time, start, ft, float(10.0 ** rng.uniform(-3, 18)), n, int(rng.integers(2)), int(rng.integers(2))))
    for mode in MODES:
        for wrap in WRAPS:
            for n, start, ft in ((4, 0.0, 0.25), (5, START, FRAME_TIME), (7, -3.5, 2.0), (65536, 1e6, 1e-3), (2, 0.1, 0.1)):
                last = start + ft * (n - 1); period = ft * n
                times = [start + ft * k for k in range(min(n, 9))] + [last, start + period, start - period, 0.375, 0.375 + period, 0.375 - period]
                times += [math.nextafter(start, -math.inf), math.nextafter(start, math.inf), math.nextafter(last, math.inf), math.nextafter(last, -math.inf)]
                times += [1e300, -1e300, 1e308, -1e308, 5e-324, -5e-324, 0.0, -0.0] + [_time(_below_one(k) + k) for k in range(5)]
                cases += [(t, start, ft, 1e18, n, mode, wrap) for t in times]
            cases += [(1e300, 0.0, 1e-300, 0.8e18, 4, mode, wrap), (-1e300, 0.0, 1e-300, 0.0, 4, mode, wrap), (-1e-300, 0.0, 0.25, 1.0, 4, mode, wrap)]
    return cases


@K.needs_hipcc
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_segment_weights_and_reach_are_the_restatement_bit_for_bit(pkg, tmp_path, sanitized):
    """The host half of the feature -- kf_segment, kf_weights and kf_reach of csrc/keyframes.hip -- built into the stand-alone program
    tests/keyframes_host_check.cpp (no device is touched) against tests/keyframes_ref.py: the same segment, taps, u, weights and reach, bit for
    bit.  `sanitized`: the same program under the host's address and undefined-behaviour sanitizers, which must stay silent."""
    exe = K.build_host_check("keyframes_host_check", ["keyframes.hip"], tmp_path, sanitized)
    cases = _host_check_cases()
    assert len(cases) > 3000
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(np.array([len(cases), 0], np.uint32).tobytes())
        for time, start, ft, radius, n, mode, wrap in cases:
            f.write(np.array([time, start, ft, radius], np.float64).tobytes()); f.write(np.array([n, mode, wrap, 0], np.uint32).tobytes())
    K.run_host_check(exe, tmp_path, sanitized)
    raw = open(str(tmp_path / "out.bin"), "rb").read()
    assert len(raw) == 72 * len(cases)
    for i, (time, start, ft, radius, n, mode, wrap) in enumerate(cases):
        ints = np.frombuffer(raw, np.uint32, 6, 72 * i); reals = np.frombuffer(raw, np.float64, 6, 72 * i + 24)
        k, u = F.segment(time, start, ft, n, wrap)
        tap = F.taps(k, n, mode, wrap); w = F.weights(u, mode)
        want_i = [k, len(tap)] + tap + [0] * (4 - len(tap)); want_r = np.array([u] + w + [0.0] * (4 - len(w)) + [F.reach(radius, mode)])
        assert ints.tolist() == want_i and np.array_equal(bits(reals), bits(want_r)), (cases[i], ints.tolist(), reals.tolist(), want_i, want_r.tolist())
        assert 0 <= k < n and 0.0 <= u < 1.0 and all(0 <= t < n for t in tap)


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("small", [True, False])
def test_on_a_keyframe_the_scene_is_that_frame(pkg, small, normals, mode):
    s = K.scene(pkg, small); vf, nf = _frames(pkg, small)
    R, O = _pair(pkg, small, mode, F.CLAMP, normals)
    K.assert_arrays(R, s.vertex, s.normal)                                   # setting keyframes moves nothing
    for k in (3, 0, 2, 4, 1):
        R.update_keyframes(_time(k)); O.update_vertices(vf[k], nf[k] if normals else s.normal)
        K.assert_arrays(R, vf[k], nf[k] if normals else s.normal)           # the frame as given: negative zeros (k = 2) and normals of length 1.03 (k = 3) included
        K.assert_same(K.state(pkg, R, film=k == 2, arrays=True), K.state(pkg, O, film=k == 2, arrays=True))
        ki = R.keyframe_info()
        assert (ki.last_frame, ki.last_u, ki.last_time) == (k, 0.0, _time(k))
    ki = R.keyframe_info(); ui = R.update_info()
    assert (ki.n_frames, ki.interpolation, ki.wrap, ki.updates) == (N_FRAMES, mode, F.CLAMP, 5) and ui.updates == 5 and 0 < ki.last_ms <= ui.last_update_ms
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("small", [True, False])
def test_between_keyframes_the_arrays_are_the_restatement(pkg, small, mode, wrap):
    """The first, a middle and the last segment (under LOOP also the wrap-around segment K - 1 -> 0), u = 0.25, 0.5 and the largest u below 1."""
    R, O = _pair(pkg, small, mode, wrap)
    vf, _ = _frames(pkg, small)
    segments = [0, 2, N_FRAMES - 2] + ([N_FRAMES - 1] if wrap == F.LOOP else [])
    for k in segments:
        for u in (0.25, 0.5, _below_one(k)):
            t = _time(k + u)
            assert F.segment(t, START, FRAME_TIME, N_FRAMES, wrap) == (k, u)
            _check_against_oracle(pkg, R, O, small, t, mode, wrap, film=u == 0.5)
            ki = R.keyframe_info()
            assert (ki.last_frame, ki.last_u, ki.last_time) == (k, u, t)
    v, _ = R.vertices()
    assert not any(np.array_equal(v, f) for f in vf)
    assert R.keyframe_info().updates == 3 * len(segments) == R.update_info().updates
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_loop_is_periodic_and_clamp_holds_the_end_frames(pkg, mode):
    small = True
    vf, nf = _frames(pkg, small)
    R, O = _pair(pkg, small, mode, F.LOOP)
    period = FRAME_TIME * N_FRAMES
    for t in (0.375, _time(4.5), _time(2.0)):
        got = []
        for shifted in (t, t + period, t - period, t + 3 * period):
            R.update_keyframes(shifted); got.append(R.vertices())
            assert F.segment(shifted, START, FRAME_TIME, N_FRAMES, F.LOOP) == F.segment(t, START, FRAME_TIME, N_FRAMES, F.LOOP)
        for v, n in got[1:]:
            assert np.array_equal(bits(v), bits(got[0][0])) and np.array_equal(bits(n), bits(got[0][1]))
        K.assert_arrays(R, *_want(pkg, small, t, mode, F.LOOP))
    _set(pkg, R, small, mode, F.CLAMP)
    for t, k in ((_time(-0.5), 0), (-1e300, 0), (_time(4.0), 4), (_time(4.5), 4), (1e300, 4), (_time(0.0), 0)):
        R.update_keyframes(t)
        K.assert_arrays(R, vf[k], nf[k])
        assert (R.keyframe_info().last_frame, R.keyframe_info().last_u) == (k, 0.0)
    R.update_keyframes(1e300); O.update_vertices(vf[4], nf[4])
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    R.close(); O.close()


@pytest.mark.gpu
def test_without_normal_frames_every_call_writes_the_normals_of_set_up(pkg):
    small = True
    s = K.scene(pkg, small); vf, nf = _frames(pkg, small)
    R, O = K.pair(pkg, None, max_depth=6, scene=s)
    R.update_vertices(s.vertex, nf[1])                                       # the normals at set-up are not the file's
    R.set_vertex_keyframes(vf, None, START, FRAME_TIME, F.CATMULL_ROM, F.LOOP)
    for t in (_time(1.5), _time(3.0), _time(4.75)):
        R.update_vertices(s.vertex, nf[2])                                   # overwritten in between: the call writes the captured normals, not these
        _check_against_oracle(pkg, R, O, small, t, F.CATMULL_ROM, F.LOOP, normals=False, film=False, rest_normal=nf[1])
    R.close(); O.close()


@pytest.mark.gpu
def test_auto_normals_run_after_the_keyframes(pkg):
    small = True
    R, O = _pair(pkg, small, F.LINEAR, F.CLAMP)
    for r in (R, O):
        r.set_auto_normals()
    before = R.normals_info().updates
    for i, t in enumerate((_time(1.5), _time(2.0), _time(3.25))):
        v, n = _want(pkg, small, t, F.LINEAR, F.CLAMP)
        R.update_keyframes(t); O.update_vertices(v, n)
        a, b = K.state(pkg, R, film=i == 0, arrays=True), K.state(pkg, O, film=i == 0, arrays=True)
        K.assert_same(a, b)
        assert np.array_equal(bits(a["vertex"]), bits(v)) and not np.array_equal(a["normal"], n)      # the pass has rewritten the sphere's normals
        assert R.normals_info().updates == before + i + 1
    R.close(); O.close()


@pytest.mark.gpu
def test_keyframes_skin_and_morph_leave_each_other_alone(pkg):
    small = False
    s = K.scene(pkg, small); sphere, _ = K.parts(pkg, small)
    vb, vw, nb, nw = K.bend(pkg)
    si = np.flatnonzero(sphere)
    targets = ([(si, s.vertex[si] - CENTRE)], [(si, np.random.default_rng(3).uniform(-0.2, 0.2, (len(si), 3)))])
    w = np.array([0.15])
    R, O = _pair(pkg, small, F.CATMULL_ROM, F.CLAMP)
    bare = K.pair(pkg, None, max_depth=6, scene=s)[0]                        # a context that never has keyframes
    for r in (R, bare):
        r.set_vertex_skin(vb, vw, nb, nw, N_BONES); r.set_vertex_morph(*targets)
    t = _time(2.25)
    first = _check_against_oracle(pkg, R, O, small, t, F.CATMULL_ROM, F.CLAMP, film=False)
    R.update_skin(BEND); bare.update_skin(BEND)
    K.assert_arrays(R, S.skin_vertices(s.vertex, vb, vw, BEND), S.skin_normals(s.normal, nb, nw, BEND))   # the skin's rest pose: the scene at ITS set-up
    K.assert_arrays(bare, *R.vertices())
    R.update_keyframes(t)                                                    # the keyframes again: what they gave the first time
    K.assert_same(K.state(pkg, R, film=False, arrays=True), first)
    R.update_morph(w); bare.update_morph(w)
    K.assert_arrays(R, M.morph_vertices(s.vertex, targets[0], w), M.morph_normals(s.normal, targets[1], w))
    K.assert_arrays(bare, *R.vertices())
    R.update_keyframes(t)
    K.assert_same(K.state(pkg, R, film=False, arrays=True), first)
    assert (R.keyframe_info().updates, R.skin_info().updates, R.morph_info().updates, R.transform_info().updates, R.update_info().updates) == (3, 1, 1, 0, 5)
    R.close(); O.close(); bare.close()


@pytest.mark.gpu
def test_counters_and_bookkeeping(pkg):
    small = True
    s = K.scene(pkg, small); nv = s.vertex.shape[0]; vf, nf = _frames(pkg, small)
    R, O = K.pair(pkg, None, max_depth=6, scene=s)
    base = R.info().device_bytes
    ki = R.keyframe_info()
    assert (ki.n_frames, ki.updates, ki.device_bytes, ki.last_ms) == (0, 0, 0, 0.0)
    stride = 8 * (3 * nv + 1)                                                # 3 n is odd: one double of padding per frame
    R.set_vertex_keyframes(vf, nf, START, FRAME_TIME, F.LINEAR, F.LOOP)
    assert R.info().device_bytes - base == R.keyframe_info().device_bytes == 2 * N_FRAMES * stride + 2 * 24 * nv
    R.set_vertex_keyframes(vf[:3], None)                                     # replaces: the old buffers are released, the normal frames included
    ki = R.keyframe_info()
    assert R.info().device_bytes - base == ki.device_bytes == 3 * stride + 2 * 24 * nv and (ki.n_frames, ki.interpolation, ki.wrap) == (3, F.LINEAR, F.CLAMP)
    R.set_vertex_keyframes(vf, nf, START, FRAME_TIME, F.LINEAR, F.LOOP)
    counts = lambda: (R.update_info().updates, R.keyframe_info().updates, R.transform_info().updates, R.skin_info().updates, R.morph_info().updates)
    assert counts() == (0, 0, 0, 0, 0)
    for r in (R, O):
        r.clear(); r.render(4, seed=5)
    film = R.read_accum(); rays = R.counters().rays
    R.update_keyframes(_time(0.5))
    assert counts() == (1, 1, 0, 0, 0)
    assert np.array_equal(bits(R.read_accum()), bits(film)) and R.counters().rays == rays                           # film and counters stay untouched
    R.update_keyframes(_time(1.0))                                           # on a keyframe: counted like any other call
    assert counts() == (2, 2, 0, 0, 0) and R.reproject_info().reprojections == 0
    R.update_keyframes_reproject(_time(1.75), feature_spp=4, feature_seed=3, max_history=16.0)
    assert counts() == (3, 3, 0, 0, 0) and R.reproject_info().reprojections == 1
    ki = R.keyframe_info(); ui = R.update_info()
    assert (ki.last_frame, ki.last_u, ki.last_time) == (1, 0.75, _time(1.75)) and 0 < ki.last_ms <= ui.last_update_ms
    R.close(); O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_camera", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_reprojection_follows_the_keyframes(pkg, mode, with_camera):
    small = True
    R, O = _pair(pkg, small, mode, F.LOOP)
    cam = pkg.scenes.Camera((0.62, 0.55, 2.25), (0.5, 0.45, 0.0), (0.0, 1.0, 0.0), 40.0, W, H) if with_camera else None
    t = _time(4.25)                                                          # the wrap-around segment
    v, n = _want(pkg, small, t, mode, F.LOOP)
    opts = dict(feature_spp=4, feature_seed=3, max_history=16.0)
    for r in (R, O):
        r.clear(); r.render(8, seed=5)
    R.update_keyframes_reproject(t, camera=cam, **opts)
    O.update_vertices_reproject(v, n, camera=cam, **opts)
    assert np.array_equal(bits(R.read_accum()), bits(O.read_accum()))
    ia, ib = R.reproject_info(), O.reproject_info()
    assert (ia.reprojections, ia.pixels_reused) == (ib.reprojections, ib.pixels_reused) == (1, ib.pixels_reused) and ia.pixels_reused > 0.5 * W * H
    assert np.array_equal(bits(R.features()), bits(O.features()))
    K.assert_arrays(R, v, n)
    K.assert_same(K.state(pkg, R, film=False), K.state(pkg, O, film=False))
    plain = K.pair(pkg, lambda r: _set(pkg, r, small, mode, F.LOOP), max_depth=6, scene=K.scene(pkg, small))[0]
    plain.update_keyframes(t)
    if cam is not None:
        plain.set_camera(cam)
    K.assert_same(K.state(pkg, R, film=False, arrays=True), K.state(pkg, plain, film=False, arrays=True))        # arrays and trees: the plain form's
    R.close(); O.close(); plain.close()


@pytest.mark.gpu
def test_clone_and_rebuild_carry_the_keyframes(pkg):
    small = True
    R, O = _pair(pkg, small, F.CATMULL_ROM, F.LOOP)
    R.update_keyframes(_time(0.5))
    clone = R.clone()
    ki = clone.keyframe_info()
    assert (ki.n_frames, ki.interpolation, ki.wrap, ki.updates, ki.device_bytes) == (N_FRAMES, F.CATMULL_ROM, F.LOOP, 0, R.keyframe_info().device_bytes)
    assert clone.info().device_bytes == R.info().device_bytes              # (neither has rendered yet: no pools)
    K.assert_arrays(clone, *_want(pkg, small, _time(0.5), F.CATMULL_ROM, F.LOOP))
    R.update_keyframes(_time(3.5)); clone.update_keyframes(_time(3.5))       # the clone's next update equals the source's
    K.assert_same(K.state(pkg, clone, arrays=True), K.state(pkg, R, arrays=True))
    _check_against_oracle(pkg, clone, O, small, _time(4.75), F.CATMULL_ROM, F.LOOP, film=False)
    K.assert_arrays(R, *_want(pkg, small, _time(3.5), F.CATMULL_ROM, F.LOOP))   # the source did not move with its clone
    # a rebuild leaves the set alone: the next update is that of a fresh context on the same frames, put on the same pose and rebuilt the same way
    for builder in (pkg.REBUILD_HOST, pkg.REBUILD_DEVICE):
        fresh = K.pair(pkg, lambda r: _set(pkg, r, small, F.CATMULL_ROM, F.LOOP), max_depth=6, scene=K.scene(pkg, small))[0]
        fresh.update_vertices(*R.vertices())
        R.rebuild(builder); fresh.rebuild(builder); O.update_vertices(*R.vertices()); O.rebuild(builder)
        assert R.keyframe_info().n_frames == N_FRAMES
        t = _time(1.25 if builder == pkg.REBUILD_HOST else 2.5)
        R.update_keyframes(t); fresh.update_keyframes(t)
        K.assert_same(K.state(pkg, R, arrays=True), K.state(pkg, fresh, arrays=True))
        _check_against_oracle(pkg, R, O, small, t, F.CATMULL_ROM, F.LOOP, film=False)
        fresh.close()
    clone.close(); R.close(); O.close()


@pytest.mark.gpu
def test_setting_again_replaces_frames_and_options(pkg):
    small = True
    vf, nf = _frames(pkg, small)
    R, O = _pair(pkg, small, F.LINEAR, F.CLAMP)
    R.update_keyframes(_time(1.5))
    other = (vf[::-1][:4].copy(), nf[::-1][:4].copy())                       # four frames, in another order, on another clock
    R.set_vertex_keyframes(other[0], other[1], start_time=-1.5, frame_time=2.0, interpolation=F.CATMULL_ROM, wrap=F.LOOP)
    K.assert_arrays(R, *_want(pkg, small, _time(1.5), F.LINEAR, F.CLAMP))    # setting moves nothing
    ki = R.keyframe_info()
    assert (ki.n_frames, ki.interpolation, ki.wrap, ki.updates) == (4, F.CATMULL_ROM, F.LOOP, 1)
    for t in (2.0, -1.5 + 2.0 * 3.5, -1.5 - 8.0 + 0.5):
        _check_against_oracle(pkg, R, O, small, t, F.CATMULL_ROM, F.LOOP, film=False, frames=other, start=-1.5, frame_time=2.0)
    assert R.keyframe_info().last_frame == 0 and R.keyframe_info().last_u == 0.25
    R.close(); O.close()


@pytest.mark.gpu
def test_update_between_renders_without_a_sync(pkg):
    small = True
    R, O = _pair(pkg, small, F.CATMULL_ROM, F.LOOP)
    _set(pkg, O, small, F.CATMULL_ROM, F.LOOP)
    R.clear()
    R.render(4, seed=9, first_sample=0); R.update_keyframes(_time(0.5)); R.render(4, seed=9, first_sample=4)      # nothing in between
    R.update_keyframes(_time(3.25)); R.update_keyframes(_time(2.0)); R.update_keyframes(_time(4.5))              # back-to-back calls keep their order
    R.render(2, seed=9, first_sample=8)
    got = R.read_accum()
    O.clear()
    O.render(4, seed=9, first_sample=0); O.sync(); O.update_keyframes(_time(0.5)); O.sync(); O.render(4, seed=9, first_sample=4); O.sync()
    for x in (3.25, 2.0, 4.5):
        O.update_keyframes(_time(x)); O.sync()
    O.render(2, seed=9, first_sample=8); O.sync()
    assert np.array_equal(bits(got), bits(O.read_accum())) and np.all(got[..., 3] == 10)
    K.assert_arrays(R, *_want(pkg, small, _time(4.5), F.CATMULL_ROM, F.LOOP))
    R.close(); O.close()


@pytest.mark.gpu
def test_keyframe_refusals(pkg):
    small = True
    s = K.scene(pkg, small); n = s.vertex.shape[0]
    vf, nf = _frames(pkg, small)
    plain = pkg.Renderer(s, max_depth=6, flags=pkg.FLAG_DETERMINISTIC)
    for call in (lambda: plain.set_vertex_keyframes(vf, nf), lambda: plain.update_keyframes(0.5), lambda: plain.update_keyframes_reproject(0.5),
                 lambda: plain.keyframe_info()):
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % UNSUPPORTED in str(e.value)
    plain.close()
    R = pkg.Renderer(s, max_depth=6, flags=FLAGS(pkg))
    o, d = K.rays(pkg)
    film = render_film(R, 4, 5); trace = R.probe_trace4(o, d); arrays = R.vertices(); bytes0 = R.info().device_bytes
    expect = {"n_frames": 0, "bytes": 0, "mode": 0, "wrap": 0}

    def unchanged():
        ki = R.keyframe_info()
        assert R.update_info().updates == 0 and R.reproject_info().reprojections == 0
        assert (ki.n_frames, ki.updates, ki.device_bytes, ki.interpolation, ki.wrap, ki.last_ms) == (expect["n_frames"], 0, expect["bytes"], expect["mode"], expect["wrap"], 0.0)
        assert R.info().device_bytes == bytes0 + expect["bytes"]
        assert np.array_equal(bits(render_film(R, 4, 5)), bits(film))
        for x, y in zip(trace, R.probe_trace4(o, d)):
            assert np.array_equal(bits(x), bits(y))
        for x, y in zip(arrays, R.vertices()):
            assert np.array_equal(bits(x), bits(y))

    def refused(call, name, status=INVALID):
        with pytest.raises(pkg.McptError) as e:
            call()
        assert "status %d" % status in str(e.value) and name in str(e.value)
        unchanged()
        return str(e.value)

    # ---- mcpt_update_keyframes before any set-up; a time that is not finite is judged first
    assert "no keyframes are set" in refused(lambda: R.update_keyframes(0.5), "mcpt_update_keyframes:")
    assert "no keyframes are set" in refused(lambda: R.update_keyframes_reproject(0.5), "mcpt_update_keyframes_reproject:")
    assert "not finite" in refused(lambda: R.update_keyframes(math.nan), "mcpt_update_keyframes:")
    # ---- mcpt_set_vertex_keyframes
    SET = "mcpt_set_vertex_keyframes:"
    used = T.used_vertices(s)
    iu = int(np.flatnonzero(used)[11]); idle = int(np.flatnonzero(~used)[0])

    def edit(a, k, i, c, x):
        a = a.copy(); a[k, i, c] = x
        return a

    lib = R.lib
    opts = pkg.KeyframeOpts(); opts.struct_size = C.sizeof(pkg.KeyframeOpts); opts.frame_time = 1.0
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def raw_set(v=vf, n_vertex=n, nr=nf, n_normal=n, n_frames=N_FRAMES, o=opts):
        st = lib.mcpt_set_vertex_keyframes(R.ctx, None if v is None else vp(v), n_vertex, None if nr is None else vp(nr), n_normal, n_frames, None if o is None else C.byref(o))
        return st, (lib.mcpt_last_error() or b"").decode()

    def opts_with(**fields):
        c = pkg.KeyframeOpts(); C.memmove(C.byref(c), C.byref(opts), C.sizeof(c))
        for k, x in fields.items():
            setattr(c, k, x)
        return c

    for kw, word in ((dict(v=None), "null vertex frames"), (dict(n_vertex=n - 1), "differ from the scene's"), (dict(n_normal=n + 1), "differ from the scene's"),
                     (dict(nr=None, n_normal=n - 1), "differ from the scene's"),
                     (dict(o=opts_with(struct_size=C.sizeof(pkg.KeyframeOpts) - 4)), "struct_size"), (dict(o=opts_with(struct_size=0)), "struct_size"),
                     (dict(n_frames=1), "n_frames"), (dict(n_frames=0), "n_frames"), (dict(n_frames=65537), "n_frames"), (dict(n_frames=2 ** 32 - 1), "n_frames"),
                     # precedence, as the header lists it
                     (dict(v=None, n_vertex=n - 1), "null vertex frames"), (dict(n_vertex=n - 1, o=opts_with(struct_size=0)), "differ from the scene's"),
                     (dict(o=opts_with(struct_size=0, interpolation=7)), "struct_size"), (dict(o=opts_with(interpolation=2, wrap=2)), "interpolation"),
                     (dict(o=opts_with(wrap=2), n_frames=1), "wrap"), (dict(n_frames=1, o=opts_with(start_time=math.nan)), "n_frames"),
                     (dict(o=opts_with(start_time=math.inf, frame_time=0.0)), "start_time"), (dict(v=edit(vf, 0, iu, 0, math.nan), o=opts_with(frame_time=-1.0)), "frame_time"),
                     (dict(v=edit(vf, 4, iu, 2, math.inf), nr=edit(nf, 0, 0, 0, math.nan)), "coordinate"),
                     (dict(v=edit(vf, 1, iu, 1, 1e18), nr=edit(nf, 2, 3, 1, -math.inf)), "a component is not finite")):
        st, msg = raw_set(**kw)
        assert st == INVALID and msg.startswith(SET) and word in msg, (kw.keys(), msg)
    unchanged()
    refused(lambda: R.set_vertex_keyframes(vf, nf, interpolation=2), SET); refused(lambda: R.set_vertex_keyframes(vf, nf, wrap=5), SET)
    refused(lambda: R.set_vertex_keyframes(vf[:1], nf[:1]), SET); refused(lambda: R.set_vertex_keyframes(vf[:, :-1], nf), SET); refused(lambda: R.set_vertex_keyframes(vf, nf[:, :-1]), SET)
    for x in (math.nan, math.inf, -math.inf):
        refused(lambda: R.set_vertex_keyframes(vf, nf, start_time=x), SET); refused(lambda: R.set_vertex_keyframes(vf, nf, frame_time=x), SET)
    refused(lambda: R.set_vertex_keyframes(vf, nf, frame_time=0.0), SET); refused(lambda: R.set_vertex_keyframes(vf, nf, frame_time=-0.25), SET)
    for x in (math.nan, math.inf, -math.inf, 1.0000001e18):
        assert not F.accepts(edit(vf, 3, iu, 1, x), nf, used, n, n)
        assert "frame 3, vertex %d" % iu in refused(lambda: R.set_vertex_keyframes(edit(vf, 3, iu, 1, x), nf), SET)
    for x in (math.nan, math.inf, -math.inf):
        assert not F.accepts(vf, edit(nf, 4, 5, 2, x), used, n, n)
        assert "frame 4, normal 5" in refused(lambda: R.set_vertex_keyframes(vf, edit(nf, 4, 5, 2, x)), SET)
    # the reach alone: every coordinate passes its own rule
    assert "conservative" in refused(lambda: R.set_vertex_keyframes(edit(vf, 0, iu, 0, 1e18), nf), SET)
    assert "conservative" in refused(lambda: R.set_vertex_keyframes(edit(vf, 0, iu, 0, -0.9e18), nf, interpolation=F.CATMULL_ROM), SET)
    assert F.accepts(edit(vf, 0, iu, 0, -0.9e18), nf, used, n, n) and not F.accepts(edit(vf, 0, iu, 0, -0.9e18), nf, used, n, n, interpolation=F.CATMULL_ROM)
    # accepted; then a refused replacement leaves the set that is there
    R.set_vertex_keyframes(vf, None)
    R.set_vertex_keyframes(vf, nf, START, FRAME_TIME, F.CATMULL_ROM, F.LOOP)
    expect.update(n_frames=N_FRAMES, bytes=2 * N_FRAMES * 8 * (3 * n + 1) + 2 * 24 * n, mode=F.CATMULL_ROM, wrap=F.LOOP)
    unchanged()
    refused(lambda: R.set_vertex_keyframes(vf[:1], nf[:1]), SET); refused(lambda: R.set_vertex_keyframes(edit(vf, 3, iu, 1, math.nan), None), SET)
    refused(lambda: R.set_vertex_keyframes(vf, nf, frame_time=0.0), SET)
    # ---- mcpt_update_keyframes and _reproject: the time, then the camera, then the options
    for x in (math.nan, math.inf, -math.inf):
        assert "not finite" in refused(lambda: R.update_keyframes(x), "mcpt_update_keyframes:")
        assert "not finite" in refused(lambda: R.update_keyframes_reproject(x), "mcpt_update_keyframes_reproject:")
    cam = s.camera
    bad_cam = pkg.scenes.Camera(cam.eye, cam.eye, cam.up, cam.fovy, W, H)
    REP = "mcpt_update_keyframes_reproject"
    refused(lambda: R.update_keyframes_reproject(0.5, camera=pkg.scenes.Camera(cam.eye, cam.lookat, cam.up, cam.fovy, W + 1, H)), REP)
    refused(lambda: R.update_keyframes_reproject(0.5, camera=bad_cam), REP)
    refused(lambda: R.update_keyframes_reproject(0.5, feature_spp=65), REP); refused(lambda: R.update_keyframes_reproject(0.5, max_history=0.5), REP)
    assert "eye == lookat" in refused(lambda: R.update_keyframes_reproject(0.5, camera=bad_cam, feature_spp=65), REP)         # a bad camera before bad options
    assert "not finite" in refused(lambda: R.update_keyframes_reproject(math.nan, camera=bad_cam, feature_spp=65), REP)      # a bad time before a bad camera
    R.validate_trees()
    R.update_keyframes(_time(1.5))                                           # and the context still works
    K.assert_arrays(R, *_want(pkg, small, _time(1.5), F.CATMULL_ROM, F.LOOP))
    assert R.update_info().updates == 1 and R.keyframe_info().updates == 1
    # a vertex that no face uses is not judged: a far-away value there is accepted and played
    far = edit(vf, 2, idle, 0, 2e18)
    assert F.accepts(far, nf, used, n, n)
    R.set_vertex_keyframes(far, nf, START, FRAME_TIME)
    R.update_keyframes(_time(2.0))
    K.assert_arrays(R, far[2], nf[2])
    R.validate_trees()
    R.close()


@pytest.mark.gpu
def test_facade_keyframes(pkg, tmp_path):
    exe = kit.build_facade("facade_keyframes.cpp", tmp_path)
    a = pkg.scenes.cornell_box(44, 30, sphere_lon=24, sphere_lat=12)
    obj = a.write(str(tmp_path / "a"))
    # the program reads the 9-digit text of the file: the same numbers scenes.py keeps (SceneData is rounded through that text form)
    part = np.zeros(a.vertex.shape[0], bool); part[np.unique(a.face[a.face[:, 0, 3] == SPHERE][:, :, 0])] = True
    ni = np.unique(a.face[a.face[:, 0, 3] == SPHERE][:, :, 1])
    vf = np.repeat(a.vertex[None], 4, 0); nf = np.repeat(a.normal[None], 4, 0)
    p = a.vertex[part]
    for k in range(4):
        vf[k][part] = p + LIFT + 0.02 * (k + 1) * np.stack([np.sin(9.0 * p[:, 1] + k), np.sin(7.0 * p[:, 2]), np.sin(8.0 * p[:, 0] - k)], 1)
        q = a.normal[ni] + 0.1 * k
        nf[k][ni] = q / np.linalg.norm(q, axis=1, keepdims=True)
    start, ft, t1, t2 = 2.0, 0.5, 2.625, 3.75                               # segment 1 at u = 0.25; segment 3 -> 0 at u = 0.5
    mode, wrap = F.CATMULL_ROM, F.LOOP
    want = [F.play_vertices(vf, t1, start, ft, mode, wrap), F.play_normals(nf, t1, start, ft, mode, wrap),
            F.play_vertices(vf, t2, start, ft, mode, wrap), F.play_normals(nf, t2, start, ft, mode, wrap)]
    assert F.segment(t1, start, ft, 4, wrap) == (1, 0.25) and F.segment(t2, start, ft, 4, wrap) == (3, 0.5)
    names = ["vf", "nf", "v1", "n1", "v2", "n2"]
    for arr, name in zip([vf, nf] + want, names):
        np.ascontiguousarray(arr, np.float64).tofile(str(tmp_path / (name + ".bin")))
    ins = [str(tmp_path / (x + ".bin")) for x in names]
    outs = [str(tmp_path / x) for x in ("kf.bin", "upd.bin", "kf_rp.bin", "upd_rp.bin")]
    k = 4
    line = kit.run_facade(exe, [obj, str(k), "4", str(mode), str(wrap), repr(start), repr(ft), repr(t1), repr(t2)] + ins + outs)
    w_, h_ = int(line[0]), int(line[1])
    assert (w_, h_, int(line[2])) == (44, 30, k)
    kf, upd, kf_rp, upd_rp = [np.fromfile(x, np.float32).reshape(h_, w_, 4) for x in outs]
    assert np.all(kf[..., 3] == k) and kf[..., :3].sum() > 0                 # the picture started again and ends at k samples
    assert np.array_equal(bits(kf), bits(upd))                             # the time on the device = the restated arrays through update()
    assert np.array_equal(bits(kf_rp), bits(upd_rp)) and not np.array_equal(kf_rp, kf)      # and so with the film carried over
    assert np.all(kf_rp[..., 3] >= 1) and np.all(kf_rp[..., 3] <= 5) and (kf_rp[..., 3] > 1).mean() > 0.5   # history capped at 4, plus the new frame


def _write_sequence(pkg, directory, count=5, faces=None, drop_vertex=False):
    """A `count`-file OBJ sequence of S-cornell-small at 40 x 32 written by the package's scene writer -- frame_0000.obj ... -- whose sphere is
    lifted off the floor and displaced by a different smooth offset per frame (walls and lamp fixed: the room's bounding box stays).  (the printf
    pattern, the paths.)"""
    base = pkg.scenes.cornell_box_small(40, 32)
    part = np.zeros(base.vertex.shape[0], bool); part[np.unique(base.face[base.face[:, 0, 3] == SPHERE][:, :, 0])] = True
    p = base.vertex[part]
    paths = []
    for j in range(count):
        v = base.vertex.copy()
        v[part] = p + LIFT + 0.015 * j * np.stack([np.sin(9.0 * p[:, 1] + j), np.sin(7.0 * p[:, 2] + 2 * j), np.sin(8.0 * p[:, 0] - j)], 1)
        face = base.face if faces is None or j != count - 1 else faces(base.face)
        if drop_vertex and j == count - 1:
            v = np.concatenate([v, v[:1]])                                   # one vertex more than the scene has (no face uses it)
        frame = pkg.scenes.SceneData("frame_%04d" % j, v, base.normal, base.texcoord, face, base.materials, base.camera, dict(base.meta))
        paths.append(frame.write(str(directory)))
    return str(directory / "frame_%04d.obj"), paths


COMMON = ["--spp", "4", "--depth", "5", "--deterministic"]


@pytest.fixture(scope="module")
def played(pkg, tmp_path_factory):
    """The five-file sequence, written once, and the five turntable frames mcpt_cli plays from it with --slowdown 1, rendered once and shared:
    (pattern, paths, the frames' PNG bytes)."""
    d = tmp_path_factory.mktemp("sequence")
    pattern, paths = _write_sequence(pkg, d / "seq")
    out = str(d / "played")
    p = kit.run_cli([paths[0], "--turntable", "5", "--out", out] + COMMON + ["--sequence", pattern, "5", "--slowdown", "1"])
    assert p.returncode == 0, p.stderr[-2000:]
    frames = kit.turntable_frames(out, 5)
    assert len(set(frames)) == 5
    return pattern, paths, frames


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(5))
def test_cli_sequence_frame_is_that_file_alone(played, tmp_path, j):
    """--slowdown 1: turntable frame j is OBJ j alone, seen from turntable frame j's camera."""
    pattern, paths, frames = played
    alone = str(tmp_path / "alone")
    q = kit.run_cli([paths[j], "--turntable", "5", "--out", alone] + COMMON)
    assert q.returncode == 0, q.stderr[-2000:]
    assert kit.turntable_frames(alone, 5)[j] == frames[j]


@pytest.mark.gpu
def test_cli_sequence_slowed_down_and_smooth(played, tmp_path):
    """--slowdown 2 --smooth: the even frames are the files (a spline passes through its keys), the odd ones lie between and differ from both
    neighbours."""
    pattern, paths, frames = played
    out = str(tmp_path / "slow")
    p = kit.run_cli([paths[0], "--turntable", "9", "--out", out] + COMMON + ["--sequence", pattern, "5", "--slowdown", "2", "--smooth"])
    assert p.returncode == 0, p.stderr[-2000:]
    slow = kit.turntable_frames(out, 9)
    for j in range(1, 9, 2):
        assert slow[j] != slow[j - 1] and slow[j] != slow[j + 1]


@pytest.mark.gpu
def test_cli_sequence_combines_with_reproject_auto_normals_and_rebuild(played, tmp_path):
    pattern, paths, frames = played
    p = kit.run_cli([paths[0], "--turntable", "3", "--out", str(tmp_path / "all")] + COMMON + ["--sequence", pattern, "5", "--reproject", "8", "--auto-normals", "--rebuild-above", "1.0"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(set(kit.turntable_frames(str(tmp_path / "all"), 3))) == 3


@pytest.mark.gpu
def test_cli_sequence_clean_errors(pkg, played, tmp_path):
    pattern, paths, _ = played
    base = [paths[0], "--turntable", "3", "--spp", "2", "--out", str(tmp_path / "img")]

    def error(args):
        q = kit.run_cli(args)
        assert q.returncode == 2 and "--sequence" in q.stderr and "Error:" in q.stderr, (args, q.returncode, q.stderr[-500:])
        return q.stderr

    error(base + ["--sequence", pattern, "6"])                               # frame 5 does not exist
    assert "did not load" in error(base + ["--sequence", str(tmp_path / "nothing_%d.obj"), "2"])
    error(base + ["--sequence", pattern, "1"]); error(base + ["--sequence", pattern, "0"]); error(base + ["--sequence", pattern])
    for s_ in ("0", "-1", "nan", "inf"):
        error(base + ["--sequence", pattern, "5", "--slowdown", s_])
    for bad in (paths[0], pattern.replace("%04d", "%s"), pattern.replace("%04d", "%d_%d"), pattern.replace("%04d", "%04x")):
        assert "conversion" in error(base + ["--sequence", bad, "5"])
    for other in (["--wobble", "0.01"], ["--spin", "glossy"], ["--bend", "glossy", "25"], ["--swell", "glossy", "0.2"]):
        error(base + ["--sequence", pattern, "5"] + other)
    error([paths[0], "--sequence", pattern, "5"])                            # without --turntable
    error(base + ["--slowdown", "2"]); error(base + ["--smooth"])            # without --sequence
    # a frame with other faces, and one with another vertex count
    swapped, _ = _write_sequence(pkg, tmp_path / "faces", faces=lambda f: np.concatenate([f[:-1], f[-1:, ::-1]]))
    assert "faces" in error(base + ["--sequence", swapped, "5"])
    longer, _ = _write_sequence(pkg, tmp_path / "count", drop_vertex=True)
    assert "vertices" in error(base + ["--sequence", longer, "5"])
