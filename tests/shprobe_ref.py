"""Plain numpy restatement of the light-probe stage (csrc/shprobe.hip) and the error model of tests/test_shprobe_ref.py
(CPU) and tests/test_shprobe.py (device).  Written from the definitions in include/mcpt.h and DESIGN.md section 28.

`rays` takes per item its direction slot j = item & 63 and the two fp32 random numbers of block 0 and works in ONE floating-point type after
that: np.float64 restates the device, one rounding per operation in the device's operation order; np.longdouble is the same formulas with 11
more bits.  `basis`, `project` and `resolve` are fp32, one rounding per operation, and `tree_sum` is the reduction the projection kernel's wave
performs -- s[j] + s[j + 32], then + 16, ... + 1 --, so they give the device's bits.

Error model, as sections 25's and 27's.  S is the worst |float64 restatement - longdouble restatement| over every (unrounded) direction
component of every slot under every pair of bake_ref.XI_SET and a random tail, in units of 2^-52 (1 + |value|): what the formulas themselves
lose in float64.  tests/test_shprobe_ref.py measures it; the device is allowed S_BOUND = 4 S rounded up to a power of two, a stand-in for its
sincos / sqrt / division chain.  A direction component is rounded to fp32 on the device: it gets half an fp32 ulp of the reference on top.  (An
origin is the host's world - centre, one subtraction, and is held to equality.)

    S measured on the CPU: 1.97 (slot 59, the y component), 4 S = 7.88, so S_BOUND = 8
    the device on an MI355X: see DESIGN.md section 28
"""
from __future__ import annotations

import numpy as np

from tests import bake_ref

F32 = np.float32
PI = 3.14159265358979323846
DIRS = 64
S_CPU = 1.97                                                # measured by tests/test_shprobe_ref.py::test_float64_slack
S_BOUND = 8.0
SEED = 20280

# the nine constants, rounded to fp32 first
C0, C1, C2, C6, C8 = (F32(x) for x in (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396))
BAND = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])                # l of k = l (l + 1) + m
BAND_FACTOR = np.array([F32(PI), F32(2.0 * PI / 3.0), F32(PI / 4.0)], F32)


def slot_uv(slot, xi, T=np.float64):
    """(u, v) in type T: the stratified pair of slot j = jx + 8 jy under the block's first two numbers."""
    slot = np.asarray(slot).reshape(-1).astype(np.int64); xi = np.asarray(xi, F32).reshape(-1, 2)
    u = ((slot & 7).astype(T) + xi[:, 0].astype(T)) / T(8.0)
    v = ((slot >> 3).astype(T) + xi[:, 1].astype(T)) / T(8.0)
    return u, v


def rays(slot, xi, T=np.float64):
    """(N, 3) directions in type T: what the device rounds to fp32."""
    u, v = slot_uv(slot, xi, T)
    z = T(1.0) - T(2.0) * u
    r = T(2.0) * np.sqrt(u * (T(1.0) - u))
    phi = (T(2.0) * T(PI)) * v
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)


def xi_cases(n, seed=SEED):
    """(n, 2) fp32 numbers of block 0: every pair of bake_ref.XI_SET first, then random k 2^-24."""
    return bake_ref.xi_cases(n, seed)


def dir_ratio(got_d, ref_d, s_bound=S_BOUND):
    """Per ray the worst |difference| / bound over the three components: half an fp32 ulp of the reference plus s_bound slack."""
    ref_d = np.asarray(ref_d, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.abs(np.asarray(got_d, np.float64) - ref_d) / (bake_ref.half_ulp32(ref_d) + s_bound * bake_ref.slack(ref_d))
    return np.where(np.isnan(r), np.inf, r).max(1)


def slack_used(got_d, ref_d):
    """What a set of directions needs of the float64 slack beyond its half fp32 ulp, in the slack's units.  A figure to print, not a check."""
    ref_d = np.asarray(ref_d, np.float64)
    return float((np.maximum(np.abs(np.asarray(got_d, np.float64) - ref_d) - bake_ref.half_ulp32(ref_d), 0.0) / bake_ref.slack(ref_d)).max())


def basis(d):
    """(N, 9) fp32: the real spherical harmonics of bands 0 .. 2 at the fp32 directions d, k = l (l + 1) + m, one rounding per operation."""
    d = np.asarray(d).astype(F32).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    one, three = F32(1.0), F32(3.0)
    return np.stack([np.full(x.shape, C0, F32), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C6 * (three * (z * z) - one), C2 * (x * z), C8 * ((x * x) - (y * y))], -1).astype(F32)


def tree_sum(t):
    """The wave's sum over axis 0 (64 entries) of fp32 `t`, in the kernel's tree: s_6 = t, s_(m-1)[j] = s_m[j] + s_m[j + 2^(m-1)], the result s_0[0]."""
    s = np.asarray(t, F32)
    assert s.shape[0] == DIRS
    while s.shape[0] > 1:
        h = s.shape[0] // 2
        s = (s[:h] + s[h:]).astype(F32)
    return s[0]


def project(film, d):
    """(n, 3, 9) fp32: per probe the pass's 27 sums.  film: (64 n, >= 3) fp32 L per item (a component that is not finite counts as 0), d: (64 n, 3)
    directions holding fp32 values."""
    L = np.asarray(film, F32).reshape(-1, np.asarray(film).shape[-1])[:, :3]
    L = np.where(np.isfinite(L), L, F32(0.0)).astype(F32)
    Y = basis(d)
    n = L.shape[0] // DIRS
    with np.errstate(over="ignore", invalid="ignore"):
        t = (L[:, :, None] * Y[:, None, :]).astype(F32).reshape(n, DIRS, 3, 9)
        return np.stack([tree_sum(t[p]) for p in range(n)]) if n else np.zeros((0, 3, 9), F32)


def resolve(acc, rays_count, irradiance=False):
    """(n, 3, 9) fp32: kf acc with kf = float(4 pi) / float(rays), times the band's factor for irradiance; 0 where rays == 0."""
    acc = np.asarray(acc, F32).reshape(-1, 3, 9); cnt = np.asarray(rays_count).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        kf = F32(4.0 * PI) / cnt.astype(F32)
        out = (kf[:, None, None] * acc).astype(F32)
    out = np.where((cnt == 0)[:, None, None], F32(0.0), out).astype(F32)
    if irradiance:
        with np.errstate(over="ignore", invalid="ignore"):
            out = (BAND_FACTOR[BAND][None, None, :] * out).astype(F32)
    return out


def basis64(n):
    """(N, 9) float64: the same nine functions at unit vectors n, in float64 (mcpt_sh_eval's formulas)."""
    n = np.asarray(n, np.float64).reshape(-1, 3)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    c1, c2 = 0.4886025119029199, 1.0925484305920792
    return np.stack([np.full(x.shape, 0.28209479177387814), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), 0.31539156525252005 * (3.0 * (z * z) - 1.0), c2 * (x * z),
                     0.5462742152960396 * ((x * x) - (y * y))], -1)


def evaluate(coeffs, normal):
    """(N, 3) float64: mcpt_sh_eval's formula -- the normal normalised, the sum over k in ascending order; 0 for a normal of length 0 or not finite."""
    c = np.asarray(coeffs, F32).reshape(-1, 3, 9).astype(np.float64); n = np.broadcast_to(np.asarray(normal, np.float64).reshape(-1, 3), (c.shape[0], 3))
    with np.errstate(all="ignore"):
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = (length > 0) & np.isfinite(length)
        Y = basis64(n / np.where(ok, length, 1.0)[:, None])
        s = np.zeros((c.shape[0], 3))
        for k in range(9):
            s = s + c[:, :, k] * Y[:, k:k + 1]
    return np.where(ok[:, None], s, 0.0)


def grid(lo, hi, nx, ny, nz):
    """(nx ny nz, 3) float64: mcpt_sh_grid's cell centres, x fastest."""
    lo = np.asarray(lo, np.float64); hi = np.asarray(hi, np.float64)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cell = np.stack([i.ravel(), j.ravel(), k.ravel()], -1).astype(np.float64)
    return lo[None] + ((cell + 0.5) / np.array([nx, ny, nz], np.float64)[None]) * (hi - lo)[None]
