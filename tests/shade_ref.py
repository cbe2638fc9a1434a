"""A plain restatement of the BSDF of csrc/pt_device.h (make_bsdf, bsdf_eval, bsdf_sample) in numpy, the error model its comparisons use, and
the deliberately awkward inputs of the BSDF and light-sampling edge tests (tests/test_shade_ref.py on the CPU, tests/test_shade_edges.py on the
device).  Written from the behaviour documented in pt_device.h and oracle/mcpt_oracle.cpp.

The restatement.  `bsdf_ref` takes inputs that are fp32 values (anything else is rounded to fp32 on entry, as the probe does) and works in
float64 by default: every result is then exact to ~1e-15 and a difference from it is the ERROR OF THE SIDE UNDER TEST, not an input rounding.
It follows the device's definitions: the truncated pi 3.1415926f, the luminance weights as fp32 constants, the mirror lobe for Ns >= 10000 with
any nonzero Ks, the energy rescale when !(max(kd + ks) < 1), the frame switch at |n.x| > 0.9f, `n` used as given.  Every step keeps the
operation order of oracle/mcpt_oracle.cpp (dot = (x*x + y*y) + z*z, normalize = v * (1 / sqrt(dot)), theta = acos(1 - 2 xi2) / 2 for the
diffuse lobe), so `dtype=np.float32` replays the reference's own fp32 arithmetic: that mode is what pins the FORMULAS to the recorded answers of
the real reference at 1e-6 (test_shade_ref.py); float64 is the same code at higher precision.

The error model.  For an output q of a case with exponent Ns the allowed difference is

    K * 2^-23 * (|q| * (1 + Ns * c_q) + s_q)   +   |y * log2(x)| * 2^-22 * |q|   +   K * D_q

c_q = 1 for the outputs that hold H.z^Ns (fx, f and both pdfs of a Blinn-Phong material), else 0: Ns * c_q is the conditioning of t -> t^Ns, one
ulp of H.z is Ns ulps of the result in any fp32 arithmetic.  s_q is the natural scale of the output: 1 for directions and pdfs, max(kd, ks)/pi
(after the energy rescale) for fx and f.  The second term is pow_pos's own error and goes to the outputs that contain pow_pos(x, y): H.z^Ns, and
xi2^(1/(Ns+1)) in the direction of a Phong pick (whose exponent is at most 1, so that direction gets c_q = 0).  D_q is the one conditioning the
first term cannot express, and it is the reference formula's, not an implementation's: Specular::Sample takes sin(theta) = sqrt(1 - cos^2(theta))
with cos(theta) = xi2^(1/(Ns+1)) held in fp32, so half an ulp of a cosine near 1 (2^-25) moves the sine by 2^-25 / sin(theta), and below
sin(theta) = 2^-12 the subtraction quantises (at xi2 = 1 - 2^-24, Ns = 10 the true sine is 1.0e-4 and fp32 returns 0 or 3.5e-4; the fp32 oracle is
2e-4 off in the direction there).  D_q = 2^-23 / max(sin(theta), 2^-12) for the direction of a Phong pick, and that times w_diff / pi for the
sample's pdf, whose diffuse companion is wi.z / pi * w_diff.  Without D_q the oracle would need K = 1600 for that one family (xi_edges) and the
bound would say nothing anywhere else; test_shade_ref.py prints that figure beside the measured K.

K is measured, not chosen: K_ORACLE is the smallest K (rounded up) at which the fp32 ORACLE -- the reference's own arithmetic with correctly
rounded libm -- stays inside the model against the float64 restatement on `bsdf_edge_cases(EDGE_SEED)`, outside `marginal`.  Measured 1.57 (worst
families grazing_axis and frame_switch, a sampled direction); test_shade_ref.py prints it per family and asserts measured <= K_ORACLE = 2.  The
DEVICE is given DEVICE_FACTOR = 4 times that: it replaces about four correctly rounded operations per output (divide, 1/sqrt, pow, sin/cos) by
operations of 1 ulp or worse (v_rcp_f32, v_rsq_f32, v_exp_f32(y * v_log_f32(x)), __sinf / __cosf).  On an MI355X the device's worst ratio to the
oracle's budget is 1.97 (family grazing_axis; every family between 0.77 and 1.97), so it needs half of what it is given.  The bound on a sampled
direction: 4 K 2^-23 (|q| + 1) <= 1.91e-6 for a diffuse or mirror pick (device worst 5.2e-7: __sinf / __cosf near 2 pi included), that plus
9.5e-7 / sin(theta) for a Phong pick (<= 9.7e-5 where sin(theta) >= 0.01; device worst 4.6e-6).

`marginal` marks the cases whose DISCRETE outcome (mirror flag, failed or not, lobe) legitimately hangs on fp32 rounding, decided by the restatement
alone: |m_wo.z| (or the evaluated direction's local z) below 4 ulp of its fp32 computation -- 4 * 2^-24 * sum |a_k b_k| over the three products of
the dot product, so an exact zero from an axis-aligned normal, computed without any rounding, is NOT marginal --; a sampled local |wi.z| below 1e-6;
a lobe margin |w_spec - xi * total| of at most 2^-22.  Not marginal: Ns exactly at the mirror threshold (an fp32 comparison of an input), and the
exact tie w_spec == xi * total of a grey material with kd == ks at xi = 0.5 (both weights come from the same operations on the same numbers, so they
are bit-equal and 0.5 * (w + w) == w in every binary arithmetic).  The generator keeps the marginal share at or below 1 %.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

F32 = np.float32
PI_F = F32(3.1415926)                                       # PT_PI: the reference's truncated pi
LUM = (F32(0.212671), F32(0.715160), F32(0.072169))
MIRROR_NS = 10000.0
FRAME_SWITCH = F32(0.9)
EPS24 = 2.0 ** -24
ONE_BELOW = F32(1.0 - EPS24)                                # the largest random number the generator can return
EDGE_SEED = 20261
K_ORACLE = 2.0                                              # measured 1.57, see the module docstring
DEVICE_FACTOR = 4.0
NS_LIST = (0.0, 1.0, 10.0, 50.0, 400.0, 2000.0, 5000.0, 9999.0, 10000.0, 20000.0)
GRAZING_Z = (0.0, 1e-6, -1e-6, 1e-4, 1e-2)
XI_EDGES = (0.0, EPS24, 0.5, 1.0 - EPS24)
DIFFUSE, PHONG, MIRROR = 0, 1, 2                            # BSDF_DIFFUSE / BSDF_PHONG / BSDF_MIRROR; also the lobe a sample took
# columns of `out12`, the probe's layout: fx[3] pdf | wo[3] f[3] pdf mirror
FX, PDF, S_WO, S_F, S_PDF, S_MIRROR = slice(0, 3), 3, slice(4, 7), slice(7, 10), 10, 11


# ------------------------------------------------------------------------------------------------------------------------ the restatement
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], 1)


def _normalize(a, T):
    return a * (T(1) / np.sqrt(_dot(a, a)))[:, None]


def _in(x, T, cols):
    x = np.asarray(x, np.float64).astype(F32).astype(T)
    return x.reshape(-1, cols) if cols else x.reshape(-1)


def frame(n, T=np.float64):
    """(u, v, w) of make_bsdf for normals `n` (N, 3): w = n, the helper axis switches at |n.x| > 0.9f."""
    n = _in(n, T, 3)
    a = np.where((np.abs(n[:, 0]) > T(FRAME_SWITCH))[:, None], np.array([0, 1, 0], T), np.array([1, 0, 0], T))
    v = _normalize(_cross(n, a), T)
    return _cross(n, v), v, n


def bsdf_ref(n, wi, kd, ks, ns, wo, xi, dtype=np.float64):
    """make_bsdf + bsdf_eval(wo) + bsdf_sample(xi = lobe, xi1, xi2) for N cases.  Returns a namespace of
      out12      (N, 12)  evaluation fx[3], pdf | sample world wo[3], f[3], pdf, mirror flag     (the probe's layout)
      m_wo_z, wo_z, s_wi_z    local z of the incoming direction, of the evaluated one, of the sampled one
      hz_eval, hz_sample      H.z of the two half vectors (1 where no Blinn-Phong term was evaluated)
      margin                  |w_spec - xi_lobe * total| (inf for a one-lobe material)
      z_eps                   4 ulp of the fp32 computation of m_wo_z and of wo_z: (N, 2)
      kind, lobe, failed, black, nonfinite (N, 12), scale (max(kd, ks) after the rescale), w_spec, w_diff, up (m_wo_z is not below 0),
      sin_t (of Specular::Sample), wo_diffuse / wo_specular (the world direction either lobe would have returned)
    """
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        return _bsdf_ref(T, _in(n, T, 3), _in(wi, T, 3), _in(kd, T, 3), _in(ks, T, 3), _in(ns, T, 0), _in(wo, T, 3), _in(xi, T, 3))


def _bsdf_ref(T, n, wi, kd, ks, ns, wo, xi):
    N = n.shape[0]
    # libm in the working precision, correctly rounded: evaluated in float64 and rounded once (numpy's own float32 loops are a few ulp off)
    lib = lambda f: (lambda *x: f(*[np.asarray(a, np.float64) for a in x]).astype(T))
    sin, cos, arccos, power = lib(np.sin), lib(np.cos), lib(np.arccos), lib(np.power)
    pi, zero, one = T(PI_F), np.zeros(N, T), np.ones(N, T)
    u, v, w = frame(n, T)
    m_wo = np.stack([_dot(wi, u), _dot(wi, v), _dot(wi, w)], 1)
    wl = np.stack([_dot(wo, u), _dot(wo, v), _dot(wo, w)], 1)
    z_eps = 4 * EPS24 * np.stack([(np.abs(wi) * np.abs(w)).sum(1), (np.abs(wo) * np.abs(w)).sum(1)], 1)

    has_spec = np.any(ks != 0, 1)
    kind = np.where(has_spec, np.where(ns >= T(MIRROR_NS), MIRROR, PHONG), DIFFUSE)
    ks = np.where((kind == MIRROR)[:, None], T(1), np.where(has_spec[:, None], ks, T(0)))
    lum = lambda c: c[:, 0] * T(LUM[0]) + c[:, 1] * T(LUM[1]) + c[:, 2] * T(LUM[2])
    lum_d, lum_s = lum(kd), lum(ks)
    total_lum = np.where(has_spec, lum_s + lum_d, lum_d)
    black = total_lum == 0
    inv = T(1) / np.where(black, one, total_lum)
    w_spec, w_diff = np.where(black, zero, lum_s * inv), np.where(black, zero, lum_d * inv)
    maxc = (ks + kd).max(1)
    rescale = ~(maxc < 1)
    div = np.where(rescale, maxc, one)[:, None]
    kd, ks = np.where(rescale[:, None], kd / div, kd), np.where(rescale[:, None], ks / div, ks)

    def phong(d):                                                     # (fx (N, 3), pdf, H.z) of the Blinn-Phong lobe for a local direction
        on = (kind == PHONG) & ~((d[:, 2] < 0) | (m_wo[:, 2] < 0))
        hz = np.where(on, _normalize(d + m_wo, T)[:, 2], one)
        p = power(hz, ns)
        fx = np.where(on[:, None], ks * ((ns + T(2)) / (T(2) * pi))[:, None] * p[:, None], T(0))
        return fx, np.where(on, (ns + T(1)) / (T(2) * pi) * p, zero), hz

    def diffuse_pdf(d):
        return np.where((d[:, 2] < 0) | (m_wo[:, 2] < 0), zero, d[:, 2] / pi)

    # ---- evaluation: lobes in the reference's order, [Phong | mirror] + Diffuse; the mirror lobe evaluates to nothing
    p_fx, p_pdf, hz_eval = phong(wl)
    fx = p_fx + kd / pi
    pdf = p_pdf * w_spec + diffuse_pdf(wl) * w_diff

    # ---- sample
    two = kind != DIFFUSE
    total = np.where(two, w_spec + w_diff, w_diff)
    pick_spec = two & (w_spec >= xi[:, 0] * total)                    # lower_bound over the prefix sums
    margin = np.where(two, np.abs(w_spec - xi[:, 0] * total), np.inf)
    lobe = np.where(pick_spec, kind, DIFFUSE)
    up = ~(m_wo[:, 2] < 0)
    phi = xi[:, 1] * T(2) * pi
    sp, cp = sin(phi), cos(phi)
    # Diffuse::Sample
    theta = T(0.5) * arccos(T(1) - T(2) * xi[:, 2])
    d_dir = np.stack([sin(theta) * cp, sin(theta) * sp, cos(theta)], 1)
    # Specular::Sample: H about the normal, the incoming direction reflected about it
    cos_t = power(xi[:, 2], T(1) / (ns + T(1)))
    sin_t = np.sqrt(np.maximum(T(1) - cos_t * cos_t, T(0)))
    H = np.stack([sin_t * cp, sin_t * sp, cos_t], 1)
    p_dir = -m_wo + H * T(2) * _dot(H, m_wo)[:, None]
    p_ok = up & ~(p_dir[:, 2] < 0)
    # specular_reflection::Sample
    m_dir = np.stack([-m_wo[:, 0], -m_wo[:, 1], m_wo[:, 2]], 1)

    is_d, is_p, is_m = lobe == DIFFUSE, lobe == PHONG, lobe == MIRROR
    ok = np.where(is_p, p_ok, up)                                     # the picked lobe returned a direction
    s_dir = np.where(ok[:, None], np.where(is_d[:, None], d_dir, np.where(is_p[:, None], p_dir, m_dir)), T(0))
    own_pdf = np.where(is_d, np.abs(d_dir[:, 2]) / pi, np.where(is_p, (ns + T(1)) / (T(2) * pi) * power(cos_t, ns), one))
    own_w = np.where(is_d, w_diff, w_spec)
    c_fx, c_pdf, hz_sample = phong(s_dir)                             # Blinn-Phong at the sampled direction: own f of a Phong pick, companion of a diffuse one
    s_pdf = np.where(ok, own_pdf, zero) * own_w
    s_f = np.where((ok & is_d)[:, None], kd / pi, T(0)) + np.where((ok & is_m)[:, None], (T(1) / np.where(is_m, m_wo[:, 2], one))[:, None], T(0))
    s_f = s_f + np.where((ok | is_d)[:, None], c_fx, T(0))             # (a failed Phong pick keeps f = 0; the companion of a failed diffuse pick is 0 by its own test)
    s_pdf = s_pdf + np.where(is_d, c_pdf * w_spec, zero)
    s_f = s_f + np.where(is_d[:, None], T(0), kd / pi)                # the diffuse companion of a specular pick: Diffuse::Fx has no hemisphere test
    s_pdf = s_pdf + np.where(is_d, zero, diffuse_pdf(s_dir) * w_diff)
    world = lambda d: d[:, 0:1] * u + d[:, 1:2] * v + d[:, 2:3] * w
    s_wo = world(s_dir)
    wo_diffuse, wo_specular = world(d_dir), world(np.where((kind == MIRROR)[:, None], m_dir, p_dir))   # what each lobe would have returned
    mirror = ok & is_m

    out = np.concatenate([fx, pdf[:, None], s_wo, s_f, s_pdf[:, None], mirror.astype(T)[:, None]], 1)
    return SimpleNamespace(out12=out, m_wo_z=m_wo[:, 2], wo_z=wl[:, 2], s_wi_z=np.where(is_p, p_dir[:, 2], s_dir[:, 2]), hz_eval=hz_eval,
                           hz_sample=hz_sample, margin=margin, z_eps=z_eps, kind=kind, lobe=lobe, failed=s_pdf == 0, black=black,
                           nonfinite=~np.isfinite(out), scale=np.maximum(kd, ks).max(1), w_spec=w_spec, w_diff=w_diff, up=up, sin_t=sin_t, wo_diffuse=wo_diffuse,
                           wo_specular=wo_specular)


def marginal(case, ref=None):
    """The cases whose discrete outcome may legitimately differ between two fp32 implementations (module docstring), from the restatement alone."""
    r = ref or bsdf_ref(*case_arrays(case))
    tie = (r.margin == 0) & (r.w_spec == r.w_diff) & (np.asarray(case["xi"])[:, 0] == F32(0.5))
    m = (np.abs(r.m_wo_z) < r.z_eps[:, 0]) | (np.abs(r.wo_z) < r.z_eps[:, 1])
    m |= (r.lobe == PHONG) & r.up & (np.abs(r.s_wi_z) < 1e-6)
    m |= (r.margin <= 2.0 ** -22) & ~tie
    return m


def budget(case, ref, K, sin_term=True):
    """(N, 12) allowed |difference| per output for the constant K (module docstring); 0 for the mirror flag."""
    q = np.abs(ref.out12)
    ns = np.asarray(case["ns"], np.float64)
    ph = ref.kind == PHONG
    c = np.zeros((len(ns), 12)); s = np.ones((len(ns), 12)); powt = np.zeros((len(ns), 12))
    c[:, 0:4] = ph[:, None]; c[:, 7:11] = ph[:, None]
    s[:, 0:3] = ref.scale[:, None] / np.pi; s[:, 7:10] = ref.scale[:, None] / np.pi
    with np.errstate(all="ignore"):
        le, ls = np.abs(ns * np.log2(ref.hz_eval)), np.abs(ns * np.log2(ref.hz_sample))
        xi2 = np.asarray(case["xi"], np.float64)[:, 2]
        ld = np.where((ref.lobe == PHONG) & (xi2 > 0), np.abs(np.log2(xi2) / (ns + 1)), 0.0)
    powt[:, 0:4] = np.where(ph & np.isfinite(le), le, 0.0)[:, None]
    powt[:, 7:11] = np.where(ph & np.isfinite(ls), ls, 0.0)[:, None]
    powt[:, 4:7] = ld[:, None]
    q = np.where(np.isfinite(q), q, 0.0)
    b = K * 2.0 ** -23 * (q * (1 + ns[:, None] * c) + s) + powt * 2.0 ** -22 * q
    if sin_term:
        t = K * np.where(ref.lobe == PHONG, 2.0 ** -23 / np.maximum(ref.sin_t, 2.0 ** -12), 0.0)
        b[:, 4:7] += t[:, None]
        b[:, 10] += t * ref.w_diff / np.pi                             # the diffuse companion's pdf is wi.z / pi * w_diff
    b[:, 11] = 0
    return b


def smallest_k(case, ref, got, sin_term=True):
    """The smallest K at which `got` (N, 12) stays inside the model against `ref`, per case (N,): non-finite outputs of the restatement count 0."""
    unit, zero_k = budget(case, ref, 1.0, sin_term), budget(case, ref, 0.0, sin_term)
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(got, np.float64) - ref.out12)
        k = np.where(ref.nonfinite, 0.0, (err - zero_k) / np.where(unit > zero_k, unit - zero_k, 1.0))
    k[:, 11] = 0
    return np.maximum(np.where(np.isnan(k), np.inf, k), 0.0).max(1)


# ------------------------------------------------------------------------------------------------------------------------ the BSDF edge inputs
def case_arrays(case):
    return tuple(case[k] for k in ("n", "wi", "kd", "ks", "ns", "wo", "xi"))


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _upper(rng, nrm, n, zmin=0.2):
    """Directions at least `zmin` above the tangent plane of each normal: away from every sign test, and m_wo.z well conditioned."""
    u, v, w = frame(nrm)
    z = rng.uniform(zmin, 1.0, n); ph = rng.uniform(0, 2 * np.pi, n); r = np.sqrt(1 - z * z)
    return (r * np.cos(ph))[:, None] * u + (r * np.sin(ph))[:, None] * v + z[:, None] * w


def _at_z(rng, nrm, z):
    """Unit directions whose local z about `nrm` is z (exactly so, up to the fp32 rounding of the components, for axis-aligned normals)."""
    u, v, w = frame(nrm)
    z = np.broadcast_to(np.asarray(z, np.float64), (len(w),)); ph = rng.uniform(0, 2 * np.pi, len(w)); r = np.sqrt(1 - z * z)
    return (r * np.cos(ph))[:, None] * u + (r * np.sin(ph))[:, None] * v + z[:, None] * w


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
# kd, ks, ns of the stock materials: diffuse, Blinn-Phong at Ns 0 / 10 / 2000, mirror
STOCK = {"diffuse": ((0.6, 0.5, 0.3), (0, 0, 0), 1.0), "phong0": ((0.3, 0.2, 0.1), (0.4, 0.5, 0.3), 0.0), "phong10": ((0.3, 0.3, 0.3), (0.5, 0.4, 0.5), 10.0),
         "phong2000": ((0.2, 0.3, 0.1), (0.5, 0.5, 0.6), 2000.0), "mirror": ((0.1, 0.2, 0.1), (0.3, 0.3, 0.3), 20000.0)}


def _rand_xi(rng, n):
    return rng.integers(1, 1 << 24, (n, 3)).astype(np.float64) / (1 << 24)


def bsdf_edge_cases(seed=EDGE_SEED):
    """About 3500 fp32-exact cases as a dict of arrays n, wi, kd, ks, ns, wo, xi (float32) and `family` (str), in named families so that a failure
    says which one -- grazing angles (axis-aligned normals, where the local z is exact, and generic ones), the highlight peak, the exponents, the
    frame switch, the energy rescale, single lobes and the black material, the lobe pick at its boundary, the ends of the random numbers -- and
    plain random cases.  Deterministic in `seed`."""
    rng = np.random.default_rng(seed)
    rows = {k: [] for k in ("n", "wi", "kd", "ks", "ns", "wo", "xi", "family")}

    def add(family, n, wi, wo, kd, ks, ns, xi):
        m = len(n)
        for k, a, cols in (("n", n, 3), ("wi", wi, 3), ("wo", wo, 3), ("kd", kd, 3), ("ks", ks, 3), ("xi", xi, 3)):
            rows[k].append(np.broadcast_to(np.asarray(a, np.float64), (m, cols)).astype(F32))
        rows["ns"].append(np.broadcast_to(np.asarray(ns, np.float64), (m,)).astype(F32))
        rows["family"].append(np.full(m, family))

    def stock(names, m):
        pick = [STOCK[names[i % len(names)]] for i in range(m)]
        return np.array([p[0] for p in pick]), np.array([p[1] for p in pick]), np.array([p[2] for p in pick])

    # grazing, axis-aligned normals: the local z of wi and of wo IS the fp32 number asked for, 0 included
    zz = np.array([(a, b) for a in GRAZING_Z for b in GRAZING_Z])
    for mat in ("diffuse", "phong0", "phong2000", "mirror"):
        nrm = np.repeat(AXES, len(zz), 0); z = np.tile(zz, (len(AXES), 1))
        kd, ks, ns = STOCK[mat]
        add("grazing_axis", nrm, _at_z(rng, nrm, z[:, 0]), _at_z(rng, nrm, z[:, 1]), kd, ks, ns, _rand_xi(rng, len(nrm)))
    # ... and wo == -wi in the tangent plane under a Blinn-Phong material: the half vector is normalize(0), not a number
    for mat in ("phong0", "phong2000"):
        kd, ks, ns = STOCK[mat]
        wi = _at_z(rng, AXES, 0.0).astype(F32).astype(np.float64)
        add("grazing_axis", AXES, wi, -wi, kd, ks, ns, _rand_xi(rng, len(AXES)))
    # grazing, generic normals (no mirror: 1 / m_wo.z of a cancelling dot product is ill-conditioned in ANY fp32 arithmetic, which is not the subject)
    gz = np.array([(a, b) for a in GRAZING_Z[1:] for b in GRAZING_Z[1:]])
    nrm = _unit(rng, 12 * len(gz)).astype(F32).astype(np.float64); z = np.tile(gz, (12, 1))
    kd, ks, ns = stock(("diffuse", "phong0", "phong10", "phong2000"), len(nrm))
    add("grazing_generic", nrm, _at_z(rng, nrm, z[:, 0]), _at_z(rng, nrm, z[:, 1]), kd, ks, ns, _rand_xi(rng, len(nrm)))
    # highlight peak: wo within 1e-3 of the mirror direction, every Blinn-Phong exponent
    m = 320
    nrm = _unit(rng, m).astype(F32).astype(np.float64); wi = _upper(rng, nrm, m)
    refl = 2 * (wi * nrm).sum(1)[:, None] * nrm - wi
    wo = refl + 1e-3 * rng.uniform(0, 1, (m, 1)) * _unit(rng, m); wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    add("highlight", nrm, wi, wo, rng.uniform(0.05, 0.4, (m, 3)), rng.uniform(0.05, 0.5, (m, 3)), np.resize(NS_LIST[:8], m), _rand_xi(rng, m))
    # exponents: every Ns of the list, mirror threshold and its neighbour included, both lobes picked
    m = 40 * len(NS_LIST)
    nrm = _unit(rng, m).astype(F32).astype(np.float64)
    add("exponents", nrm, _upper(rng, nrm, m), _upper(rng, nrm, m, 0.05), rng.uniform(0.05, 0.4, (m, 3)), rng.uniform(0.05, 0.5, (m, 3)),
        np.repeat(NS_LIST, 40), _rand_xi(rng, m))
    # frame switch: n.x at 0.9f and its two fp32 neighbours, both signs, and the six axis normals
    nx = np.array([FRAME_SWITCH, np.nextafter(FRAME_SWITCH, F32(1)), np.nextafter(FRAME_SWITCH, F32(0))], np.float64)
    nx = np.concatenate([nx, -nx]); m = 30
    ph = rng.uniform(0, 2 * np.pi, (len(nx), m)); r = np.sqrt(1 - nx * nx)[:, None]
    nrm = np.stack([np.broadcast_to(nx[:, None], ph.shape), r * np.cos(ph), r * np.sin(ph)], -1).reshape(-1, 3)
    nrm = np.concatenate([nrm, np.repeat(AXES, 20, 0)]).astype(F32).astype(np.float64); m = len(nrm)
    kd, ks, ns = stock(("diffuse", "phong10", "mirror", "phong2000"), m)
    add("frame_switch", nrm, _upper(rng, nrm, m), _upper(rng, nrm, m, 0.05), kd, ks, ns, _rand_xi(rng, m))
    # energy rescale: max(kd + ks) exactly 1, one ulp below, above; 0.5 - 2^-24 + 0.5 is exact in fp32
    below = 0.5 - EPS24
    for kd, ks, ns in (((0.5, 0.25, 0.125), (0.5, 0.25, 0.125), 10.0), ((0.5, 0.25, 0.125), (below, 0.25, 0.125), 10.0),
                       ((0.7, 0.5, 0.25), (0.8, 0.25, 0.125), 50.0), ((1.0, 0.5, 0.25), (0, 0, 0), 1.0), ((1.0 - EPS24, 0.5, 0.25), (0, 0, 0), 1.0),
                       ((1.5, 2.5, 0.25), (0, 0, 0), 1.0), ((0.0, 0.0, 0.0), (0.3, 0.3, 0.3), 10000.0), ((0.25, 0.5, 0.125), (0.3, 0.3, 0.3), 10000.0),
                       ((0.25, below, 0.125), (0.125, 0.5, 0.25), 400.0), ((0.25, 0.5, 0.125), (0.125, 0.5, 0.25), 400.0)):
        m = 30
        nrm = _unit(rng, m).astype(F32).astype(np.float64)
        add("energy", nrm, _upper(rng, nrm, m), _upper(rng, nrm, m, 0.05), kd, ks, ns, _rand_xi(rng, m))
    # single lobes and the black material
    for kd, ks, ns in (((0.6, 0.5, 0.3), (0, 0, 0), 50.0), ((0, 0, 0), (0.4, 0.5, 0.3), 50.0), ((0, 0, 0), (0.4, 0.5, 0.3), 0.0), ((0, 0, 0), (0.3, 0.3, 0.3), 10000.0),
                       ((0, 0, 0), (0, 0, 0), 10.0), ((0, 0, 0), (0, 0, 0), 0.0), ((0, 0, 0), (0, 0, 0), 20000.0)):
        m = 40
        nrm = _unit(rng, m).astype(F32).astype(np.float64)
        wi = _upper(rng, nrm, m); wi[::8] = -wi[::8]                              # some from below the surface
        add("single_lobe", nrm, wi, _upper(rng, nrm, m, 0.05), kd, ks, ns, _rand_xi(rng, m))
    # lobe pick at its boundary: grey kd == ks, xi_lobe = 0.5 exactly (the tie goes to the specular lobe), its fp32 neighbours, 0 and 1 - 2^-24
    for g, ns in ((0.25, 10.0), (0.4, 400.0), (0.3, 10000.0), (0.45, 0.0)):
        for x, m in ((0.5, 30), (0.5 + EPS24, 2), (0.5 - EPS24, 2), (0.0, 10), (1.0 - EPS24, 10)):
            nrm = _unit(rng, m).astype(F32).astype(np.float64); xi = _rand_xi(rng, m); xi[:, 0] = x
            ks = (g, g, g) if ns < MIRROR_NS else (1.0, 1.0, 1.0)
            add("lobe_boundary", nrm, _upper(rng, nrm, m), _upper(rng, nrm, m, 0.05), (g, g, g) if ns < MIRROR_NS else (1.0, 1.0, 1.0), ks, ns, xi)
    # ends of the random numbers: xi1, xi2 in {0, 2^-24, 0.5, 1 - 2^-24}, each lobe forced by xi_lobe = 0 / 1 - 2^-24
    ee = np.array([(a, b) for a in XI_EDGES for b in XI_EDGES])
    for mat in STOCK:
        for lobe_xi in (0.0, 1.0 - EPS24):
            m = 2 * len(ee)
            nrm = _unit(rng, m).astype(F32).astype(np.float64)
            xi = np.concatenate([np.full((m, 1), lobe_xi), np.tile(ee, (2, 1))], 1)
            kd, ks, ns = STOCK[mat]
            add("xi_edges", nrm, _upper(rng, nrm, m), _upper(rng, nrm, m, 0.05), kd, ks, ns, xi)
    # plain random cases, directions from the whole sphere
    m = 600
    nrm = _unit(rng, m).astype(F32).astype(np.float64)
    kd, ks, ns = rng.uniform(0, 0.6, (m, 3)), rng.uniform(0, 0.6, (m, 3)) * (rng.uniform(size=(m, 1)) < 0.7), rng.choice(NS_LIST, m)
    wi = _upper(rng, nrm, m); wi[::10] = -wi[::10]
    add("random", nrm, wi, _unit(rng, m), kd, ks, ns, _rand_xi(rng, m))
    return {k: np.concatenate(a) for k, a in rows.items()}


# ------------------------------------------------------------------------------------------------------------------------ the light edge inputs
def light_faces(scene):
    """Face indices of the light triangles, in the order of the device's and the oracle's light table (radiance longer than 0.01)."""
    return np.array([f for f in range(scene.n_faces) if np.linalg.norm(scene.materials[scene.face[f, 0, 3]].radiance) > 0.01], np.int64)


def light_index(xi_l, n_lights):
    """The light the device and the reference pick: int(xi * n) in fp32, clamped to n - 1 (Render.cpp:204-205).  (index, clamp was needed)"""
    raw = (np.asarray(xi_l, F32) * F32(n_lights)).astype(np.int64)
    return np.minimum(raw, n_lights - 1), raw > n_lights - 1


def light_edge_inputs(scene, seed=7):
    """Points (M, 3) fp64, xi (M, 3) fp32 and a family name per row for probe_sample_light on `scene`:
      index     xi_l = 0, 1 - 2^-24, every fp32(k / n_lights) with its two neighbours, and n_lights / n_lights = 1.  The clamp acts where
                xi_l * n_lights reaches n_lights in fp32, and below 2^24 lights that is xi_l = 1 ALONE: for n in (2^k, 2^(k+1)) the fp32 spacing
                below n is 2^(k-23), and (1 - 2^-24) n lies n 2^-24 > 2^(k-24), more than half a spacing, below n, so it rounds down (for
                n = 2^k the product is exact).  The generator's numbers end at 1 - 2^-24; the reference's own float generator can return 1
      fold      (u, v) with u + v exactly 1 (not folded), one fp32 ulp above 1 (folded), (0, 0), and both at 1 - 2^-24
      near      points 1e-4 below each light (along its vertex normal)
      in_plane  points in the plane of each axis-aligned light: cs == 0, the pdf must be exactly 0
      far       points 1e3 from a light
    """
    rng = np.random.default_rng(seed)
    lf = light_faces(scene); n = len(lf)
    P = scene.vertex[scene.face[lf][:, :, 0]].astype(np.float64)                 # (n, 3 corners, 3)
    Nv = scene.normal[scene.face[lf][:, :, 1]].astype(np.float64)
    cen, nrm = P.mean(1), Nv.mean(1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    size = np.linalg.norm(P[:, 1] - P[:, 0], axis=1)
    pts, xis, fam = [], [], []

    def add(family, p, xi):
        p = np.asarray(p, np.float64).reshape(-1, 3); xi = np.broadcast_to(np.asarray(xi, np.float64), (len(p), 3))
        pts.append(p); xis.append(xi.astype(F32)); fam.append(np.full(len(p), family))

    def below(i, dist, m, spread=0.5):
        t = _unit(rng, m); t -= (t * nrm[i]).sum(1)[:, None] * nrm[i]
        return cen[i] + dist * nrm[i] + spread * size[i] * t

    ks = np.arange(1, n, dtype=np.float64).astype(F32) / F32(n)
    xl = np.concatenate([[F32(0), ONE_BELOW, F32(1)], ks, np.nextafter(ks, F32(0)), np.nextafter(ks, F32(1))]).astype(F32)
    for i in range(40):
        p = below(i % n, 0.3 * max(size[i % n], 0.1), len(xl))
        add("index", p, np.concatenate([xl[:, None], _rand_xi(rng, len(xl))[:, 1:]], 1))
    uv = [(0.25, 0.75), (0.5, 0.5), (0.5, 0.5 + 2.0 ** -23), (0.75, 0.25 + 2.0 ** -23), (0.0, 0.0), (1 - EPS24, 1 - EPS24), (1.0 - EPS24, EPS24), (0.0, 1 - EPS24)]
    for i in range(n):
        x = (i + 0.5) / n
        for u_, v_ in uv:
            add("fold", below(i, 0.3 * max(size[i], 0.1), 20), (x, u_, v_))
        add("near", below(i, 1e-4, 60, 0.2), np.concatenate([np.full((60, 1), x), _rand_xi(rng, 60)[:, 1:]], 1))
        add("far", cen[i] + 1e3 * _upper(rng, np.repeat(nrm[i:i + 1], 60, 0), 60), np.concatenate([np.full((60, 1), x), _rand_xi(rng, 60)[:, 1:]], 1))
        for ax in range(3):                                                      # a light in a coordinate plane, lit along that axis
            if np.all(P[i, :, ax] == P[i, 0, ax]) and np.all(np.abs(Nv[i, :, ax]) == 1) and np.all(np.delete(Nv[i], ax, 1) == 0):
                p = cen[i] + size[i] * rng.uniform(-3, 3, (80, 3)); p[:, ax] = P[i, 0, ax]
                add("in_plane", p, np.concatenate([np.full((80, 1), x), _rand_xi(rng, 80)[:, 1:]], 1))
    p, xi, fam = np.concatenate(pts), np.concatenate(xis), np.concatenate(fam)
    # Keep the rows where the pdf is well conditioned (or exactly 0, the in-plane family).  The pdf divides by the cosine at the light, a dot product
    # that any fp32 arithmetic holds to ~2^-24 sum |d_k n_k|; where the terms cancel to less than 1/50 of that sum the 1e-4 relative tolerance of
    # the comparison would measure the cancellation, not the arithmetic.  (An axis-aligned light has one term: kept at any grazing angle.)
    idx, _ = light_index(xi[:, 0], n)
    uu, vv = xi[:, 1].astype(np.float64), xi[:, 2].astype(np.float64)
    fold = (xi[:, 1] + xi[:, 2]) > 1
    uu, vv = np.where(fold, 1 - uu, uu), np.where(fold, 1 - vv, vv)
    q = (1 - uu - vv)[:, None] * P[idx, 0] + uu[:, None] * P[idx, 1] + vv[:, None] * P[idx, 2]
    nq = (1 - uu - vv)[:, None] * Nv[idx, 0] + uu[:, None] * Nv[idx, 1] + vv[:, None] * Nv[idx, 2]
    d = q - p
    keep = (50 * np.abs((d * nq).sum(1)) >= np.abs(d * nq).sum(1)) | (fam == "in_plane")
    return p[keep], xi[keep], fam[keep]


def nine_light_scene(pkg, width=64, height=64):
    """S-cornell-small with seven more faces made emissive (a floor, a back-wall, a left-wall and a right-wall triangle and three of the sphere):
    nine light triangles, the smallest table the shade kernel reads from global memory instead of LDS, and a light count that is no power of two,
    so that the boundaries k / 9 are not fp32 numbers and xi_l * 9 rounds."""
    S = pkg.scenes
    b = S.cornell_box_small(width, height)
    mats = list(b.materials) + [S.Material("lamp", kd=(0.5, 0.5, 0.5), radiance=(3.0, 5.0, 2.0))]
    face = b.face.copy()
    face[[0, 5, 7, 8, 40, 200, 411], :, 3] = len(mats) - 1
    return S.SceneData("nine-lights", b.vertex, b.normal, b.texcoord, face, mats, b.camera, dict(b.meta))
