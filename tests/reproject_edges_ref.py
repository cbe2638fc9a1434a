"""Per-pixel restatement of temporal reprojection (csrc/reproject.hip: rp_reproject_kernel, rp_reproject_motion_kernel,
rp_gather) that DECIDES every comparison of the kernel instead of forgiving the pixels near one.

tests/reproject_ref.py masks a pixel when a decision is within 1e-4 of flipping.  Here every quantity the kernel compares carries an explicit
bound on how far a legitimate device evaluation may lie from the value computed here; a comparison whose operands are further apart than the
bound is decided, one whose operands are closer is followed down BOTH branches to the end, and the pixel is *undecided* only if the branches
end in different outputs (written or not, or another count).  What is left undecided is what rounding really leaves open.

THE fp64 STEPS (camera constants, centre ray, surface point, basis inverse, c0, sx, sy, r; for motion the barycentric point and normal) are
evaluated with mpmath at 160 bits from the caller's doubles, so the value here is the real-number one.  Each carries a running error bound,
class E below, propagated by the textbook rules with u = 2^-53:

    x (+-) y : e = ex + ey + u |result|          x * y : e = |x| ey + |y| ex + ex ey + u |result|
    x / y    : e = (ex + |q| ey) / (|y| - ey) + u |q|            sqrt x : e = ex / (2 sqrt(x - ex)) + u |result|
    tan x    : e = ex (1 + tan^2) + 2 u |result|   (libm: within one ulp = 2 u)
    rsq64 x  : e = ex |r| / (2 (x - ex)) + 4 u |r| (pt_device.h: a hardware seed and two Newton steps, "~1 ulp"; two ulps are allowed here)

i.e. ONE u |result| per operation of the kernel (or host) expression, written out operation by operation in the functions below in the order
of the C++ source -- the operation count is not summarised into one multiple, it is carried through.  reproject.hip is built with
-ffp-contract=fast: a fused multiply-add commits one rounding where the unfused pair commits two, so the unfused count taken here bounds both
forms.  An operation on error-free operands whose real result is a double commits no rounding (x + 0.5, a product with an exact 0 or 1, a
difference of equal eyes): it adds nothing, which is what lets axis-aligned cameras give an exact c0 = 0.

THE fp32 STEPS.  Three kinds:
  * single IEEE operations on fp32 values that no contraction can reach -- (float) of an fp64 value, 1.f - fx, qn.w - r, depth_tolerance * r,
    rintf, fminf -- are emulated exactly with numpy.float32 (bound 0).  The conversions inherit the fp64 bound: if the fp64 value lies within
    it of a rounding boundary both neighbouring floats are followed.
  * sums of products -- nn, qq, the cosine, sw, sc, sc / sw, the colour sums -- go through class R.  R.v is what the UNFUSED evaluation gives,
    emulated operation by operation (each result rounded to fp32: beyond the range infinite, below half the least subnormal zero; subnormals
    kept, gfx9's default; divide and square root correctly rounded, HIP's default).  The only freedom the compiler has is to fuse a product
    into the sum it feeds, so a sum of error-free operands also tries the product unrounded, and R.e is the distance between the forms: 0 when
    they give the same float.  From there on e grows by the running rules above with u = 2^-24, plus 2^-149 per operation for gradual
    underflow.  On the dyadic lattice the tests use (counts 1 .. 4, means in eighths, weights in sixteenths, axis normals) every product is an
    fp32 value, all forms coincide, e stays 0, and a tie such as sc / sw = 2.5 is decided (half to even); so is a stray tap of weight 1e-14,
    which moves no sum in any form.
  * the colour where the forms do not coincide, below.

THE COLOUR is computed in fp64 from the same fp32 inputs (fx, fy and their complements as emulated, the old sums and counts):
rgb = (sum wq mean / sum wq) nh.  The kernel's roundings, relative, in units of u = 2^-24, unfused form:
    wq = a * b                      1   (the factors are exact here)
    mean = sum / count              1
    wq * mean                       1
    sr += ...   four additions      4   (each at most u times a partial sum, itself at most sum wq |mean|)
        numerator: (1 + 1 + 1 + 4) = 7 times sum wq |mean|
    sw: wq 1, four additions 4      5   relative to sw (positive terms)
    sr / sw, * nh                   2
so |device - here| <= K u sum wq |mean| nh / sw with K = 7 + 5 + 2 = 14 (first order; the fused forms commit fewer roundings; second-order terms
and this module's own fp64 arithmetic are covered by the factor 1 + 2^-20).  Where class R finds that all forms of the colour arithmetic give
the same floats -- the lattice, in particular wherever sw is a power of two there -- the pixel must match BIT FOR BIT (`exact`, bound 0).
None of these figures was measured on a device.
"""
from __future__ import annotations

import collections
import math

import mpmath
import numpy as np

from tests.kit import bits

F32 = np.float32
MP = mpmath.mp.clone()
MP.prec = 160
mpf = MP.mpf
U64 = mpf(2) ** -53
U32 = 2.0 ** -24
K_COLOUR = 14
MAX_BRANCHES = 256


def _is_double(v):
    return v == mpf(float(v))


class E:
    """An fp64 quantity of the kernel: v, its real value; e, a bound on |a legitimate device value - v| (module docstring)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v = mpf(v); self.e = mpf(e)

    @staticmethod
    def _rounded(v, ein, ulps=1):
        if ein == 0 and _is_double(v):
            return E(v, 0)
        return E(v, ein + ulps * U64 * (abs(v) + ein))

    def __add__(a, b):
        return E._rounded(a.v + b.v, a.e + b.e)

    def __sub__(a, b):
        return E._rounded(a.v - b.v, a.e + b.e)

    def __mul__(a, b):
        return E._rounded(a.v * b.v, abs(a.v) * b.e + abs(b.v) * a.e + a.e * b.e)

    def __truediv__(a, b):
        if abs(b.v) <= b.e:
            raise ZeroDivisionError("division by a quantity that may be zero")
        q = a.v / b.v
        return E._rounded(q, (a.e + abs(q) * b.e) / (abs(b.v) - b.e))

    def __neg__(a):
        return E(-a.v, a.e)

    def sqrt(a):
        if a.v == 0 and a.e == 0:
            return E(0)
        if a.v - a.e <= 0:
            raise ZeroDivisionError("square root of a quantity that may be zero")
        return E._rounded(MP.sqrt(a.v), a.e / (2 * MP.sqrt(a.v - a.e)))

    def rsq(a):
        if a.v - a.e <= 0:
            raise ZeroDivisionError("rsq of a quantity that may be zero")
        r = 1 / MP.sqrt(a.v)
        return E(r, a.e * r / (2 * (a.v - a.e)) + 4 * U64 * r) if not (a.e == 0 and _is_double(r)) else E(r, 0)


def _c(x):
    return E(float(x))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def camera_constants(cam, centre):
    """scene_build.cpp camera_constants() operation by operation."""
    pi = E(MP.pi, abs(mpf(math.pi) - MP.pi))                                 # PI_D, a rounded literal
    ang = _c(cam.fovy) * pi / _c(180.0) * _c(0.5)
    t = MP.tan(ang.v)
    h = E(t, ang.e * (1 + t * t) * (1 + mpf(2) ** -20) + 2 * U64 * abs(t)) * _c(2.0)
    eye, lookat, up = [_c(x) for x in cam.eye], [_c(x) for x in cam.lookat], [_c(x) for x in cam.up]
    fr = [lookat[a] - eye[a] for a in range(3)]
    inv = _c(1.0) / _dot(fr, fr).sqrt()
    front = [fr[a] * inv for a in range(3)]
    rt = [front[1] * up[2] - up[1] * front[2], front[2] * up[0] - up[2] * front[0], front[0] * up[1] - up[0] * front[1]]
    inv = _c(1.0) / _dot(rt, rt).sqrt()
    right = [rt[a] * inv for a in range(3)]
    return dict(eye=[eye[a] - _c(centre[a]) for a in range(3)], front=front, right=right, up=up, h=h, width=int(cam.width), height=int(cam.height))


def basis_inverse(c):
    """reproject.h rp_basis_inverse(): rows of the inverse of [front | right | up], or None for a basis the host refuses.  (The refusal compares
    |det| with 1e-12 of the column lengths; a camera within rounding of THAT is outside what these tests build, and is refused here too.)"""
    f, r, u = c["front"], c["right"], c["up"]
    rxu, uxf, fxr = _cross(r, u), _cross(u, f), _cross(f, r)
    det = _dot(f, rxu)
    scale = MP.sqrt(sum(x.v ** 2 for x in f)) * MP.sqrt(sum(x.v ** 2 for x in r)) * MP.sqrt(sum(x.v ** 2 for x in u))
    if not abs(det.v) - det.e > mpf("2e-12") * scale:
        return None
    return [[x / det for x in row] for row in (rxu, uxf, fxr)]


# ------------------------------------------------------------------------------------------------------------------------ fp32
def f32(x):
    """x rounded to fp32 (to nearest even; beyond the range infinite, below half the least subnormal zero), as a Python float."""
    with np.errstate(over="ignore", under="ignore"):
        return float(F32(x))


class R:
    """An fp32 quantity of the kernel.  v: the value the UNFUSED evaluation gives on the device; e: a bound on how far another legitimate
    evaluation -- one that fused a product into the sum it feeds -- lies from v; x: for a product of error-free factors, the product before its
    rounding, which is what a fused sum would add (module docstring)."""
    __slots__ = ("v", "e", "x")

    def __init__(self, v, e=0.0, x=None):
        self.v = float(v); self.e = float(e); self.x = x

    @staticmethod
    def _rounded(v, ein, x=None):
        if v != v or ein != ein:
            return R(math.nan)
        r = f32(v)
        if ein == 0.0 or math.isinf(r):
            return R(r, 0.0, x)
        return R(r, ein + U32 * (abs(r) + ein) + 2.0 ** -149)

    def __add__(a, b):
        if a.e == 0.0 and b.e == 0.0 and not (math.isinf(a.v) or math.isinf(b.v)):
            unfused = f32(a.v + b.v)
            e = 0.0
            if a.x is not None and a.x != a.v:
                e = max(e, abs(f32(a.x + b.v) - unfused))
            if b.x is not None and b.x != b.v:
                e = max(e, abs(f32(a.v + b.x) - unfused))
            return R(unfused, e)
        return R._rounded(a.v + b.v, a.e + b.e)

    def __mul__(a, b):
        if math.isinf(a.v) or math.isinf(b.v):
            return R(a.v * b.v)                                             # (inf * 0 = NaN)
        exact = a.e == 0.0 and b.e == 0.0
        return R._rounded(a.v * b.v, abs(a.v) * b.e + abs(b.v) * a.e + a.e * b.e, a.v * b.v if exact else None)

    def __truediv__(a, b):
        if b.e > 0.0 and abs(b.v) <= b.e:
            raise Branching("division by a quantity that may be zero")
        sign = math.copysign(1.0, a.v) * math.copysign(1.0, b.v)
        if a.v != a.v or b.v != b.v or (math.isinf(a.v) and math.isinf(b.v)) or (a.v == 0.0 and b.v == 0.0):
            return R(math.nan)
        if math.isinf(a.v) or b.v == 0.0:
            return R(sign * math.inf)
        if math.isinf(b.v):
            return R(sign * 0.0)
        q = a.v / b.v
        return R._rounded(q, (a.e + abs(q) * b.e) / (abs(b.v) - b.e))

    def sqrt(a):
        if math.isinf(a.v) or a.v == 0.0:
            return R(a.v)
        if a.v - a.e <= 0.0:
            raise Branching("square root of a quantity that may be zero")
        return R._rounded(math.sqrt(a.v), a.e / (2.0 * math.sqrt(a.v - a.e)))


def _rint(x):
    """rintf under round-to-nearest-even."""
    return x if (math.isinf(x) or x != x) else float(round(x))


class Branching(Exception):
    """A pixel whose both-branch evaluation cannot be carried through (more than MAX_BRANCHES, or a quantity without a bound)."""


class Decider:
    """Follows one assignment of the ambiguous decisions of a pixel; `pending` collects the assignments still to follow."""

    def __init__(self, path, stats):
        self.path, self.i, self.pending, self.stats = list(path), 0, [], stats if not path else None

    def pick(self, options):
        """One of `options` (the first is the nominal one); an ambiguous choice when there are several."""
        if len(options) == 1:
            return options[0]
        if self.i == len(self.path):
            for j in range(1, len(options)):
                self.pending.append(self.path[:self.i] + [j])
            self.path.append(0)
        k = self.path[self.i]; self.i += 1
        return options[k]

    def cmp(self, name, nominal, ambiguous=False, equal=False):
        """The outcome of comparison `name`: `nominal` unless ambiguous, then both in turn.  The first evaluation of a pixel tallies which side
        each comparison took, and whether its operands were exactly equal or within their bound."""
        nominal = bool(nominal)
        if self.stats is not None:
            self.stats[(name, nominal)] += 1
            if equal:
                self.stats[(name, "equal")] += 1
            if ambiguous:
                self.stats[(name, "within bound")] += 1
        return self.pick([nominal, not nominal] if ambiguous else [nominal])

    def gt0(self, name, q):
        return self.cmp(name, q.v > 0, abs(q.v) <= q.e and q.e > 0, q.v == 0 and q.e == 0)

    def ge(self, name, q, bound):
        """q >= bound for an R or E q and an exact bound."""
        if q.v != q.v:
            return self.cmp(name, False)
        return self.cmp(name, q.v >= bound, q.e > 0 and abs(q.v - bound) <= q.e, q.v == bound and q.e == 0)

    def to_f32(self, q):
        """(float) of the fp64 quantity q: the neighbouring float too when q's bound reaches across a rounding boundary."""
        lo, hi = f32(float(q.v - q.e)), f32(float(q.v + q.e))
        mid = f32(float(q.v))
        if lo == hi:
            return mid
        if not (lo <= mid <= hi) or (mid != lo and mid != hi) or f32(np.nextafter(F32(lo), F32(np.inf))) != hi:
            raise Branching("a conversion to fp32 with more than two candidates")
        return self.pick([mid, hi if mid == lo else lo])


NONE = (False, 0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), True)


def _gather(dec, p, memo, vec, n_p, film, feat):
    """rp_gather for one pixel.  vec: three E; n_p: three R, the unit normal the taps are compared with; memo: the pixel's fp64 quantities, which are
    the same in every branch.  Returns (written, count, rgb, tolerance, exact)."""
    W, H, inv, hh = p["w"], p["h"], p["inv"], p["old"]["h"]
    if "c" not in memo:
        memo["c"] = [inv[k][0] * vec[0] + inv[k][1] * vec[1] + inv[k][2] * vec[2] for k in range(3)]
    c = memo["c"]
    if not dec.gt0("in front of the old eye", c[0]):
        return NONE
    if abs(c[0].v) <= c[0].e:
        # c0 may be anything in (0, |v| + e]: no bound on c1 / c0, but a lower one on its size.  If that puts sx or sy outside the window by itself
        # the pixel has no history whatever c0 is.
        ax = (abs(c[1].v) - c[1].e) / (abs(c[0].v) + c[0].e) / (hh.v * 1.001) * H
        ay = (abs(c[2].v) - c[2].e) / (abs(c[0].v) + c[0].e) / (hh.v * 1.001) * H
        if ax > W + 2 or ay > H + 2:
            dec.cmp("inside the old window", False)
            return NONE
        raise Branching("c0 within its bound of zero and the quotient not bounded away from the window")
    if "sx" not in memo:
        aspect = hh * _c(W) / _c(H)
        memo["sx"] = ((c[1] / c[0]) / aspect + _c(0.5)) * _c(W) - _c(0.5)
        memo["sy"] = ((c[2] / c[0]) / hh + _c(0.5)) * _c(H) - _c(0.5)
        memo["r"] = _dot(vec, vec).sqrt()
    sx, sy = memo["sx"], memo["sy"]
    inside = True
    for name, q, lim, below in (("sx > -1", sx, -1, False), ("sx < W", sx, W, True), ("sy > -1", sy, -1, False), ("sy < H", sy, H, True)):
        amb = abs(q.v - lim) <= q.e
        if not dec.cmp(name, q.v < lim if below else q.v > lim, amb, q.v == lim and q.e == 0):
            inside = False
            break
    if not inside:
        return NONE
    r = dec.to_f32(memo["r"])
    x0fx = []
    for name, q, size in (("floor sx", sx, W), ("floor sy", sy, H)):
        n = int(MP.floor(q.v + mpf(0.5)))                                    # the whole number sx may be rounding across
        if abs(q.v - n) <= q.e:
            fl = n if dec.cmp(name + " takes the upper cell", q.v >= n, True) else n - 1
        else:
            fl = int(MP.floor(q.v))
        # (within the window the floor is in [-1, size - 1]; a forced branch at the window's own edge keeps that)
        fl = min(max(fl, -1), size - 1)
        frac = q - E(fl)                                                     # fp64 subtraction
        lo, hi = max(frac.v - frac.e, mpf(0)), min(frac.v + frac.e, mpf(1))
        if lo == 0 and 0 < hi < mpf(2) ** -30:
            # on the whole number within the bound: the upper tap's fraction is 0 or some tiny positive float.  All tiny values act alike (the
            # complement is 1.f, the weight a tiny positive number that moves no sum unless it multiplies an infinite count), so one stands for them.
            f = R(dec.pick([f32(float(hi)), 0.0]))
        else:
            # (float) of the fraction: one float, or -- next to a rounding boundary, or for a small fraction, where floats lie closer together
            # than the fp64 bound -- the floats the bound reaches, as an R
            f = R(f32(float(frac.v)), f32(float(hi)) - f32(float(lo)))
        x0fx.append((fl, f))
    (x0, fx), (y0, fy) = x0fx
    ztol = f32(F32(p["depth_tolerance"]) * F32(r))
    sw, sc = R(0.0), R(0.0)
    taps = []
    for t in range(4):
        qx, qy = x0 + (t & 1), y0 + (t >> 1)
        a = fx if t & 1 else R(1.0) + R(-fx.v, fx.e)
        b = fy if t >> 1 else R(1.0) + R(-fy.v, fy.e)
        wq = a * b
        if not dec.cmp("tap inside the image", 0 <= qx < W and 0 <= qy < H):
            continue
        if not dec.gt0("tap weight > 0", wq):
            continue
        qf, qa = film[qy, qx], feat[qy, qx]
        cnt = float(qf[3])
        if not dec.cmp("old count > 0", cnt > 0, False, cnt == 0):
            continue
        if not dec.cmp("old coverage >= 0.5", float(qa[3]) >= 0.5, False, float(qa[3]) == 0.5):
            continue
        dz = f32(abs(F32(qa[7]) - F32(r)))
        if not dec.cmp("depth within tolerance", dz <= ztol, False, dz == ztol):
            continue
        qn = [R(float(v)) for v in qa[4:7]]
        qq = qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2]
        if qq.v != qq.v or not dec.gt0("tap normal length > 0", qq):
            continue
        qinv = R(1.0) / qq.sqrt()
        cos = (qn[0] * n_p[0] + qn[1] * n_p[1] + qn[2] * n_p[2]) * qinv
        if not dec.ge("cosine >= threshold", cos, f32(p["normal_threshold"])):
            continue
        mean = [R(0.0) if float(v) != float(v) else R(float(v)) / R(cnt) for v in qf[:3]]      # NaN sums zeroed, as the kernel does; x / inf = 0
        sw = sw + wq; sc = sc + wq * R(cnt)
        taps.append((wq, a.v * b.v, mean, [0.0 if float(v) != float(v) else float(v) / cnt for v in qf[:3]]))
    if not dec.ge("sw >= 0.25", sw, 0.25):
        return NONE
    avg = sc / sw
    if avg.e > 0 and _rint(avg.v - avg.e) != _rint(avg.v + avg.e):
        lo, hi = _rint(avg.v - avg.e), _rint(avg.v + avg.e)
        if hi - lo != 1:
            raise Branching("the count average spans more than one rounding boundary")
        n = _rint(avg.v)
        n = dec.pick([n, hi if n == lo else lo])
        if dec.stats is not None:
            dec.stats[("rint", "within bound")] += 1
    else:
        n = _rint(avg.v)
        if dec.stats is not None and not math.isinf(avg.v):
            dec.stats[("rint", "tie" if abs(avg.v - math.floor(avg.v) - 0.5) == 0 else ("up" if n > avg.v else "down" if n < avg.v else "whole"))] += 1
    cap = f32(p["max_history"])
    nh = cap if dec.cmp("count above the cap", n > cap, False, n == cap) else n
    if not dec.cmp("history >= 1", nh >= 1, False, nh == 1):
        return NONE
    # the colour.  Emulated first: where every form of the kernel's arithmetic gives the same floats (e = 0) that is the answer, bit for bit
    # A stray tap of a whole-pixel landing has a weight somewhere in (0, bound], for which ONE value stood above.  The emulation is the answer only
    # if it comes out the same with the stray taps left out: rounding is monotone, so every weight in between then gives those floats too.
    def emulate(which):
        out, s_w = [], R(0.0)
        for wq, _, _, _ in which:
            s_w = s_w + wq
        for ch in range(3):
            sr = R(0.0)
            for wq, _, mean, _ in which:
                sr = sr + wq * mean[ch]
            out.append(sr / s_w * R(nh))
        return out if s_w.e == 0.0 and all(q.e == 0.0 and q.v == q.v for q in out) else None
    stray = [t for t in taps if t[1] < 2.0 ** -30]
    emulated = emulate(taps)
    if emulated is not None and stray:
        without = emulate([t for t in taps if t[1] >= 2.0 ** -30])
        if without is None or any(bits(F32(p.v)) != bits(F32(q.v)) for p, q in zip(emulated, without)):
            emulated = None
    if emulated is not None:
        return (True, nh, tuple(q.v for q in emulated), (0.0, 0.0, 0.0), True)
    # otherwise fp64 from the same fp32 inputs, and the bound of the module docstring -- plus all a stray tap can add, since its weight is open
    SW = sum(w for _, w, _, _ in taps)
    rgb, tol = [], []
    for ch in range(3):
        s = sum(w * m[ch] for _, w, _, m in taps); mag = sum(w * abs(m[ch]) for _, w, _, m in taps)
        open_part = sum(w * abs(m[ch]) for _, w, _, m in stray)
        rgb.append(s / SW * nh); tol.append((K_COLOUR * U32 * mag + open_part) * nh / SW * (1 + 2.0 ** -20))
    return (True, nh, tuple(rgb), tuple(tol), False)


def _alive(dec, fa, fn):
    """The new pixel's own tests; its squared normal length as an R (or None)."""
    if not dec.cmp("new coverage >= 0.5", float(fa[3]) >= 0.5, False, float(fa[3]) == 0.5):
        return None
    z = float(fn[3])
    if not dec.cmp("new depth > 0", z > 0, False, z == 0):
        return None
    n = [R(float(v)) for v in fn[:3]]
    nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
    if nn.v != nn.v or not dec.gt0("new normal length > 0", nn):
        return None
    return nn


def _pixel_camera(dec, p, memo, x, y, film, feat_old, feat_new):
    fa, fn = feat_new[y, x, :4], feat_new[y, x, 4:]
    nn = _alive(dec, fa, fn)
    if nn is None:
        return NONE
    if math.isinf(float(fn[3])):
        # zi = inf: every component of v is +-inf (d != 0) or NaN (inf * 0), so c0 and c1 are +-inf or NaN, c1 / c0 is NaN whenever c0 > 0 holds at
        # all, and the window comparison is false: no history, in any evaluation order.
        return NONE
    ninv = R(1.0) / nn.sqrt()
    n_p = [R(float(v)) * ninv for v in fn[:3]]
    if "vec" not in memo:
        c, o = p["new"], p["old"]
        W, H = _c(p["w"]), _c(p["h"])
        u = (((E(x + 0.5) / W - _c(0.5)) * c["h"]) * W) / H
        v = (E(y + 0.5) / H - _c(0.5)) * c["h"]
        d = [c["front"][a] + u * c["right"][a] + v * c["up"][a] for a in range(3)]
        zi = E(float(fn[3])) * _dot(d, d).rsq()
        memo["vec"] = [(c["eye"][a] - o["eye"][a]) + zi * d[a] for a in range(3)]
    return _gather(dec, p, memo, memo["vec"], n_p, film, feat_old)


def _pixel_motion(dec, p, memo, m, x, y, film, feat_old, feat_new):
    fa, fn = feat_new[y, x, :4], feat_new[y, x, 4:]
    if _alive(dec, fa, fn) is None:
        return NONE
    f = int(m["hit_face"][y, x])
    if not dec.cmp("first hit names a triangle", 0 <= f < m["face"].shape[0]):
        return NONE
    if not dec.cmp("first hit is no emitter", not m["emissive"][f]):
        return NONE
    if "vec" not in memo:
        bu, bv = E(float(m["hit_uv"][y, x, 0])), E(float(m["hit_uv"][y, x, 1]))
        bw = _c(1.0) - bu - bv
        V = [[E(float(c)) for c in m["old_vertex"][m["face"][f, k, 0]]] for k in range(3)]
        N = [[E(float(c)) for c in m["old_normal"][m["face"][f, k, 1]]] for k in range(3)]
        o = p["old"]
        memo["vec"] = [((bw * V[0][a] + bu * V[1][a] + bv * V[2][a]) - _c(m["centre"][a])) - o["eye"][a] for a in range(3)]
        memo["n"] = n = [bw * N[0][a] + bu * N[1][a] + bv * N[2][a] for a in range(3)]
        memo["nl"] = _dot(n, n)
        memo["facing"] = _dot(n, memo["vec"])
    vec, n, nl = memo["vec"], memo["n"], memo["nl"]
    if not dec.gt0("old normal length > 0", nl):
        return NONE
    flip = dec.gt0("old normal faces away from the old eye", memo["facing"])
    ninv = nl.rsq()
    n_p = []
    for a in range(3):                                                       # (float) of the fp64 component: the floats its bound reaches, as an R
        q = n[a] * (-ninv if flip else ninv)
        lo, hi = f32(float(q.v - q.e)), f32(float(q.v + q.e))
        n_p.append(R(f32(float(q.v)), hi - lo))
    return _gather(dec, p, memo, vec, n_p, film, feat_old)


class Expected:
    """What the kernel must write.  film: (h, w, 4) float64 {rgb, count} of each pixel's nominal evaluation; tol: (h, w, 3) the colour bound
    (0 where `exact`: bit for bit); undecided: (h, w) bool; alts: {(y, x): [(rgb, tol), ...]} the other branches' colours where they differ
    from the nominal one though the count does not; stats: how often each named comparison went which way; branches: evaluations made."""

    def __init__(self, h, w):
        self.film = np.zeros((h, w, 4)); self.tol = np.zeros((h, w, 3)); self.exact = np.ones((h, w), bool); self.undecided = np.zeros((h, w), bool)
        self.alts, self.stats, self.branches = {}, collections.Counter(), 0


def _run(p, pixel, h, w):
    out = Expected(h, w)
    for y in range(h):
        for x in range(w):
            todo, results, memo = [[]], [], {}
            try:
                while todo:
                    if len(results) >= MAX_BRANCHES:
                        raise Branching("too many branches")
                    dec = Decider(todo.pop(), out.stats)
                    results.append(pixel(dec, memo, x, y))
                    todo.extend(dec.pending)
            except (Branching, ZeroDivisionError) as why:
                out.undecided[y, x] = True
                out.stats[("given up", str(why))] += 1
                continue
            finally:
                out.branches += len(results)
            first = results[0]
            out.film[y, x, :3] = first[2]; out.film[y, x, 3] = first[1]; out.tol[y, x] = first[3]; out.exact[y, x] = first[4]
            if any((r[0], r[1]) != (first[0], first[1]) for r in results):
                out.undecided[y, x] = True
            else:
                others = sorted({(r[2], r[3]) for r in results if r[2] != first[2]})
                if others:
                    out.alts[(y, x)] = others
    return out


def _params(old_cam, new_cam, max_history, depth_tolerance, normal_threshold, centre):
    co, cn = camera_constants(old_cam, centre), camera_constants(new_cam, centre)
    return dict(old=co, new=cn, w=cn["width"], h=cn["height"], inv=basis_inverse(co), max_history=F32(max_history), depth_tolerance=F32(depth_tolerance),
                normal_threshold=F32(normal_threshold))


def reproject_edges_ref(old_cam, new_cam, old_film, old_feat, new_feat, max_history=32.0, depth_tolerance=0.05, normal_threshold=0.9, centre=(0.0, 0.0, 0.0)):
    """rp_reproject_kernel: an Expected.  Arguments as tests/reproject_ref.py reproject_ref."""
    p = _params(old_cam, new_cam, max_history, depth_tolerance, normal_threshold, centre)
    w, h = p["w"], p["h"]
    film = np.asarray(old_film, F32).reshape(h, w, 4); fo = np.asarray(old_feat, F32).reshape(h, w, 8); fn = np.asarray(new_feat, F32).reshape(h, w, 8)
    if p["inv"] is None:
        return Expected(h, w)
    return _run(p, lambda dec, memo, x, y: _pixel_camera(dec, p, memo, x, y, film, fo, fn), h, w)


def reproject_motion_edges_ref(old_cam, new_cam, old_film, old_feat, new_feat, hit_face, hit_uv, face, emissive, old_vertex, old_normal, max_history=32.0,
                               depth_tolerance=0.05, normal_threshold=0.9, centre=(0.0, 0.0, 0.0)):
    """rp_reproject_motion_kernel: an Expected.  Arguments as tests/reproject_motion_ref.py reproject_motion_ref."""
    p = _params(old_cam, new_cam, max_history, depth_tolerance, normal_threshold, centre)
    w, h = p["w"], p["h"]
    film = np.asarray(old_film, F32).reshape(h, w, 4); fo = np.asarray(old_feat, F32).reshape(h, w, 8); fn = np.asarray(new_feat, F32).reshape(h, w, 8)
    if p["inv"] is None:
        return Expected(h, w)
    m = dict(hit_face=np.asarray(hit_face, np.int64).reshape(h, w), hit_uv=np.asarray(hit_uv, F32).reshape(h, w, 2), face=np.asarray(face),
             emissive=np.asarray(emissive, bool), old_vertex=np.asarray(old_vertex, np.float64), old_normal=np.asarray(old_normal, np.float64),
             centre=[float(c) for c in centre])
    return _run(p, lambda dec, memo, x, y: _pixel_motion(dec, p, memo, m, x, y, film, fo, fn), h, w)


def compare_decided(got, reused, want, undecided):
    """The device's film and its count of reused pixels against an Expected: `reused` is the number of pixels `got` has written, and the
    reference's own number when nothing is undecided; every decided pixel has the reference's count, an unwritten one is all +0, a written one's
    colour is within its bound of the nominal branch's (or of another branch's), bit for bit where the bound is 0."""
    got = np.asarray(got, F32)
    h, w = undecided.shape
    assert got.shape == (h, w, 4)
    assert int(reused) == int((got[..., 3] > 0).sum()), (int(reused), int((got[..., 3] > 0).sum()))
    if not undecided.any():
        assert int(reused) == int((want.film[..., 3] > 0).sum()), (int(reused), int((want.film[..., 3] > 0).sum()))
    ok = ~undecided
    bad = ok & (got[..., 3].astype(np.float64) != want.film[..., 3])
    assert not bad.any(), ("count", [(int(y), int(x), float(got[y, x, 3]), float(want.film[y, x, 3])) for y, x in np.argwhere(bad)[:8]])
    empty = ok & (want.film[..., 3] == 0)
    assert np.all(bits(got)[empty] == 0)
    worst = 0.0
    for y, x in np.argwhere(ok & (want.film[..., 3] > 0)):
        g = got[y, x, :3]
        cands = [(tuple(want.film[y, x, :3]), tuple(want.tol[y, x]))] + want.alts.get((int(y), int(x)), [])
        fits = False
        for rgb, tol in cands:
            if all(t == 0.0 for t in tol):
                fit = np.array_equal(bits(g), bits(np.asarray(rgb, F32)))
            else:
                err = np.abs(g.astype(np.float64) - np.asarray(rgb))
                fit = bool(np.all(err <= np.asarray(tol)))
                if fit:
                    worst = max(worst, float(np.max(err / np.maximum(np.asarray(tol), 1e-300))))
            fits |= fit
        assert fits, ("colour", int(y), int(x), [float(v) for v in g], cands)
    print("[edges] %d decided pixels (%d written, %d bit for bit), %d undecided; largest colour error / bound %.3g"
          % (int(ok.sum()), int((ok & (want.film[..., 3] > 0)).sum()), int((ok & (want.film[..., 3] > 0) & want.exact).sum()), int(undecided.sum()), worst))
