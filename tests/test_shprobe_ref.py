"""CPU: the light-probe stage's restatement (tests/shprobe_ref.py) -- the float64 slack S that sizes the device's bound,
the exact properties of the stratified directions, the reduction tree's order, the basis functions, the resolve, and the host-only helpers
mcpt_sh_grid and mcpt_sh_eval through ctypes and as a sanitized stand-alone program, the struct's layout.  No device is touched."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

from tests import bake_ref, deform_kit as K, kit, shprobe_ref as R
from tests.kit import bits

NEW_SYMBOLS = ["mcpt_set_sh_probes", "mcpt_bake_sh", "mcpt_clear_sh", "mcpt_read_sh", "mcpt_read_sh_film", "mcpt_get_sh_info", "mcpt_probe_sh_rays", "mcpt_read_sh_pass",
               "mcpt_sh_grid", "mcpt_sh_eval"]
METHODS = ["set_sh_probes", "bake_sh", "clear_sh", "read_sh", "read_sh_film", "sh_info", "probe_sh_rays", "read_sh_pass"]
INVALID = 1
F32 = np.float32


def _all_slots(n_xi=272):
    """Every slot under xi_cases' pairs (the 16 pairs of XI_SET and a random tail, a different tail per slot): (slot (N,), xi (N, 2))."""
    slot = np.repeat(np.arange(R.DIRS), n_xi)
    xi = np.concatenate([R.xi_cases(n_xi, R.SEED + j) for j in range(R.DIRS)])
    return slot, xi


def test_library_exports_the_light_probe_entry_points(pkg):
    kit.assert_exports(pkg, NEW_SYMBOLS, METHODS)
    assert (pkg.SH_RADIANCE, pkg.SH_IRRADIANCE, pkg.SH_DIRECTIONS, pkg.SH_MAX_PROBES) == (0, 1, 64, 0x3ffffff // 64)
    assert callable(pkg.sh_grid) and callable(pkg.sh_eval)


def test_null_context_is_an_invalid_argument_for_the_light_probe_calls(pkg):
    lib = pkg.load_library()
    buf = np.zeros(64, np.float64); p = buf.ctypes.data_as(C.c_void_p); info = pkg.ShInfo()
    assert lib.mcpt_set_sh_probes(None, p, 1) == INVALID
    assert lib.mcpt_bake_sh(None, 1, 0, 0) == INVALID
    assert lib.mcpt_clear_sh(None) == INVALID
    assert lib.mcpt_read_sh(None, 0, p) == INVALID
    assert lib.mcpt_read_sh_film(None, p, p) == INVALID
    assert lib.mcpt_get_sh_info(None, C.byref(info)) == INVALID
    assert lib.mcpt_probe_sh_rays(None, 0, 0, 0, 1, p, p) == INVALID
    assert lib.mcpt_read_sh_pass(None, p, p) == INVALID


def test_sh_info_has_the_headers_layout(pkg, tmp_path):
    """sizeof and every offsetof of mcpt_sh_info as a C compiler sees include/mcpt.h, against the ctypes class; the constants are the header's."""
    c, py, consts = K.c_layout(pkg.ShInfo, "mcpt_sh_info", tmp_path, ["MCPT_SH_RADIANCE", "MCPT_SH_IRRADIANCE", "MCPT_SH_DIRECTIONS", "MCPT_SH_MAX_PROBES"])
    assert c == py and c[0] == 56
    assert consts == [pkg.SH_RADIANCE, pkg.SH_IRRADIANCE, pkg.SH_DIRECTIONS, pkg.SH_MAX_PROBES]
    assert [f[0] for f in pkg.ShInfo._fields_] == ["struct_size", "n_probes", "bakes", "reserved0", "passes", "last_stage_ms", "device_bytes", "reserved"]


# ------------------------------------------------------------------------------------------------------------------------ the restatement
def test_float64_slack():
    """S: the worst difference between the float64 restatement and the same formulas in np.longdouble over every slot under every pair of
    bake_ref.XI_SET and a random tail, every unrounded direction component, in units of 2^-52 (1 + |value|).  S_BOUND, what the device is
    allowed, is 4 S rounded up to a power of two."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no more bits than float64 on this platform: S cannot be measured here"
    slot, xi = _all_slots()
    grid = np.array([(a, b) for a in bake_ref.XI_SET for b in bake_ref.XI_SET], F32)
    assert np.array_equal(xi[:16], grid) and len(slot) == 64 * 272
    a = R.rays(slot, xi); b = R.rays(slot, xi, T=np.longdouble)
    assert a.dtype == np.float64 and b.dtype == np.longdouble
    err = np.abs(a.astype(np.longdouble) - b) / (np.longdouble(2.0) ** -52 * (1 + np.abs(b)))
    S = float(err.max()); where = np.unravel_index(np.argmax(err), err.shape)
    bound = 2.0 ** np.ceil(np.log2(4.0 * S))
    print("S = %.3f (slot %d, xi %s, component %d), 4 S = %.2f, S_BOUND = %g" % (S, slot[where[0]], xi[where[0]], where[1], 4 * S, bound))
    assert abs(S - R.S_CPU) < 0.01 and bound == R.S_BOUND, "tests/shprobe_ref.py states S = %.2f and S_BOUND = %g" % (R.S_CPU, R.S_BOUND)


def test_directions_lie_in_their_cells_and_have_unit_length():
    """Exact properties of the restatement, for every slot and every pair: z lies in [1 - 2 (jx + 1) / 8, 1 - 2 jx / 8] (and stays there when
    rounded to fp32: the cell's borders are fp32 numbers); the azimuth parameter v lies in cell jy, [jy / 8, (jy + 1) / 8), and so does the
    angle of (x, y) wherever the direction is not at a pole; |d| rounded to fp32 is within 2 fp32 ulp (2 x 2^-23) of 1."""
    slot, xi = _all_slots()
    jx = (slot & 7).astype(np.float64); jy = (slot >> 3).astype(np.float64)
    d = R.rays(slot, xi); u, v = R.slot_uv(slot, xi)
    for z in (d[:, 2], d[:, 2].astype(F32).astype(np.float64)):
        assert (z >= 1 - 2 * (jx + 1) / 8).all() and (z <= 1 - 2 * jx / 8).all()
    assert (v >= jy / 8).all() and (v < (jy + 1) / 8).all() and (u >= jx / 8).all() and (u < (jx + 1) / 8).all()
    ring = np.hypot(d[:, 0], d[:, 1]) > 1e-3
    ang = np.mod(np.arctan2(d[:, 1], d[:, 0]), 2 * np.pi) / (2 * np.pi)
    off = np.minimum(np.abs(ang - v), 1 - np.abs(ang - v))                      # (v = 0 may come back as an angle just under 1 turn)
    assert ring.mean() > 0.99 and off[ring].max() < 1e-15 / 1e-3
    d32 = d.astype(F32).astype(np.float64)
    length = np.sqrt((d32 * d32).sum(1))
    print("%d directions: worst | |d| - 1 | = %.3e (bound %.3e)" % (len(d), np.abs(length - 1).max(), 2 * 2.0 ** -23))
    assert np.abs(length - 1).max() <= 2 * 2.0 ** -23
    # the 64 cells tile the sphere with equal measure: the mean direction of the cell centres vanishes
    centre = R.rays(np.arange(64), np.full((64, 2), 0.5, F32))
    assert np.abs(centre.mean(0)).max() < 1e-14


def test_tree_order_is_pinned():
    """tree_sum equals an explicit loop over the definition s_(m-1)[j] = s_m[j] + s_m[j + 2^(m-1)], bit for bit, on random fp32 data of mixed
    magnitude; and it is THAT order: for a crafted input it differs from the left-to-right fp32 sum and from np.sum in fp64."""
    rng = np.random.default_rng(R.SEED)
    t = (rng.standard_normal((64, 27)) * 10.0 ** rng.integers(-6, 7, (64, 27))).astype(F32)
    want = np.zeros(27, F32)
    for q in range(27):
        s = [F32(x) for x in t[:, q]]
        for m in range(6, 0, -1):
            h = 2 ** (m - 1)
            s = [F32(s[j] + s[j + h]) for j in range(h)]
        want[q] = s[0]
    got = R.tree_sum(t)
    assert got.dtype == F32 and np.array_equal(bits(got), bits(want))
    # crafted: 2^24 meets its partner -2^24 at the LAST level only; on the way each swallows the ones of its own half
    c = np.ones(64, F32); c[0] = 2.0 ** 24; c[1] = -2.0 ** 24
    tree = float(R.tree_sum(c)); seq = F32(0)
    for x in c:
        seq = F32(seq + x)
    print("crafted input: tree %g, left to right in fp32 %g, np.sum in fp64 %g" % (tree, float(seq), c.astype(np.float64).sum()))
    assert c.astype(np.float64).sum() == 62.0 and tree != 62.0 and float(seq) == 62.0
    # s_1 = {the tree over the lanes of even index, the tree over the lanes of odd index}: each half loses ones of its own before the two meet
    even = R.tree_sum(np.concatenate([c[0::2], np.zeros(32, F32)])); odd = R.tree_sum(np.concatenate([c[1::2], np.zeros(32, F32)]))
    assert tree == float(F32(even + odd))


def test_project_zeroes_what_is_not_finite_and_sums_per_probe():
    """project over 3 probes: a NaN or infinite component of L counts as 0 (the same bits as the film with zeros in their places), the other
    components of that item still count, and a probe is the tree sum of ITS 64 items."""
    rng = np.random.default_rng(R.SEED + 1)
    n = 3
    film = np.concatenate([rng.uniform(0, 20, (64 * n, 3)), np.ones((64 * n, 1))], 1).astype(F32)
    d = R.rays(np.tile(np.arange(64), n), rng.integers(0, 1 << 24, (64 * n, 2)) / F32(1 << 24)).astype(F32).astype(np.float64)
    clean = R.project(film, d)
    assert clean.shape == (n, 3, 9) and clean.dtype == F32 and np.isfinite(clean).all()
    bad = film.copy(); bad[5, 0] = np.nan; bad[70, 1] = np.inf; bad[130, 2] = -np.inf
    zeroed = film.copy(); zeroed[5, 0] = 0; zeroed[70, 1] = 0; zeroed[130, 2] = 0
    assert np.array_equal(bits(R.project(bad, d)), bits(R.project(zeroed, d)))
    assert not np.array_equal(bits(R.project(bad, d)[0, 0]), bits(clean[0, 0])) and np.array_equal(bits(R.project(bad, d)[0, 1:]), bits(clean[0, 1:]))
    Y = R.basis(d)
    for p in range(n):
        rows = slice(64 * p, 64 * p + 64)
        assert np.array_equal(bits(clean[p, 1, 4]), bits(R.tree_sum((film[rows, 1] * Y[rows, 4]).astype(F32))))
    # L = 1 everywhere: band 0 sums to 64 Y0
    ones = R.project(np.ones((64, 4), F32), d[:64])
    assert abs(float(ones[0, 0, 0]) - 64 * 0.28209479) < 1e-4


def test_basis_closed_forms_and_orthonormality():
    """At the six axes and at (1, 1, 1) / sqrt(3) the nine functions equal their closed forms to fp32 rounding (4 x 2^-24 relative to the
    largest constant: three roundings and the fp32 input); under a 256 x 512 midpoint quadrature of the sphere they are orthonormal to 1e-4."""
    c0, c1, c2, c6, c8 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
    tol = 4 * 2.0 ** -24 * c2
    for a in range(3):
        for s in (1.0, -1.0):
            e = np.zeros(3); e[a] = s
            x, y, z = e
            want = [c0, c1 * y, c1 * z, c1 * x, 0, 0, c6 * (3 * z * z - 1), 0, c8 * (x * x - y * y)]
            assert np.abs(R.basis(e[None])[0].astype(np.float64) - want).max() <= tol
    w = 1.0 / np.sqrt(3.0)
    want = [c0, c1 * w, c1 * w, c1 * w, c2 / 3, c2 / 3, 0, c2 / 3, 0]
    assert np.abs(R.basis(np.full((1, 3), w))[0].astype(np.float64) - want).max() <= tol
    nt, nph = 256, 512
    zc = 1 - 2 * (np.arange(nt) + 0.5) / nt; ph = 2 * np.pi * (np.arange(nph) + 0.5) / nph           # equal-area cells: 4 pi / (nt nph) each
    Z, P = np.meshgrid(zc, ph, indexing="ij"); rr = np.sqrt(1 - Z * Z)
    d = np.stack([rr * np.cos(P), rr * np.sin(P), Z], -1).reshape(-1, 3)
    Y = R.basis(d).astype(np.float64)
    gram = Y.T @ Y * (4 * np.pi / (nt * nph))
    print("worst deviation of the Gram matrix from the identity: %.2e" % np.abs(gram - np.eye(9)).max())
    assert np.abs(gram - np.eye(9)).max() < 1e-4
    assert np.abs(R.basis64(d) - Y).max() < 1e-6


def test_resolve():
    """kf = float(4 pi) / float(rays) in fp32; irradiance = radiance times the band's fp32 factor; 0 where no ray was counted.  A constant
    radiance L resolves to c0 = L sqrt(4 pi) and E = pi L for every normal."""
    acc = np.zeros((3, 3, 9), F32); acc[0, :, 0] = F32(0.28209479177387814) * F32(128) * np.array([1, 2, 3], F32); acc[2] = 5
    cnt = np.array([128, 64, 0])
    rad = R.resolve(acc, cnt); irr = R.resolve(acc, cnt, irradiance=True)
    assert rad.dtype == F32 and (rad[2] == 0).all() and (irr[2] == 0).all() and (rad[1] == 0).all()
    assert np.allclose(rad[0, :, 0], np.sqrt(4 * np.pi) * np.array([1, 2, 3]), rtol=1e-6)
    assert np.array_equal(bits(irr), bits((R.BAND_FACTOR[R.BAND][None, None] * rad).astype(F32)))
    assert np.allclose(R.evaluate(irr[:1], [0.3, -0.5, 0.8]), np.pi * np.array([[1, 2, 3]]), rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------------------ the host helpers
def test_sh_grid_counts_order_capacity_and_refusals(pkg):
    """mcpt_sh_grid: nx ny nz cell centres in x-fastest order, equal to the restatement bit for bit; capacity < the count is
    MCPT_ERR_INVALID_ARG with *out_n set and nothing written (mcpt_lightmap_points' protocol); refusals."""
    lo, hi = np.array([-1.0, 0.25, 2.0]), np.array([3.0, 0.75, 2.0])
    g = pkg.sh_grid(lo, hi, 4, 3, 2)
    assert g.shape == (24, 3) and np.array_equal(bits(g), bits(R.grid(lo, hi, 4, 3, 2)))
    assert np.array_equal(g[:4, 0], [-0.5, 0.5, 1.5, 2.5]) and (g[:4, 1] == g[0, 1]).all() and g[4, 1] > g[0, 1] and (g[:, 2] == 2.0).all()
    assert np.array_equal(pkg.sh_grid(lo, hi, 1, 1, 1), 0.5 * (lo + hi)[None])
    lib = pkg.load_library()
    n = C.c_uint32(99); out = np.full((24, 3), 7.0)
    args = (lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p))
    assert lib.mcpt_sh_grid(*args, 4, 3, 2, 23, out.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID
    assert n.value == 24 and (out == 7.0).all() and b"capacity" in lib.mcpt_last_error()
    assert lib.mcpt_sh_grid(*args, 4, 3, 2, 24, out.ctypes.data_as(C.c_void_p), C.byref(n)) == 0 and n.value == 24 and np.array_equal(out, g)
    assert lib.mcpt_sh_grid(*args, 4, 3, 2, 24, None, C.byref(n)) == INVALID and n.value == 24
    assert lib.mcpt_sh_grid(*args, 4, 3, 2, 24, out.ctypes.data_as(C.c_void_p), None) == INVALID
    assert lib.mcpt_sh_grid(None, args[1], 4, 3, 2, 24, out.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID and n.value == 0
    for dims in ((0, 3, 2), (4, 0, 2), (4, 3, 0), (1024, 1024, 1), (0xffffffff, 0xffffffff, 0xffffffff)):
        assert lib.mcpt_sh_grid(*args, *dims, 24, out.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID and n.value == 0
    assert lib.mcpt_sh_grid(*args, 1023, 1025, 1, 0, None, C.byref(n)) == INVALID and n.value == 1023 * 1025         # 1 048 575: the most a context takes
    for bad_lo, bad_hi in ((np.array([np.nan, 0, 0]), hi), (lo, np.array([np.inf, 1, 3])), (np.array([4.0, 0.25, 2.0]), hi), (np.full(3, -1e308), np.full(3, 1e308))):
        with pytest.raises(pkg.McptError, match="mcpt_sh_grid: the box"):
            pkg.sh_grid(bad_lo, bad_hi, 2, 2, 2)


def _eval_cases():
    rng = np.random.default_rng(R.SEED + 2)
    coeffs = rng.standard_normal((40, 27)).astype(F32)
    normal = rng.standard_normal((40, 3)) * 10.0 ** rng.integers(-3, 4, (40, 1))
    normal[0] = 0.0; normal[1] = (0, 0, 1); normal[2] = (0, -2, 0); normal[3] = (1e-200, 0, 0); normal[4] = (np.nan, 1, 0); normal[5] = (1e200, 1e200, 0)
    return coeffs, normal


def test_sh_eval_against_the_numpy_formula(pkg):
    """mcpt_sh_eval equals the restatement bit for bit: the normal normalised in fp64, the sum over k ascending; 0 for a zero normal, for one
    whose length underflows to 0, overflows or is not a number.  A band-0-only probe gives the same value for every normal."""
    coeffs, normal = _eval_cases()
    got = pkg.sh_eval(coeffs, normal); want = R.evaluate(coeffs, normal)
    assert np.array_equal(bits(got + 0.0), bits(want + 0.0))
    assert (got[[0, 3, 4, 5]] == 0).all() and (got[[1, 2]] != 0).all()
    flat = np.zeros((1, 27), F32); flat[0, 0::9] = (1, 2, 3)
    assert np.array_equal(pkg.sh_eval(flat, [0, 1, 0]), pkg.sh_eval(flat, [0.6, 0, -0.8]))
    lib = pkg.load_library()
    assert lib.mcpt_sh_eval(None, normal.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p)) == INVALID


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
def test_host_helpers_as_a_stand_alone_program(pkg, tmp_path, sanitized):
    """The host half of the feature -- sh_grid_points, sh_check_probes and sh_eval_probe of csrc/shprobe_plan.h -- built into the stand-alone
    program tests/shprobe_host_check.cpp (no device is touched), plain and under the host's address and undefined-behaviour sanitizers: the
    same positions and values as the library gives through ctypes; every grid passes mcpt_set_sh_probes' rule inside the program and a NaN in
    it is refused by name."""
    exe = K.build_host_check("shprobe_host_check", [], tmp_path, sanitized)
    grids = [((-1.0, 0.25, 2.0), (3.0, 0.75, 2.0), (4, 3, 2)), ((0, 0, 0), (1, 1, 1), (1, 1, 1)), ((-0.3, -0.1, 0.7), (0.9, 1.3, 0.71), (7, 5, 3)),
             ((0, 0, 0), (1, 1, 1), (0, 2, 2)), ((0, 0, 0), (np.nan, 1, 1), (2, 2, 2)), ((0, 0, 0), (1, 1, 1), (1024, 1024, 2))]
    coeffs, normal = _eval_cases()
    blob = struct.pack("<I", len(grids))
    for lo, hi, dims in grids:
        blob += np.array(lo + hi, np.float64).tobytes() + struct.pack("<3I", *dims)
    blob += struct.pack("<I", len(coeffs))
    for c, nrm in zip(coeffs, normal):
        blob += c.tobytes() + nrm.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    K.run_host_check(exe, tmp_path, sanitized)
    out = (tmp_path / "out.bin").read_bytes(); at = 0
    for k, (lo, hi, dims) in enumerate(grids):
        status, n = struct.unpack_from("<2I", out, at); at += 8
        xyz = np.frombuffer(out, np.float64, 3 * n, at).reshape(n, 3); at += 24 * n
        if k < 3:
            assert status == 0 and np.array_equal(bits(xyz), bits(pkg.sh_grid(lo, hi, *dims)))
        else:
            assert status == 1 and n == 0
    got = np.frombuffer(out, np.float64, 3 * len(coeffs), at).reshape(-1, 3); at += 24 * len(coeffs)
    assert at == len(out)
    assert np.array_equal(bits(got + 0.0), bits(pkg.sh_eval(coeffs, normal) + 0.0))
