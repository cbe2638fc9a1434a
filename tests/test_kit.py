"""The comparison helpers of tests/kit.py and tests/deform_kit.py, which most suites lean on: bits() must tell apart what "bit for bit" means to
tell apart, compare_with_ref() must reject what lies just past its bounds, and assert_same(), assert_records() and c_layout() must name what
differs.  CPU only; milliseconds, but for two calls of the C compiler."""
import ctypes as C

import numpy as np
import pytest

from tests.deform_kit import assert_records, assert_same, c_layout
from tests.kit import bits, compare_with_ref, synthetic_film


# ------------------------------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bits_tells_the_two_zeros_apart(dtype):
    a, b = np.array([0.0, 1.0], dtype), np.array([-0.0, 1.0], dtype)
    assert np.array_equal(a, b)                                              # by value they are equal
    assert not np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(a), bits(a.copy()))


def test_bits_tells_nan_payloads_apart():
    for u, f in ((np.uint32, np.float32), (np.uint64, np.float64)):
        quiet = np.array([0x7FC00000 if u is np.uint32 else 0x7FF8000000000000], u).view(f)
        other = np.array([0x7FC00001 if u is np.uint32 else 0x7FF8000000000001], u).view(f)
        assert np.isnan(quiet).all() and np.isnan(other).all()
        assert not np.array_equal(quiet, quiet)                              # by value a NaN equals nothing
        assert np.array_equal(bits(quiet), bits(quiet.copy()))               # bit for bit it equals itself ...
        assert not np.array_equal(bits(quiet), bits(other))                  # ... and no NaN of another payload


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bits_tells_one_ulp_apart(dtype):
    a = np.array([[1.0, 3.0], [1e-30, -7.5]], dtype)
    b = a.copy(); b[1, 1] = np.nextafter(b[1, 1], dtype(0))
    assert bits(a).dtype == (np.uint32 if dtype is np.float32 else np.uint64) and bits(a).shape == a.shape
    assert not np.array_equal(bits(a), bits(b))
    assert int(np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64)).sum()) == 1
    # a double is never compared through its rounding to fp32: these two are one fp32 number and two fp64 numbers
    if dtype is np.float64:
        assert np.array_equal(a.astype(np.float32), b.astype(np.float32))


def test_bits_passes_integers_through_and_takes_strided_views():
    for dtype in (np.int32, np.uint32, np.uint8, np.int64, np.bool_):
        a = np.arange(6).astype(dtype)
        assert bits(a).dtype == a.dtype and np.array_equal(bits(a), a)
    f = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(bits(f[:, ::2]), np.ascontiguousarray(f[:, ::2]).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------ compare_with_ref
RTOL, ATOL = 1e-3, 1e-6                                                      # the bounds tests/test_reproject.py compares with


def _case():
    """A film as the restatement would give it, the same film as the device's, two marginal pixels and the count of reused ones."""
    want = synthetic_film(23, 37, 3)
    marg = np.zeros((23, 37), bool); marg[2, 3] = marg[5, 7] = True
    want[2, 3] = (4.0, 2.0, 6.0, 4.0); want[9, 9] = (4.0, 2.0, 6.0, 4.0); want[11, 4] = 0.0      # a marginal, a reused and an empty pixel
    return want.copy(), want, marg, int((want[..., 3] > 0).sum())


def _off_by(want, factor):
    """`want`'s colour moved by `factor` times the bound."""
    w = want.astype(np.float64)
    return (w + factor * (RTOL * np.abs(w) + ATOL)).astype(np.float32)


def test_compare_with_ref_accepts_up_to_its_bounds():
    got, want, marg, reused = _case()
    compare_with_ref(got, reused, want, marg)
    got[..., :3] = _off_by(want[..., :3], 0.9)
    compare_with_ref(got, reused, want, marg)
    compare_with_ref(got, reused, want, marg, rtol=RTOL, atol=ATOL)          # the defaults are those bounds
    compare_with_ref(got, reused + 2, want, marg); compare_with_ref(got, reused - 2, want, marg)   # two marginal pixels: two either way


def test_compare_with_ref_rejects_a_colour_just_past_the_tolerance():
    got, want, marg, reused = _case()
    got[9, 9, 1] = _off_by(want[9, 9, 1], 1.1)
    with pytest.raises(AssertionError):
        compare_with_ref(got, reused, want, marg)
    compare_with_ref(got, reused, want, marg, rtol=2 * RTOL)                 # it was the tolerance that rejected it
    # where the restatement holds 0 the absolute part alone is the bound
    got, want, marg, reused = _case()
    got[11, 4, 2] = 0.9 * ATOL
    compare_with_ref(got, reused, want, marg)
    got[11, 4, 2] = 1.1 * ATOL
    with pytest.raises(AssertionError):
        compare_with_ref(got, reused, want, marg)
    # a tighter tolerance given by the caller is the one applied
    got, want, marg, reused = _case()
    got[..., :3] = _off_by(want[..., :3], 0.9)
    with pytest.raises(AssertionError):
        compare_with_ref(got, reused, want, marg, rtol=0.5 * RTOL, atol=0.5 * ATOL)


def test_compare_with_ref_looks_past_marginal_pixels_only():
    got, want, marg, reused = _case()
    got[2, 3] = (9.0, 9.0, 9.0, 1.0)                                         # marginal: the device may decide otherwise
    compare_with_ref(got, reused, want, marg)
    marg[2, 3] = False
    with pytest.raises(AssertionError):
        compare_with_ref(got, reused, want, marg)


def test_compare_with_ref_rejects_another_sample_count():
    got, want, marg, reused = _case()
    got[9, 9, 3] += 1
    with pytest.raises(AssertionError):
        compare_with_ref(got, reused, want, marg)


def test_compare_with_ref_rejects_a_reused_count_past_the_marginal_share():
    got, want, marg, reused = _case()
    for off in (3, -3):                                                      # one more than the two marginal pixels allow
        with pytest.raises(AssertionError):
            compare_with_ref(got, reused + off, want, marg)
    with pytest.raises(AssertionError):
        compare_with_ref(got, reused + 1, want, np.zeros_like(marg))         # no marginal pixel: the counts must be equal


# ------------------------------------------------------------------------------------------------------------------------ assert_same
def _state():
    return {"t": np.array([0.5, 1.25, 0.0], np.float32), "face": np.array([3, -1, 7], np.int32), "pos": np.array([[1.0, -2.0], [0.0, 1e-30]])}


def test_assert_same_passes_on_equal_dicts_and_honours_skip():
    a, b = _state(), _state()
    assert_same(a, b)
    b["pos"][0, 1] = 9.0
    assert_same(a, b, skip=("pos",))
    with pytest.raises(AssertionError):
        assert_same(a, b, skip=("t",))
    del b["pos"]
    with pytest.raises(AssertionError):                                      # the two sides hold the same keys
        assert_same(a, b)


@pytest.mark.parametrize("key", ["t", "pos"])
def test_assert_same_names_the_key_that_is_one_ulp_off(key):
    a, b = _state(), _state()
    b[key].flat[1] = np.nextafter(b[key].flat[1], b[key].dtype.type(0))
    with pytest.raises(AssertionError) as e:
        assert_same(a, b)
    assert e.value.args[0].split("\n")[0] == key
    assert_same(a, b, skip=(key,))


def test_assert_same_names_the_key_whose_zero_changed_its_sign():
    a, b = _state(), _state()
    b["pos"][1, 0] = -0.0
    assert np.array_equal(a["pos"], b["pos"])                                # by value they are equal
    with pytest.raises(AssertionError) as e:
        assert_same(a, b)
    assert e.value.args[0].split("\n")[0] == "pos"


# ------------------------------------------------------------------------------------------------------------------------ assert_records
def test_assert_records_names_the_first_differing_record_and_the_count():
    want = np.random.default_rng(6).normal(size=(40, 3))
    assert_records(want.copy(), want, "vertex")
    assert_records(want.copy(), want.tolist(), "vertex")                     # the restatement's side may be a list
    got = want.copy()
    got[17, 2] = np.nextafter(got[17, 2], 0.0); got[30, 0] = -got[30, 0]; got[31] += 1.0
    with pytest.raises(AssertionError) as e:
        assert_records(got, want, "vertex")
    msg = e.value.args[0]
    assert msg.startswith("vertex 17 of 3 differing") and repr(got[17].tolist()) in msg and repr(want[17].tolist()) in msg


# ------------------------------------------------------------------------------------------------------------------------ c_layout
def test_c_layout_tells_a_class_with_two_fields_swapped_from_the_headers_struct(pkg, tmp_path):
    class Swapped(C.Structure):                                              # pkg.SkinInfo with `updates` and `last_ms` in each other's place
        _fields_ = [("struct_size", C.c_uint32), ("n_bones", C.c_uint32), ("last_ms", C.c_double), ("reserved0", C.c_uint32), ("updates", C.c_uint32),
                    ("reserved", C.c_uint32 * 4)]

    c, py, macros = c_layout(pkg.SkinInfo, "mcpt_skin_info", tmp_path, macros=("MCPT_SKIN_INFLUENCES", "MCPT_SKIN_DUAL_QUATERNION"))
    assert c == py and macros == [4, 1]
    c2, py2, _ = c_layout(Swapped, "mcpt_skin_info", tmp_path)
    assert c2 != py2 and c2[0] == py2[0] == c[0]                             # the same size: only the offsets give it away
    assert sorted(c2) == sorted(c)                                           # (the header's side is the real struct, asked in the class's order)
