"""The harness of tests/math_reference.py without a GPU: glibc's float functions meet every bar the device is held to, the oracle's
composed exports meet the factor-two rule, two deliberately poor substitutes are caught (a test that cannot fail proves nothing), the case
sets of sample_direction reach every path, and hiprz_selftest_math refuses bad arguments before it needs a context."""
import ctypes as C

import numpy as np
import pytest

import math_reference as M
import oracle

f32 = np.float32
N = 1 << 16  # random arguments per band here (glibc is called through ctypes, one call per argument); the device test takes 2^20


@pytest.fixture(scope="module")
def sets():
    return M.arguments(N)


def test_the_metric():
    assert M.ulp32(1.0) == 2.0 ** -23 and M.ulp32(0.999) == 2.0 ** -24 and M.ulp32(0.0) == 2.0 ** -149 and M.ulp32(-3.0) == 2.0 ** -22
    assert M.ulp32(2.0 ** -126) == 2.0 ** -149 and M.ulp32(2.0 ** -125) == 2.0 ** -148
    # one float step from the correctly rounded value is below the bar, two steps are not
    x = np.array([0.3], f32)
    want = np.sin(x.astype(np.float64))
    near = want.astype(f32)
    assert M.error_ulps(near, want) <= 0.5
    assert M.error_ulps(M.from_bits(M.bits(near) + np.uint32(1)), want) < M.BAR < M.error_ulps(M.from_bits(M.bits(near) + np.uint32(2)), want)


@pytest.mark.parametrize("function", M.FUNCTIONS)
def test_glibc_meets_every_bar(sets, function):
    rows = M.judge_function(function, M.glibc(function), sets)
    for r in rows:
        print(r.text())
    assert not [f for r in rows for f in r.failures]
    assert all(r.cases > 0 for r in rows if not r.band.startswith("subnormal quotients"))


def test_every_band_is_there(sets):
    """the bands the bars are applied to: the NaN band, the subnormal results and the exact zeros are reached"""
    rows = {(r.function, r.band): r for fn in ("acosf", "expf", "div", "wrap", "powf") for r in M.judge_function(fn, M.glibc(fn), sets)}
    assert rows[("acosf", "above 1: NaN")].cases == 64
    assert rows[("expf", "[-100, 0] subnormal")].cases > 1000 and rows[("div", "subnormal quotients subnormal")].cases > 60000
    assert rows[("powf", "medium subnormal")].cases > 1000
    u = np.array([-2.0 ** -30], f32)
    assert M.EXACT["wrap"](u)[0] == 0.0  # the + 1.0f rounds to 1 there, and the outer fmodf gives 0


def poor_powf(x, y):
    """float32 exp(y * log(x)): the product carries log's rounding, scaled by |y log x|, into the exponent"""
    with np.errstate(all="ignore"):
        return np.exp((np.asarray(y, f32) * np.log(np.asarray(x, f32))).astype(f32)).astype(f32)


def poor_acosf(x):
    """float32 atan2(sqrt(1 - x x), x): 1 - x x cancels towards +-1"""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        return np.arctan2(np.sqrt(f32(1.0) - x * x), x).astype(f32)


@pytest.mark.parametrize("function,substitute", [("powf", poor_powf), ("acosf", poor_acosf)])
def test_a_poor_substitute_is_caught(sets, function, substitute):
    rows = M.judge_function(function, substitute, sets)
    failures = [f for r in rows for f in r.failures]
    print("\n".join(r.text() for r in rows))
    assert failures, f"the harness passes {substitute.__name__}"
    assert max(r.max_ulps for r in rows if "subnormal" not in r.band) > 4.0


@pytest.mark.parametrize("name", list(M.SAMPLERS))
def test_oracle_exports_meet_the_factor_two_rule(built, name):
    """the plain oracle against twice the largest error among itself and its stand-ins: holds by construction of the bar, and shows that
    every library has the export, that the float64 formulas are the oracle's (errors of a few float steps, not of another formula) and
    that the stand-ins do differ from the plain oracle"""
    rng = np.random.default_rng(7)
    for kind, cases in M.sampler_cases_of(name, rng, 1 << 11).items():
        bar, plain, nan = M.sampler_bar(oracle, name, cases)
        print(f"{name:<26} {kind:<26} {len(cases):>6} cases  plain oracle {plain}  bar {bar}")
        assert (plain <= bar).all()
        scale = 4.0 if name == "sample_disk" else 1.0  # radius up to 2, a frame of a normal of length 2
        assert (bar < 1.0e-2 * scale).all(), "the float64 formula is not the oracle's"
        assert (bar > 0).any() and len(cases) >= 64
        if kind == "random" and name != "sample_disk":  # away from the steep arc cosine the errors are a few float steps of 1
            assert (bar < 4.0e-6).all(), bar
        moved = M.oracle_sampler(oracle.variant("hi"), name, cases)
        assert not np.array_equal(moved, M.oracle_sampler(oracle.load(), name, cases), equal_nan=True)


def test_rederivations_are_the_oracles(built):
    """fresnel32 against rzo_fresnel bit for bit, untouched factors included: the numpy spelling the device is held to is the oracle's"""
    L = oracle.load()
    rng = np.random.default_rng(3)
    sets_ = M.fresnel_cases(rng, 2048)
    total = 0
    for kind, cases in sets_.items():
        want = M.fresnel32(cases[:, 0:3], cases[:, 3:6], cases[:, 6], cases[:, 7], cases[:, 8], cases[:, 9])
        got = np.zeros((len(cases), 3), f32)
        fact = np.zeros(2, f32)
        for i, c in enumerate(np.ascontiguousarray(cases)):
            fact[:] = c[8:10]
            got[i, 0] = L.rzo_fresnel(c[0:3].ctypes.data, c[3:6].ctypes.data, float(c[6]), float(c[7]), fact.ctypes.data)
            got[i, 1:] = fact
        assert M.same_bits_or_nan(got, want).all(), kind
        total += int(M.total_reflection32(cases[:, 0:3], cases[:, 3:6], cases[:, 6], cases[:, 7]).sum())
    edges = sets_["edges"]
    assert total > 100 and (edges[:, 6] == edges[:, 7]).any()  # total reflection and n1 == n2 are both there
    counts = M.fresnel_boundary_counts(edges)  # sin2_t exactly at the last float below 1, at 1 and at the first float above
    assert min(counts) >= 2, counts


MIN_CASES = 256  # of every path of sample_direction, in the random set and in the grid


def test_direction_cases_reach_every_path():
    rng = np.random.default_rng(11)
    for cases in (M.direction_cases_random(rng, 1 << 18), M.direction_cases_grid(rng)):
        assert cases.shape[1] == 22 and cases.dtype == f32
        path = M.direction_path(cases)
        for k in range(5):
            assert (path == k).sum() >= MIN_CASES, M.PATHS[k]
        for r in M.ROUGHNESS_EDGES:
            assert ((path == 4) & (M.bits(cases[:, 8]) == M.bits(r))).sum() >= MIN_CASES, f"glossy at roughness {r!r}"
        # the generator's first product stays inside int32 (Rng truncates through an int)
        a, b = M.rng_make(cases[:, 0], cases[:, 1], cases[:, 2])
        assert np.abs((a + f32(0.2311362)) * (b + f32(13.054377))).max() < 2.0 ** 31


WIDTHS = [(1, 1), (1, 1), (1, 2), (1, 1), (1, 1), (2, 1), (2, 1), (1, 1), (1, 1), (1, 1), (2, 1), (1, 1), (3, 6), (5, 3), (5, 3), (5, 3), (6, 3),
          (10, 3), (7, 1), (2, 1), (6, 3), (6, 3), (2, 4), (22, 21)]


def test_entry_point_refuses_bad_arguments(built):
    """hiprz_selftest_math without a context (none can exist without a GPU): refused, nothing written; the row widths of every op, and
    the refusal of an unknown one"""
    from rayzath_amd import _abi, _lib
    lib = _lib.load()
    assert len(_abi.MATH_OPS) == len(WIDTHS)
    a, b = C.c_uint32(77), C.c_uint32(78)
    for op, (w_in, w_out) in enumerate(WIDTHS):
        assert lib.hiprz_selftest_math_widths(op, C.byref(a), C.byref(b)) == _abi.OK and (a.value, b.value) == (w_in, w_out), _abi.MATH_OPS[op]
    a, b = C.c_uint32(77), C.c_uint32(78)
    for op in (len(WIDTHS), 0xFFFFFFFF):
        assert lib.hiprz_selftest_math_widths(op, C.byref(a), C.byref(b)) == _abi.ERR_INVALID
    assert lib.hiprz_selftest_math_widths(0, None, C.byref(b)) == _abi.ERR_INVALID
    assert lib.hiprz_selftest_math_widths(0, C.byref(a), None) == _abi.ERR_INVALID
    assert (a.value, b.value) == (77, 78)
    inp, out = np.full(4, 0.5, f32), np.full(4, 9.0, f32)
    assert lib.hiprz_selftest_math(None, 0, inp.ctypes.data, 1, 4, out.ctypes.data, 1) == _abi.ERR_INVALID
    assert lib.hiprz_selftest_math(None, 0, None, 1, 0, None, 1) == _abi.ERR_INVALID
    assert (out == 9.0).all()
