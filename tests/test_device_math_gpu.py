"""The device's shading arithmetic, one function call per case (hiprz_selftest_math: the RZ_* macros and RZ_DEV functions of
hiprz_device.hpp, called themselves), held to the references of tests/math_reference.py.

  * library calls: error in float32 steps at the float64 value, per function and band, against BAR = 1.5 (sqrtf, `/` and the texture wrap:
    bit-equal to numpy float32; cosf, asinf, atan2f and logf: the step count measured, BARS below).  With -s every test prints its rows;
    profiles/r20/device_math.txt is that table.
  * sincosf returns what sinf and cosf return, bit for bit, on every band.
  * arithmetic-only primitives: bit-equal to the numpy float32 re-derivations, fresnel also to the oracle's export.
  * tone map (hiprz_tonemap_image): bit-equal to the oracle's pixel wherever the conversion to a byte is defined.
  * samplers and the glossy lobe: at most twice the error of the oracle and its one-ulp stand-ins against float64, on the same cases.
  * sample_direction against the reference's formulas spelled with the separate functions: every output bit for bit, every path reached."""
import numpy as np
import pytest

import math_reference as M
import oracle
from rayzath_amd import _hiprt, scenes
from rayzath_amd.engine import Context
from rayzath_amd.scene import camera_struct, flatten

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32

# Functions measured beyond BAR on the device (profiles/r20/device_math.txt: cosf 1.5243, asinf 2.5319, atan2f 2.4475, logf 1.8729 float
# steps at the true value): held to the integer step count found — the result is 2, 3, 2 and 2 steps from the correctly rounded value —
# plus 0.5.  Device libm is deterministic, so there is no noise margin; what this means for the one-ulp stand-ins is DESIGN.md §2's.
BARS = {"cosf": 2.5 + 1.0e-6, "asinf": 3.5 + 1.0e-6, "atan2f": 2.5 + 1.0e-6, "logf": 2.5 + 1.0e-6}


@pytest.fixture(scope="module")
def ctx(built):
    world = scenes.cornell_box(64, 64)
    c = Context(0)
    c.upload_scene(flatten(world))
    c.upload_camera(camera_struct(world.camera))
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(built):
    from rayzath_amd import _abi, _lib
    params = _abi.DenoiseParams()
    _lib.load().hiprz_denoise_default_params(params)
    return M.arguments(1 << 20, sigma_normal=params.sigma_normal)


def device(ctx, op):
    return lambda *a: ctx.selftest_math(op, np.stack([np.asarray(x, f32) for x in a], 1))


@pytest.mark.parametrize("function", M.FUNCTIONS)
def test_library_call(ctx, sets, function):
    evaluate = device(ctx, function)
    rows = M.judge_function(function, lambda *a: evaluate(*a)[:, 0], sets, glibc_every=16, bar=BARS.get(function, M.BAR))
    print()
    for r in rows:
        print(r.text())
    assert not [f for r in rows for f in r.failures]


def test_sincosf_is_sinf_and_cosf(ctx, sets):
    """on every band of the angles, not on random angles only (hiprz_selftest draws those)"""
    print()
    for band, (x,) in sets["sinf"]:
        both, s, c = device(ctx, "sincosf")(x), device(ctx, "sinf")(x)[:, 0], device(ctx, "cosf")(x)[:, 0]
        ds, dc = ~M.same_bits_or_nan(both[:, 0], s), ~M.same_bits_or_nan(both[:, 1], c)
        print(f"sincosf  {band:<34} {x.size:>8} cases  sin differs {int(ds.sum())}  cos differs {int(dc.sum())}")
        assert not ds.any(), (band, x[ds][:4], both[ds][:4], s[ds][:4])
        assert not dc.any(), (band, x[dc][:4], both[dc][:4], c[dc][:4])
        assert both.shape == (x.size, 2)


def _bit_equal(name, kind, got, want):
    wrong = ~M.same_bits_or_nan(got, want).reshape(len(got), -1).all(1)
    print(f"{name:<26} {kind:<26} {len(got):>7} cases  differ {int(wrong.sum())}  NaN rows {int(np.isnan(want).reshape(len(got), -1).any(1).sum())}")
    i = int(np.argmax(wrong))
    assert not wrong.any(), f"{name} {kind}: {int(wrong.sum())} cases differ from the float32 re-derivation, first case {i}: got {got[i]!r}, want {want[i]!r}"


def test_arithmetic_primitives_are_bit_equal(ctx):
    rng = np.random.default_rng(20)
    print()
    normals = {"random": np.concatenate([M.random_units(rng, 1 << 16), M.random_units(rng, 1 << 12) * f32(0.5), M.random_units(rng, 1 << 12) * f32(2.0)]),
               "edges": M.edge_normals()}
    for kind, n in normals.items():
        _bit_equal("local_coordinate", kind, ctx.selftest_math("local_coordinate", n), np.concatenate(M.local_coordinate32(n), 1))
    tie = M.edge_normals()[6:11]
    assert (np.abs(tie[:, 0]) == np.abs(tie[:, 1])).all()
    assert (ctx.selftest_math("local_coordinate", tie)[:, 3:6] == np.cross(tie, [1.0, 0.0, 0.0]).astype(f32)).all()  # the tie takes vX = (1, 0, 0)
    L = oracle.load()
    for kind, c in M.fresnel_cases(rng, 1 << 14).items():
        got = ctx.selftest_math("fresnel", c)
        _bit_equal("fresnel", kind, got, M.fresnel32(c[:, 0:3], c[:, 3:6], c[:, 6], c[:, 7], c[:, 8], c[:, 9]))
        ref, fact = np.zeros((len(c), 3), f32), np.zeros(2, f32)
        for i, row in enumerate(np.ascontiguousarray(c)):
            fact[:] = row[8:10]
            ref[i, 0] = L.rzo_fresnel(row[0:3].ctypes.data, row[3:6].ctypes.data, float(row[6]), float(row[7]), fact.ctypes.data)
            ref[i, 1:] = fact
        _bit_equal("fresnel (oracle export)", kind, got, ref)
        total = M.total_reflection32(c[:, 0:3], c[:, 3:6], c[:, 6], c[:, 7])
        assert (got[total, 1] == 7.0).all() and (got[total, 2] == -9.0).all()  # total reflection leaves the factors untouched
        if kind == "edges":  # sin2_t on both sides of 1 among the neighbours of the critical cosine, and exactly on the boundary's floats
            crit = (c[:, 6] == 2.5) & (c[:, 7] == 1.0) & (np.abs(c[:, 5]) > 0.9) & (np.abs(c[:, 5]) < 0.93)
            assert total[crit].any() and (~total[crit]).any()
            counts = M.fresnel_boundary_counts(c)
            print(f"fresnel                    sin2_t at the last float below 1, at 1, at the first above: {counts} cases")
            assert min(counts) >= 2, counts
            below = M.bits(M.sin2_t32(c[:, 0:3], c[:, 3:6], c[:, 6], c[:, 7])) == M.bits(M.SIN2_T_BOUNDARY[0])
            assert not total[below].any() and (got[below, 1] == c[below, 6] / c[below, 7]).all()  # not total: cost = sqrt(2^-24), the factors are set
    att, nd = M.brdf_cases(rng, 1 << 16)
    for kind, c in att.items():
        _bit_equal("attenuation", kind, ctx.selftest_math("attenuation", c)[:, 0], M.attenuation32(c[:, 0], c[:, 1]))
    zero = ctx.selftest_math("attenuation", np.array([[0.0, 0.0]], f32))
    assert np.isnan(zero).all()  # 0 / 0
    for kind, c in nd.items():
        _bit_equal("ndf", kind, ctx.selftest_math("ndf", c)[:, 0], M.ndf32(c[:, 0:3], c[:, 3:6], c[:, 6]))
    for kind, c in M.vector_pair_cases(rng, 1 << 16).items():
        _bit_equal("reflect_vector", kind, ctx.selftest_math("reflect_vector", c), M.reflect_vector32(c[:, 0:3], c[:, 3:6]))
        _bit_equal("halfway_vector", kind, ctx.selftest_math("halfway_vector", c), M.halfway_vector32(c[:, 0:3], c[:, 3:6]))


def test_entry_point_refusals_with_a_context(ctx):
    """what hiprz_selftest_math refuses behind its context check: reached only with a live context.  Nothing is launched for any of
    these, and `out` stays as it was."""
    from rayzath_amd import _abi
    lib, c = ctx.lib, ctx._ctx
    inp, out = np.full(8, 0.5, f32), np.full(8, 9.0, f32)
    call = lambda op, i, w_in, n, o, w_out: lib.hiprz_selftest_math(c, op, i, w_in, n, o, w_out)
    assert call(0, None, 1, 4, out.ctypes.data, 1) == _abi.ERR_INVALID
    assert call(0, inp.ctypes.data, 1, 4, None, 1) == _abi.ERR_INVALID
    assert call(0, None, 1, 0, None, 1) == _abi.ERR_INVALID           # a null pointer is refused with no cases too
    assert call(len(_abi.MATH_OPS), inp.ctypes.data, 1, 4, out.ctypes.data, 1) == _abi.ERR_INVALID
    assert call(0xFFFFFFFF, inp.ctypes.data, 1, 4, out.ctypes.data, 1) == _abi.ERR_INVALID
    assert call(0, inp.ctypes.data, 2, 4, out.ctypes.data, 1) == _abi.ERR_INVALID   # sinf takes rows of 1
    assert call(0, inp.ctypes.data, 1, 4, out.ctypes.data, 2) == _abi.ERR_INVALID   # ... and returns rows of 1
    assert call(2, inp.ctypes.data, 1, 4, out.ctypes.data, 1) == _abi.ERR_INVALID   # sincosf returns rows of 2
    assert call(0, inp.ctypes.data, 1, (1 << 24) + 1, out.ctypes.data, 1) == _abi.ERR_INVALID  # refused before a byte is read
    assert b"selftest_math" in lib.hiprz_last_error(c)
    assert call(0, inp.ctypes.data, 1, 0, out.ctypes.data, 1) == _abi.OK      # no cases: no launch
    assert (out == 9.0).all() and (inp == 0.5).all()
    assert call(0, inp.ctypes.data, 1, 8, out.ctypes.data, 1) == _abi.OK      # and the context still works
    assert M.same_bits_or_nan(out, ctx.selftest_math("sinf", inp)[:, 0]).all() and (out != 9.0).all()
    with pytest.raises(ValueError):
        ctx.selftest_math("powf", inp)


def tonemap32(rgba, aperture, exposure_time):
    """cpu_engine_renderer.cpp:224-235 in numpy float32, up to the product with 255 (the conversion to a byte is the caller's)"""
    rgba = np.asarray(rgba, f32)
    with np.errstate(all="ignore"):
        area = f32(aperture) * f32(aperture) * M.PI_F
        c = rgba * (f32(1.0) / np.where(rgba[:, 3:4] == 0, f32(1.0), rgba[:, 3:4]))
        c = ((c * area) * f32(exposure_time)) * f32(1.0e5)
        c = c / (c + f32(1.0))
        return (c[:, :3] * f32(255.0)).astype(f32)


def test_tonemap_is_the_oracles(ctx):
    rng = np.random.default_rng(5)
    cam = camera_struct(scenes.cornell_box(64, 64).camera)
    n = cam.width * cam.height
    rgb = np.concatenate([M.mixture(rng, 0.0, 1.0e6, 3 * (n - 64)).reshape(-1, 3), M.signed(rng, M.mixture(rng, 0.0, 1.0e3, 3 * 32)).reshape(-1, 3),
                          np.array([[np.inf, 1.0, 0.0], [np.nan, 0.5, 1.0], [-1.0, -0.0, 3.0e38], [0.0, 0.0, 0.0]] * 8, f32)])
    alpha = np.concatenate([rng.choice(np.array([0.0, 1.0, 3.0, 64.0, 1.0e-3], f32), n - 32), np.array([0.0, -1.0, np.inf, 1.0e-30] * 8, f32)])
    rgba = np.concatenate([rgb, alpha[:, None]], 1).astype(f32)
    # cases that land on and around whole bytes: colour x with x / (x + 1) * 255 near k, scaled back through the exposure
    scale = float(f32(cam.aperture) * f32(cam.aperture) * M.PI_F) * float(cam.exposure_time) * 1.0e5
    k = np.arange(0, 255, dtype=np.float64)
    rgba[:255, 0] = (k / (255.0 - k) / scale).astype(f32)
    rgba[:255, 3] = 1.0
    src, dst = _hiprt.DeviceBuffer.of(rgba), _hiprt.DeviceBuffer(4 * n)
    try:
        ctx.tonemap_image(src.ptr, dst.ptr)
        ctx.sync()
        got = dst.download((n, 4), np.uint8)
    finally:
        src.free(), dst.free()
    assert (got[:, 3] == 255).all()
    value = tonemap32(rgba, cam.aperture, cam.exposure_time).astype(np.float64)
    defined = ((value >= 0) & (value < 256)).all(1)  # NaN compares false: outside
    L, ref = oracle.load(), np.zeros((n, 4), np.uint8)
    for i in np.flatnonzero(defined):
        L.rzo_tonemap_pixel(rgba[i].ctypes.data, cam.aperture, cam.exposure_time, ref[i].ctypes.data)
    print(f"\ntonemap  {n} cases, {int(defined.sum())} with every colour * 255 in [0, 256), bytes 0..{got[defined, :3].max()}")
    assert defined.sum() > n - 200 and (~defined).sum() >= 24
    wrong = defined & (got != ref).any(1)
    assert not wrong.any(), (rgba[wrong][:4], got[wrong][:4], ref[wrong][:4])
    assert (got[defined, :3] == np.trunc(value[defined]).astype(np.uint8)).all()
    assert len(np.unique(got[:255, 0])) > 200  # the bytes' boundaries were exercised


N_SAMPLER = 1 << 13  # random cases per primitive through the oracle's scalar exports (four libraries each)


@pytest.mark.parametrize("name", list(M.SAMPLERS))
def test_sampler_error_is_within_twice_the_oracles(ctx, name):
    rng = np.random.default_rng(9)
    print()
    for kind, cases in M.sampler_cases_of(name, rng, N_SAMPLER).items():
        assert len(cases) >= 256, kind
        bar, plain, oracle_nan = M.sampler_bar(oracle, name, cases)
        out = ctx.selftest_math(name, cases)
        for label, got in (("", out[:, :M.SAMPLERS[name][2]]),) + ((("as sample_direction", out[:, 2:4]),) if name == "glossy_lobe" else ()):
            err, nan = M.sampler_errors(name, cases, got)
            print(f"{name:<26} {kind:<26} {label:<20}{len(cases):>6} cases  device {err}  plain oracle {plain}  bar {bar}  NaN {int(nan.sum())} (oracles {int(oracle_nan.sum())})")
            assert (err <= bar).all(), f"{name} {kind} {label}: device {err} beyond twice the oracle's and its stand-ins' {bar}"
            assert not (nan & ~oracle_nan).any(), f"{name} {kind} {label}: NaN where no oracle library returns one: {cases[nan & ~oracle_nan][:4]}"
        if name == "glossy_lobe":
            mirror = cases[:, 1] == 0
            assert mirror.sum() >= 2 * len(M.EDGE_DRAWS) or kind != "edges"
            # a mirror's lobe is (+0, 1) on both routes, bit for bit; every other roughness runs the same sequence on both
            assert (M.bits(out[mirror]) == M.bits(np.array([0.0, 1.0, 0.0, 1.0], f32))).all()
            assert M.same_bits_or_nan(out[:, 0:2], out[:, 2:4]).all()
            tiny = M.bits(cases[:, 1]) == M.bits(f32(2.0 ** -100))
            assert (M.bits(out[tiny]) == M.bits(np.array([0.0, 1.0, 0.0, 1.0], f32))).all()


MIN_CASES = 256  # of every path, and of every roughness edge on the glossy path


@pytest.mark.parametrize("which", ["random", "grid"])
def test_sample_direction_is_its_parts(ctx, which):
    rng = np.random.default_rng(11)
    cases = M.direction_cases_random(rng, 1 << 18) if which == "random" else M.direction_cases_grid(rng)
    out = ctx.selftest_math("sample_direction", cases)
    merged, parts, word = M.direction_sides(out)
    path, flipped = word & 7, (word & 8) != 0
    names = ("direction x", "direction y", "direction z", "tint_factor", "ray material", "normal x", "normal y", "normal z", "generator a", "generator b")
    differ = merged != parts
    print(f"\nsample_direction {which}: {len(cases)} cases, differing words per output {dict(zip(names, differ.sum(0).tolist()))}")
    for k in range(5):
        print(f"  {M.PATHS[k]:<20} {int((path == k).sum()):>7} cases, {int(((path == k) & flipped).sum()):>6} flipped")
    i = int(np.argmax(differ.any(1)))
    assert not differ.any(), f"case {i} {cases[i]!r}: sample_direction {out[i, :10]!r}, its parts {out[i, 10:20]!r}, path {word[i]}"
    assert (path == M.direction_path(cases)).all(), "a draw was taken or skipped: the device took another path than the case's generator says"
    assert not (flipped & (path < 2)).any()
    # the generator's final state: one draw for refraction and reflection, two for scattering, three for diffuse and glossy
    a, b = M.rng_make(cases[:, 0], cases[:, 1], cases[:, 2])
    for draws in (1, 2, 3):
        a, b, _ = M.rng_draw(a, b)
        took = np.isin(path, {1: (1, 2), 2: (0,), 3: (3, 4)}[draws])
        assert (M.bits(out[took, 8]) == M.bits(a[took])).all() and (M.bits(out[took, 9]) == M.bits(b[took])).all(), f"{draws} draws"
    # tint factor and ray material per path
    assert (out[path == 1, 3] == 1.0).all() and (out[path == 3, 3] == 1.0).all() and (out[np.isin(path, (0, 2, 4)), 3] == cases[np.isin(path, (0, 2, 4)), 7]).all()
    assert (M.bits(out[path == 1, 4]) == M.bits(cases[path == 1, 21])).all() and (M.bits(out[path != 1, 4]) == M.bits(cases[path != 1, 20])).all()
    assert (out[path == 1, 5:8] == -cases[path == 1, 9:12]).all()
    for k in range(5):
        assert (path == k).sum() >= MIN_CASES, M.PATHS[k]
    for r in M.ROUGHNESS_EDGES:
        assert ((path == 4) & (M.bits(cases[:, 8]) == M.bits(r))).sum() >= MIN_CASES, f"glossy at roughness {r!r}"
    if which == "random":  # (the grid's mapped normal is its normal: nothing ends below the surface there but by rounding)
        for k in (2, 3, 4):
            assert ((path == k) & flipped).sum() >= MIN_CASES and ((path == k) & ~flipped).sum() >= MIN_CASES, f"{M.PATHS[k]}: the flip"
