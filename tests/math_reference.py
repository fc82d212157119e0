"""float64 references, the error metric and the argument sets for the device's shading arithmetic (hiprz_selftest_math, include/hiprz.h).
TEST INFRASTRUCTURE ONLY.  tests/test_math_reference.py runs this harness against glibc and the oracle without a GPU,
tests/test_device_math_gpu.py against the device.

THE METRIC is the real-valued error in units of the float32 step at the true value: |got - want64| / ulp32(want64), both sides in float64.
Not "steps from the float64 result rounded to float": a double that lies within its own error of a rounding tie sends that reference one
step the wrong way, and over millions of cases that happens.  A result within one float step of the correctly rounded value has an error
below 1.5: that is BAR.  Its slack is 1e-6 ulp — a double libm result is good to about one double ulp, 2^-29 float ulps.
  * want64 NaN or infinite: the same class (and sign of the infinity) is required.
  * |want64| < 2^-126: the rule is absolute, |got - want64| <= 2^-126 (every oracle comparison is relative to max(|ref|, 1), where such a
    value cannot matter); a flushed subnormal is counted, not failed.  These cases form a row of their own ("<band> subnormal").
  * want64 zero: the result is that zero, sign included (sinf(-0), atan2f(-0, x > 0), powf(0, y)).
  * sqrtf, `/` and the texture wrap are exact: bit-equal to numpy float32 (and so within 0.5).

THE ARGUMENT SETS are what the integrator produces, band by band (arguments() below cites the call sites): per band n stratified random
arguments — half uniform in value, half uniform on the bit patterns between the ends, so that small magnitudes are not starved — plus the
listed edges."""
import ctypes as C

import numpy as np

f32, f64, u32 = np.float32, np.float64, np.uint32
BAR = 1.5 + 1.0e-6
TINY = 2.0 ** -126
FLT_MAX = f32(3.402823466e+38)
PI_F = f32(3.14159265358979323846)
TWO_PI_F = f32(6.283185)  # the samplers' own constant (cpu_render_utils.cpp:85-119), not 2 * pi rounded


def bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(u32)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=u32).view(f32)


def ulp32(x):
    """the float32 step at the real value x: 2^(floor(log2 |x|) - 23), the subnormal step 2^-149 below 2^-126"""
    with np.errstate(invalid="ignore"):
        m, e = np.frexp(np.abs(np.asarray(x, f64)))
    return np.ldexp(1.0, np.clip(np.where(m == 0, -126, e - 1), -126, 127) - 23)  # (frexp(0) = (0, 0))


def error_ulps(got, want64):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(np.asarray(got, f64) - want64) / ulp32(want64)


def same_bits_or_nan(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# library calls: references, glibc, argument sets
# ---------------------------------------------------------------------------------------------------------------------------------
def _d(*a):
    return [np.asarray(x, f32).astype(f64) for x in a]


def _wrap32(u):
    u = np.asarray(u, f32)
    return np.fmod(np.fmod(u, f32(1.0)) + f32(1.0), f32(1.0)).astype(f32)  # fmod is exact in every format: numpy's float32 is the answer


def _div32(a, b):
    with np.errstate(all="ignore"):
        return np.asarray(a, f32) / np.asarray(b, f32)


REFERENCE = {  # float64, on the float32 arguments
    "sinf": lambda x: np.sin(*_d(x)), "cosf": lambda x: np.cos(*_d(x)), "acosf": lambda x: np.arccos(*_d(x)),
    "asinf": lambda x: np.arcsin(*_d(x)), "atan2f": lambda y, x: np.arctan2(*_d(y, x)), "powf": lambda x, y: np.power(*_d(x, y)),
    "expf": lambda x: np.exp(*_d(x)), "logf": lambda x: np.log(*_d(x)), "sqrtf": lambda x: np.sqrt(*_d(x)),
    "div": lambda a, b: np.divide(*_d(a, b)), "wrap": lambda u: _wrap32(u).astype(f64),
}
EXACT = {  # bit-equal to numpy float32
    "sqrtf": lambda x: np.sqrt(np.asarray(x, f32)), "div": lambda a, b: _div32(a, b), "wrap": _wrap32,
}
FUNCTIONS = ("sinf", "cosf", "acosf", "asinf", "atan2f", "powf", "expf", "logf", "sqrtf", "div", "wrap")

_libc = None


def glibc(name):
    """the C library's float function `name` as a function of float32 arrays (ctypes on the library that is already loaded)"""
    global _libc
    if _libc is None:
        _libc = C.CDLL(None)
    if name == "div":
        return EXACT["div"]
    if name == "wrap":
        fmodf = getattr(_libc, "fmodf")
        fmodf.restype, fmodf.argtypes = C.c_float, [C.c_float, C.c_float]
        return lambda u: np.array([fmodf(f32(fmodf(v, 1.0)) + f32(1.0), 1.0) for v in np.asarray(u, f32).tolist()], f32)
    fn = getattr(_libc, name)
    n_args = 2 if name in ("atan2f", "powf") else 1
    fn.restype, fn.argtypes = C.c_float, [C.c_float] * n_args
    return lambda *a: np.fromiter(map(fn, *[np.asarray(x, f32).tolist() for x in a]), dtype=f32, count=len(a[0]))


def mixture(rng, lo, hi, n):
    """n float32 in [lo, hi], 0 <= lo < hi: half stratified uniform in value, half stratified uniform on the bit patterns between"""
    lo, hi = f32(lo), f32(hi)
    k = n // 2
    v = (f64(lo) + (np.arange(k) + rng.random(k)) / k * (f64(hi) - f64(lo))).astype(f32)
    b0, b1 = int(bits(lo).ravel()[0]), int(bits(hi).ravel()[0])
    b = from_bits((b0 + (np.arange(n - k) + rng.random(n - k)) / (n - k) * (b1 - b0)).astype(u32))
    return np.clip(np.concatenate([v, b]), lo, hi).astype(f32)


def signed(rng, x):
    return np.where(rng.random(x.size) < 0.5, -x, x).astype(f32)


def neighbours(x, k):
    """the 2k + 1 floats within k steps of x (x != 0, finite; no step crosses zero)"""
    return from_bits((int(bits(f32(x)).ravel()[0]) + np.arange(-k, k + 1)).astype(u32))


def unit_draws(rng, n):
    """draws of Rng::unsignedUniform: [0, 1) — stratified in value and on bit patterns — with the ends 0, 2^-24 and 1 - 2^-24"""
    return np.concatenate([mixture(rng, 0.0, 1.0 - 2.0 ** -24, n), np.array([0.0, 2.0 ** -24, 1.0 - 2.0 ** -24], f32)])


def arguments(n=1 << 20, seed=20, sigma_normal=None):
    """{function: [(band, (argument arrays ...)), ...]}.  The call sites, all in rayzath_amd/csrc:
    sincosf  hiprz_device.hpp: cosine_sample_hemisphere, sample_sphere, sample_direction (phi = r1 * 6.283185f), sample_disk and
             generate_antialiased_ray (r * 2 * pi), sample_sphere and glossy_lobe (theta = an acosf result)
    acosf    sample_sphere (1 - 2 * r2), glossy_lobe (its argument passes 1 when powf(u2 + 1e-5, roughness) > 1)
    asinf, atan2f  hiprz_kernels.hpp, the sky's texture coordinates: asinf(d.y), atan2f(d.z, d.x) of a normalised direction
    powf     glossy_lobe (u2 + 1e-5, roughness); hiprz_kernels.hpp: powf(medium.a, ray.far_); hiprz_denoise_kernels.hpp: powf(max(0, n.n'), sigma_normal)
    expf     direct_illumination: expf(-dPL * scattering); hiprz_denoise_kernels.hpp: the depth, colour and luminance weights
    logf     hiprz_kernels.hpp: -logf(draw + 1e-4) / sigma
    sqrtf, / everywhere (normalized, the samplers, the intersection tests)
    wrap     texel_offset: fmodf(fmodf(u, 1) + 1, 1)"""
    rng = np.random.default_rng(seed)
    sets = {}
    half_pi = [f32(k * np.pi / 2) for k in (1, 2, 3, 4)]
    angles = [("[0, 2 pi]", (np.concatenate([mixture(rng, 0.0, TWO_PI_F, n // 2), unit_draws(rng, n // 2) * TWO_PI_F]),)),
              ("[0, pi]", (mixture(rng, 0.0, PI_F, n),)),
              ("k pi/2 and zeros", (np.concatenate([neighbours(h, 4) for h in half_pi] + [np.array([0.0, -0.0], f32)]),))]
    sets["sinf"] = sets["cosf"] = angles
    r2 = unit_draws(rng, n)
    sets["acosf"] = [("1 - 2 r2", (f32(1.0) - f32(2.0) * r2,)),
                     ("above 1: NaN", (neighbours(1.0, 64)[65:],)),
                     ("near -1, 0, 1", (np.concatenate([neighbours(-1.0, 1 << 15), from_bits(np.arange(1 << 15)), -from_bits(np.arange(1 << 15)),
                                                        neighbours(1.0, 1 << 15)]),))]
    one_up = neighbours(1.0, 1)[2]
    sets["asinf"] = [("[-1, 1]", (signed(rng, mixture(rng, 0.0, 1.0, n)),)),
                     ("+-1 and a step beyond", (np.array([1.0, -1.0, one_up, -one_up, 0.0, -0.0], f32),))]
    ax = np.array([1.0, 0.5, 2.0 ** -24, 1.0e-30], f32)
    zeros = np.array([0.0, 0.0, -0.0, -0.0], f32), np.array([0.0, -0.0, 0.0, -0.0], f32)
    sets["atan2f"] = [("[-1, 1]^2", (signed(rng, mixture(rng, 0.0, 1.0, n)), signed(rng, rng.permutation(mixture(rng, 0.0, 1.0, n))))),
                      ("zeros and axes", (np.concatenate([zeros[0], np.tile(np.array([0.0, -0.0], f32), 8), ax, -ax, ax, -ax]),
                                          np.concatenate([zeros[1], np.repeat(np.concatenate([ax, -ax]), 2), np.repeat(np.array([0.0, -0.0], f32), 8)])))]
    edge_y = np.array([0.0, -0.0, 2.0 ** -100, 1.0], f32)
    lobe_x = mixture(rng, 1.0e-5, 1.00001, n)
    lobe_edges_x = np.concatenate([EDGE_DRAWS + f32(1.0e-5), np.array([1.0], f32)])
    medium_x = np.concatenate([mixture(rng, 0.0, 1.0, n - 2), np.array([0.0, 1.0], f32)])
    medium_y = np.concatenate([mixture(rng, 0.0, 1.0e3, n - 64), np.full(64, FLT_MAX, f32)])
    sigma = [f32(1.0)] + ([f32(sigma_normal)] if sigma_normal is not None else [])
    dn_x = np.concatenate([mixture(rng, 0.0, 1.0, n // 2), np.array([0.0, 1.0], f32)])
    sets["powf"] = [("lobe", (lobe_x, rng.permutation(mixture(rng, 0.0, 1.0, n)))),
                    ("lobe edges", (np.repeat(np.concatenate([lobe_edges_x, lobe_x[:4096]]), edge_y.size), np.tile(edge_y, lobe_edges_x.size + 4096))),
                    ("medium", (rng.permutation(medium_x), medium_y)),
                    ("medium edges", tuple(grid(np.array([0.0, 1.0, 1.0 - 2.0 ** -24, 0.5], f32), np.array([0.0, -0.0, 1.0, 1.0e3, FLT_MAX], f32)).T)),
                    ("denoiser", (np.tile(dn_x, len(sigma)), np.repeat(np.array(sigma, f32), dn_x.size)))]
    sets["expf"] = [("[-100, 0]", (np.concatenate([-mixture(rng, 0.0, 100.0, n), np.array([-0.0, 0.0], f32)]),))]
    sets["logf"] = [("draw + 1e-4", (unit_draws(rng, n) + f32(1.0e-4),))]
    some = mixture(rng, 0.0, 1.0, n)
    sub = from_bits(rng.integers(1, 1 << 23, 1 << 16).astype(u32))
    roots = mixture(rng, 2.0 ** -60, 2.0 ** 60, 1 << 16)
    sets["sqrtf"] = [("[0, 1]", (some,)), ("subnormal arguments", (sub,)), ("squares of floats", (roots * roots,))]
    small = mixture(rng, 2.0 ** -126, 2.0 ** -100, 1 << 16)
    sets["div"] = [("[0, 1] / [0, 1]", (some, rng.permutation(some))), ("subnormal arguments", (sub, rng.permutation(np.concatenate([sub[:1 << 15], some[:1 << 15]])))),
                   ("subnormal quotients", (small, mixture(rng, 1.0, 2.0 ** 30, 1 << 16)))]
    ints = np.concatenate([np.arange(-64, 65).astype(f32), f32(2.0) ** np.arange(7, 127)])
    below = np.concatenate([from_bits(bits(ints[ints > 0]) - u32(1)), -from_bits(bits(ints[ints > 0]) - u32(1))])
    sets["wrap"] = [("|u| up to 3e38", (signed(rng, mixture(rng, 0.0, 3.0e38, n)),)), ("[-4, 4]", (signed(rng, mixture(rng, 0.0, 4.0, n // 4)),)),
                    ("integers, a step below, -2^-30", (np.concatenate([ints, -ints, below, np.array([-2.0 ** -30, -2.0 ** -149, 2.0 ** -149], f32)]),))]
    return sets


class Row:
    """one function on one band: the figures of the table and whatever broke a rule"""

    def __init__(self, function, band, cases):
        self.function, self.band, self.cases = function, band, cases
        self.max_ulps, self.worst, self.exact, self.glibc, self.failures, self.flushed = 0.0, None, float("nan"), float("nan"), [], 0

    def text(self):
        worst = "" if self.worst is None else " at " + ", ".join(f"{float(v)!r}" for v in self.worst)
        extra = f", {self.flushed} flushed to zero" if self.flushed else ""
        return (f"{self.function:<8} {self.band:<34} {self.cases:>8} cases  max {self.max_ulps:7.4f} ulp{worst}{extra}  "
                f"correctly rounded {self.exact:7.2%}  = glibc {self.glibc:7.2%}")


def judge(function, band, args, got, glibc_every=0, bar=BAR):
    """[Row for the normal range, Row for the subnormal range (if the band reaches it)] of `got` = function(*args) on one band"""
    args = [np.ascontiguousarray(a, f32) for a in args]
    got = np.ascontiguousarray(got, f32).reshape(-1)
    assert got.size == args[0].size
    with np.errstate(all="ignore"):
        want = REFERENCE[function](*args)
        rounded = want.astype(f32)
    show = lambda i: [a[i] for a in args] + [got[i]]
    nan = np.isnan(want)
    inf = np.isinf(want) | (np.abs(want) >= 2.0 ** 128 - 2.0 ** 103)  # (from there on a real value rounds to the float infinity)
    sub = ~nan & (np.abs(want) < TINY) & (want != 0)
    normal = ~nan & ~inf & ~sub
    row = Row(function, band, int(normal.sum() + nan.sum() + inf.sum()))
    bad = nan & ~np.isnan(got)
    if bad.any():
        row.failures.append(f"{function} {band}: {int(bad.sum())} results are not NaN where the true result is, first {show(int(np.argmax(bad)))}")
    bad = inf & ~(np.isinf(got) & (np.sign(got) == np.sign(want)))
    if bad.any():
        row.failures.append(f"{function} {band}: {int(bad.sum())} results are not the infinity the true result is, first {show(int(np.argmax(bad)))}")
    bad = normal & (want == 0) & ~((got == 0) & (np.signbit(got) == np.signbit(want)))
    if bad.any():
        row.failures.append(f"{function} {band}: {int(bad.sum())} results are not the zero, of that sign, the true result is, first {show(int(np.argmax(bad)))}")
    err = error_ulps(got, want)
    if normal.any():
        e = np.where(normal, err, -1.0)
        e = np.where(np.isnan(e), np.inf, e)  # a NaN where a number is due
        i = int(np.argmax(e))
        row.max_ulps, row.worst = float(e[i]), show(i)
        row.exact = float((bits(got)[normal] == bits(rounded)[normal]).mean())
        if function in EXACT:
            wrong = normal & ~same_bits_or_nan(got, EXACT[function](*args))
            if wrong.any():
                row.failures.append(f"{function} {band}: {int(wrong.sum())} results are not numpy float32's, first {show(int(np.argmax(wrong)))}")
            bar = 0.5 + 1.0e-6
        if row.max_ulps > bar:
            row.failures.append(f"{function} {band}: {row.max_ulps:.4f} ulp > {bar} at {show(i)} (true {want[i]!r}), {int((e > bar).sum())} cases beyond")
    rows = [row]
    if sub.any():
        srow = Row(function, band + " subnormal", int(sub.sum()))
        with np.errstate(all="ignore"):
            a = np.where(sub, np.abs(got.astype(f64) - want), -1.0)
        a = np.where(np.isnan(a), np.inf, a)
        i = int(np.argmax(a))
        srow.max_ulps, srow.worst = float(a[i] / 2.0 ** -149), show(i)
        srow.exact = float((bits(got)[sub] == bits(rounded)[sub]).mean())
        srow.flushed = int((sub & (got == 0) & (rounded != 0)).sum())
        if a[i] > TINY:
            srow.failures.append(f"{function} {band}: |error| {a[i]!r} > 2^-126 at {show(i)} (true {want[i]!r})")
        if function in EXACT:
            wrong = sub & ~same_bits_or_nan(got, EXACT[function](*args))
            if wrong.any():
                srow.failures.append(f"{function} {band}: {int(wrong.sum())} subnormal results are not numpy float32's, first {show(int(np.argmax(wrong)))}")
        rows.append(srow)
    if glibc_every:
        pick = np.arange(0, got.size, glibc_every)
        ref = glibc(function)(*[a[pick] for a in args])
        same = same_bits_or_nan(got[pick], ref)
        for r, mask in zip(rows, (normal | nan | inf, sub)):
            if mask[pick].any():
                r.glibc = float(same[mask[pick]].mean())
    return rows


def judge_function(function, evaluate, sets, glibc_every=0, bar=BAR):
    """every band of `function` through evaluate(*args) -> float32 results: the rows"""
    rows = []
    for band, args in sets[function]:
        rows += judge(function, band, args, evaluate(*args), glibc_every, bar)
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# composed primitives: numpy float32 re-derivations, operation by operation from the reference's formulas (cpu_render_utils.cpp:29-170,
# cpu_engine_kernel.cpp:585-594), on (n, 3) float32 arrays; numpy rounds every float32 operation separately, as -ffp-contract=off does
# ---------------------------------------------------------------------------------------------------------------------------------
def _c(v):
    v = np.asarray(v, f32)
    return v[..., 0], v[..., 1], v[..., 2]


def dot32(a, b):
    ax, ay, az = _c(a)
    bx, by, bz = _c(b)
    return (ax * bx + ay * by) + az * bz


def cross32(a, b):
    ax, ay, az = _c(a)
    bx, by, bz = _c(b)
    return np.stack([ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx], -1).astype(f32)


def local_coordinate32(n):  # :74-83 — the tie |x| == |y| goes to the else side: vX = (1, 0, 0)
    n = np.asarray(n, f32)
    b = np.abs(n[..., 0]) > np.abs(n[..., 1])
    vx = np.stack([(~b).astype(f32), b.astype(f32), np.zeros(b.shape, f32)], -1)
    with np.errstate(all="ignore"):
        vy = cross32(n, vx)
        vx = cross32(n, vy)
    return vx, vy


def reflect_vector32(i, n):  # :29-32
    with np.errstate(all="ignore"):
        return ((np.asarray(n, f32) * f32(-2.0)) * dot32(n, i)[..., None] + np.asarray(i, f32)).astype(f32)


def halfway_vector32(i, r):  # :33-36; normalise = multiply by 1 / sqrt(x x + y y + z z)
    with np.errstate(all="ignore"):
        v = (-np.asarray(i, f32)) + np.asarray(r, f32)
        x, y, z = _c(v)
        return (v * (f32(1.0) / np.sqrt((x * x + y * y) + z * z))[..., None]).astype(f32)


def fresnel32(n, i, n1, n2, fx0, fy0):  # :141-159
    n1, n2 = np.asarray(n1, f32), np.asarray(n2, f32)
    with np.errstate(all="ignore"):
        ratio = n1 / n2
        cosi = np.abs(dot32(i, n))
        sin2_t = ratio * ratio * (f32(1.0) - cosi * cosi)
        total = sin2_t >= f32(1.0)
        cost = np.sqrt(f32(1.0) - sin2_t)
        rp = ((n1 * cosi) - (n2 * cost)) / ((n1 * cosi) + (n2 * cost))
        rs = ((n2 * cosi) - (n1 * cost)) / ((n2 * cosi) + (n1 * cost))
        value = (rs * rs + rp * rp) / f32(2.0)
        fy = ratio * cosi - cost
    return np.stack([np.where(total, f32(1.0), value), np.where(total, np.asarray(fx0, f32), ratio), np.where(total, np.asarray(fy0, f32), fy)], -1).astype(f32)


def sin2_t32(n, i, n1, n2):
    with np.errstate(all="ignore"):
        ratio = np.asarray(n1, f32) / np.asarray(n2, f32)
        cosi = np.abs(dot32(i, n))
        return (ratio * ratio * (f32(1.0) - cosi * cosi)).astype(f32)


def total_reflection32(n, i, n1, n2):
    """where fresnel_specular_ratio returns early (sin2_t >= 1) and leaves the factors untouched"""
    return sin2_t32(n, i, n1, n2) >= f32(1.0)


def ndf32(n, h, roughness):  # cpu_engine_kernel.cpp:585-590
    r = np.asarray(roughness, f32)
    with np.errstate(all="ignore"):
        d = dot32(n, h)
        b = (d * d) * (r - f32(1.0)) + f32(1.0001)
        return ((r + f32(1.0e-5)) / (b * b)).astype(f32)


def attenuation32(c, roughness):  # :591-594
    c, r = np.asarray(c, f32), np.asarray(roughness, f32)
    with np.errstate(all="ignore"):
        return (c / ((c * (f32(1.0) - r)) + r)).astype(f32)


# the samplers in float64, the same formulas on the same float32 inputs (constants as the float32 values the code holds)
def _frame64(n):
    n64 = np.asarray(n, f32).astype(f64)
    b = np.abs(n64[..., 0]) > np.abs(n64[..., 1])
    x0 = np.stack([(~b).astype(f64), b.astype(f64), np.zeros(b.shape)], -1)
    vy = np.cross(n64, x0)
    return n64, np.cross(n64, vy), vy


def cosine_sample_hemisphere64(r1, r2, n):
    n64, vx, vy = _frame64(n)
    r1, r2 = _d(r1, r2)
    phi, s = r1 * f64(TWO_PI_F), np.sqrt(r2)
    return ((vx * s[:, None]) * np.cos(phi)[:, None] + (vy * s[:, None]) * np.sin(phi)[:, None]) + n64 * np.sqrt(1.0 - r2)[:, None]


def sample_sphere64(r1, r2, n, half=False):
    n64, vx, vy = _frame64(n)
    r1, r2 = _d(r1, r2)
    if half:
        r2 = r2 * 0.5
    phi = r1 * f64(TWO_PI_F)
    with np.errstate(invalid="ignore"):
        theta = np.arccos(1.0 - 2.0 * r2)
    return ((vx * np.sin(theta)[:, None]) * np.cos(phi)[:, None] + (vy * np.sin(theta)[:, None]) * np.sin(phi)[:, None]) + n64 * np.cos(theta)[:, None]


def sample_hemisphere64(r1, r2, n):
    return sample_sphere64(r1, r2, n, half=True)


def sample_disk64(r1, r2, n, radius):
    n64, vx, vy = _frame64(n)
    r1, r2, radius = _d(r1, r2, radius)
    phi = r1 * 2.0 * f64(PI_F)
    return ((vx * np.sin(phi)[:, None] + vy * np.cos(phi)[:, None]) * np.sqrt(r2)[:, None]) * radius[:, None]


def glossy_lobe64(u2, roughness):
    u2, r = _d(u2, roughness)
    with np.errstate(invalid="ignore"):
        theta = np.arccos(1.0 - 2.0 * ((1.0 - np.power(u2 + f64(f32(1.0e-5)), r)) * 0.5))
    return np.stack([np.sin(theta), np.cos(theta)], -1)


# ---------------------------------------------------------------------------------------------------------------------------------
# edges of the composed primitives
# ---------------------------------------------------------------------------------------------------------------------------------
EDGE_DRAWS = np.array([0.0, 2.0 ** -24, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -24], f32)


def edge_normals():
    import itertools
    s = f32(np.sqrt(0.5))
    rows = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),                     # the six axes
            (0.6, 0.6, 0.52915), (-0.6, 0.6, 0.52915), (0.5, -0.5, s), (s, s, 0.0), (-s, -s, -0.0),    # |x| == |y|: the tie
            (0.0, 0.6, 0.8), (-0.0, 0.6, 0.8), (0.6, 0.0, 0.8), (0.6, -0.0, 0.8), (0.6, 0.8, 0.0), (0.6, 0.8, -0.0), (-0.0, -0.0, 1.0)]
    rows += list(itertools.permutations((1.0, 1.0e-8, 0.0)))
    unit = np.array(rows, f32)
    scaled = np.concatenate([unit[6:12] * f32(0.5), unit[6:12] * f32(2.0), unit[:2] * f32(0.5), unit[2:4] * f32(2.0)])  # the frame is not orthonormal
    return np.concatenate([unit, scaled]).astype(f32)


def random_units(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(f32)


def grid(*columns):
    """the cross product of the columns (each (k,) or (k, w)) as one (N, total width) float32 array"""
    columns = [np.asarray(c, f32).reshape(len(c), -1) for c in columns]
    idx = np.stack(np.meshgrid(*[np.arange(len(c)) for c in columns], indexing="ij"), -1).reshape(-1, len(columns))
    return np.concatenate([c[idx[:, k]] for k, c in enumerate(columns)], 1)


def sampler_cases(rng, n_random, disk=False):
    """{class: (n, 5 | 6) rows of r1, r2, normal[, radius]}"""
    normals = edge_normals()
    radius_edges = np.array([0.0, 1.0e-30, 0.5], f32)
    cols = [EDGE_DRAWS, EDGE_DRAWS, normals] + ([radius_edges] if disk else [])
    edges = grid(*cols)
    rnd = [unit_draws(rng, n_random - 3)[:, None], rng.permutation(unit_draws(rng, n_random - 3))[:, None], random_units(rng, n_random)]
    if disk:
        rnd.append(mixture(rng, 0.0, 2.0, n_random)[:, None])
    return {"random": np.concatenate(rnd, 1).astype(f32), "edges": edges}


def lobe_cases(rng, n_random):
    rough_edges = np.array([0.0, -0.0, 2.0 ** -100, 2.0 ** -24, 0.5, 1.0], f32)
    return {"random": np.stack([unit_draws(rng, n_random - 3), rng.permutation(mixture(rng, 0.0, 1.0, n_random))], 1),
            "edges": grid(np.concatenate([EDGE_DRAWS, unit_draws(rng, 61)]), rough_edges)}


def fresnel_cases(rng, n_random):
    """rows of n[3], i[3], n1, n2, fx0, fy0: random pairs, and the edges: cosi 1 and 0, n1 == n2, ratios 1 / 2.5 and 2.5, the float
    neighbours of the critical cosine at ratio 2.5, and sin2_t (sin2_t32 below) exactly at the last float below 1, at 1 and at the first
    float above: n1 == n2 with cosi = 2^-12 (1 - 2^-24 is exact), cosi = 0, and n1 = 1 + 2^-23 over n2 = 1 with cosi = 2^-12 (the
    ratio's square rounds to 1 + 2^-22, its product with 1 - 2^-24 lies just below the tie and rounds to 1 + 2^-23)"""
    n = random_units(rng, n_random)
    i = random_units(rng, n_random)
    ior = np.array([1.0, 1.33, 1.5, 2.5], f32)
    rnd = np.concatenate([n, i, ior[rng.integers(0, 4, n_random)][:, None], ior[rng.integers(0, 4, n_random)][:, None],
                          np.full((n_random, 1), 7.0, f32), np.full((n_random, 1), -9.0, f32)], 1).astype(f32)
    z = np.array([[0, 0, 1]], f32)
    # incoming directions in the x-z plane against n = z: cosi = |i.z| exactly
    cos_edge = np.concatenate([np.array([1.0, 0.0, -0.0, -1.0, 2.0 ** -24], f32), neighbours(f32(np.sqrt(1.0 - 1.0 / 6.25)), 4096)])
    inc = np.stack([np.sqrt(np.maximum(0.0, 1.0 - cos_edge.astype(f64) ** 2)).astype(f32), np.zeros(cos_edge.size, f32), -cos_edge], 1)
    pairs = np.array([[1.0, 1.0], [1.5, 1.5], [1.0, 2.5], [2.5, 1.0]], f32)
    edges = grid(z, inc, pairs, np.array([[7.0, -9.0]], f32))
    c12 = f32(2.0 ** -12)
    at = np.array([[np.sqrt(1.0 - 2.0 ** -24), 0.0, -c12], [np.sqrt(1.0 - 2.0 ** -24), 0.0, c12]], f32)
    boundary = np.concatenate([grid(z, at, np.array([[1.0, 1.0], [1.5, 1.5], [1.0 + 2.0 ** -23, 1.0]], f32), np.array([[7.0, -9.0]], f32)),
                               grid(z, np.array([[1.0, 0.0, 0.0], [1.0, 0.0, -0.0]], f32), np.array([[1.0, 1.0], [2.5, 2.5]], f32), np.array([[7.0, -9.0]], f32))])
    return {"random": rnd, "edges": np.concatenate([edges, boundary]).astype(f32)}


SIN2_T_BOUNDARY = (f32(1.0) - f32(2.0 ** -24), f32(1.0), f32(1.0) + f32(2.0 ** -23))  # the last float below 1, 1, the first above


def fresnel_boundary_counts(cases):
    """how many cases put sin2_t exactly on each value of SIN2_T_BOUNDARY"""
    t = sin2_t32(cases[:, 0:3], cases[:, 3:6], cases[:, 6], cases[:, 7])
    return [int((bits(t) == bits(v)).sum()) for v in SIN2_T_BOUNDARY]


def brdf_cases(rng, n_random):
    cosines = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -24, 0.5], f32)
    rough = np.array([0.0, 1.0, 0.5, 2.0 ** -24], f32)
    att = {"random": np.stack([signed(rng, mixture(rng, 0.0, 1.0, n_random)), rng.permutation(mixture(rng, 0.0, 1.0, n_random))], 1),
           "edges": grid(cosines, rough)}  # holds attenuation(0, 0) = 0 / 0
    z = np.array([[0, 0, 1]], f32)
    h = np.stack([np.sqrt(np.maximum(0.0, 1.0 - cosines.astype(f64) ** 2)).astype(f32), np.zeros(cosines.size, f32), cosines], 1)
    nd = {"random": np.concatenate([random_units(rng, n_random), random_units(rng, n_random), rng.permutation(mixture(rng, 0.0, 1.0, n_random))[:, None]], 1).astype(f32),
          "edges": np.concatenate([grid(z, h, rough), grid(edge_normals(), edge_normals()[:6], rough)])}
    return att, nd


def vector_pair_cases(rng, n_random):
    e = edge_normals()
    return {"random": np.concatenate([random_units(rng, n_random), random_units(rng, n_random)], 1), "edges": grid(e, e)}


# ---------------------------------------------------------------------------------------------------------------------------------
# sample_direction: cases (rows of 22 floats, include/hiprz.h) and which path each takes
# ---------------------------------------------------------------------------------------------------------------------------------
def rng_make(sx, sy, r):  # cpu_render_utils.cpp:8-27
    return (np.asarray(sx, f32) + np.asarray(sy, f32)).astype(f32), (np.asarray(r, f32) * f32(245.310913)).astype(f32)


def rng_draw(a, b):
    af = (a + f32(0.2311362)) * (b + f32(13.054377))
    bf = (a + f32(251.78431)) + (b - f32(73.054312))
    a = (af - np.trunc(af)).astype(f32)
    b = (bf - np.trunc(bf)).astype(f32)
    return a, b, np.abs(b)


PATHS = ("scattering", "refraction", "specular reflection", "diffuse", "glossy")
ROUGHNESS_EDGES = np.array([0.0, -0.0, 2.0 ** -100, 1.0], f32)


def direction_path(cases):
    """0..4 per case (PATHS), from the case's own generator: the first draw decides refraction against reflection, or diffuse against glossy"""
    a, b = rng_make(cases[:, 0], cases[:, 1], cases[:, 2])
    _, _, u = rng_draw(a, b)
    alpha, scattering, fresnel, reflectance = cases[:, 3], cases[:, 4], cases[:, 5], cases[:, 6]
    return np.where(alpha > 0, np.where(scattering > 0, 0, np.where(fresnel < u, 1, 2)), np.where(u > reflectance, 3, 4))


def _as_float(words):
    return np.asarray(words, u32).view(f32)


def direction_cases_random(rng, n):
    sx, sy, r = rng.random(n).astype(f32), rng.random(n).astype(f32), (rng.random(n) * 20 - 10).astype(f32)
    alpha = np.where(rng.random(n) < 0.5, 0.0, rng.random(n) * 0.999 + 0.001).astype(f32)
    scattering = np.where(rng.random(n) < 0.75, 0.0, rng.random(n) * 4 + 0.01).astype(f32)
    fresnel = rng.random(n).astype(f32)
    reflectance = np.select([rng.random(n) < 0.1, rng.random(n) < 0.1], [0.0, 1.0], rng.random(n)).astype(f32)
    metalness = rng.random(n).astype(f32)
    kind = rng.integers(0, 8, n)
    roughness = np.where(kind < 4, ROUGHNESS_EDGES[kind % 4], mixture(rng, 0.0, 1.0, n)[rng.permutation(n)]).astype(f32)
    normal = random_units(rng, n)
    bent = normal.astype(f64) + rng.normal(size=(n, 3)) * rng.choice([0.0, 0.05, 0.6], n)[:, None]
    mapped = (bent / np.linalg.norm(bent, axis=1)[:, None]).astype(f32)
    # incoming directions: towards the surface, a third of them grazing (where the reflection can end below the surface: the flip)
    t = random_units(rng, n).astype(f64)
    t -= normal * np.sum(t * normal, 1)[:, None]
    t /= np.linalg.norm(t, axis=1)[:, None]
    down = np.where(rng.random(n) < 0.33, rng.random(n) * 0.05, rng.random(n))[:, None]
    d = t * np.sqrt(1 - down ** 2) - normal * down
    ray_d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(f32)
    refr = (rng.random((n, 2)) * 2 - 1).astype(f32)
    mats = np.stack([_as_float(rng.integers(0, 16, n)), _as_float(rng.integers(16, 32, n))], 1)
    return np.concatenate([np.stack([sx, sy, r, alpha, scattering, fresnel, reflectance, metalness, roughness], 1), normal, mapped, refr, ray_d, mats], 1).astype(f32)


def direction_cases_grid(rng, states=64):
    """the surface grid — edge normals x roughness edges x (opaque: reflectance 0, 0.5, 1 | transparent: scattering 0 / 0.5, fresnel 0, 0.5, 1)
    — crossed with `states` generator states and incoming directions each"""
    normals = edge_normals()
    rough = np.concatenate([ROUGHNESS_EDGES, np.array([0.3], f32)])
    opaque = grid([0.0], [0.0], [0.5], [0.0, 0.5, 1.0], [0.25], rough)
    clear = grid([1.0], [0.0, 0.5], [0.0, 0.5, 1.0], [0.5], [0.25], [0.3])
    surf = grid(np.concatenate([opaque, clear]), normals)
    surf = np.repeat(surf, states, 0)
    n = len(surf)
    normal = surf[:, 6:9]
    ray_d = random_units(rng, n)
    ray_d = np.where((np.sum(ray_d * normal, 1) > 0)[:, None], -ray_d, ray_d).astype(f32)
    gen = np.stack([rng.random(n), rng.random(n), rng.random(n) * 20 - 10], 1).astype(f32)
    refr = np.tile(np.array([[0.75, -0.3]], f32), (n, 1))
    mats = np.tile(_as_float([3, 7])[None, :], (n, 1))
    return np.concatenate([gen, surf[:, :6], normal, normal, refr, ray_d, mats], 1).astype(f32)


def direction_sides(out):
    """the two spellings' outputs as uint32 words (n, 10) each, NaNs made one pattern, and the path word"""
    words = np.ascontiguousarray(out, f32).view(u32).copy()
    words[np.isnan(out)] = 0x7FC00000
    return words[:, :10], words[:, 10:20], words[:, 20]


# ---------------------------------------------------------------------------------------------------------------------------------
# the samplers and the lobe against float64: errors per output component, and the bar from the oracle and its one-ulp stand-ins
# ---------------------------------------------------------------------------------------------------------------------------------
SAMPLERS = {  # primitive: (the oracle's export, the float64 formula on the case's columns, output width)
    "cosine_sample_hemisphere": ("rzo_cosine_sample_hemisphere", lambda c: cosine_sample_hemisphere64(c[:, 0], c[:, 1], c[:, 2:5]), 3),
    "sample_sphere": ("rzo_sample_sphere", lambda c: sample_sphere64(c[:, 0], c[:, 1], c[:, 2:5]), 3),
    "sample_hemisphere": ("rzo_sample_hemisphere", lambda c: sample_hemisphere64(c[:, 0], c[:, 1], c[:, 2:5]), 3),
    "sample_disk": ("rzo_sample_disk", lambda c: sample_disk64(c[:, 0], c[:, 1], c[:, 2:5], c[:, 5]), 3),
    "glossy_lobe": ("rzo_glossy_lobe", lambda c: glossy_lobe64(c[:, 0], c[:, 1]), 2),
}
STAND_INS = ("lo", "hi", "mix")  # oracle/Makefile: every inexact libm result one ulp down, up, or either


def polar_draw64(name, cases):
    """the r2 that reaches acosf(1 - 2 r2) in the primitive, in float64 (None: the primitive takes no arc cosine)"""
    c = np.asarray(cases, f32).astype(f64)
    if name == "sample_sphere":
        return c[:, 1]
    if name == "sample_hemisphere":
        return c[:, 1] * 0.5
    if name == "glossy_lobe":
        with np.errstate(all="ignore"):
            return (1.0 - np.power(c[:, 0] + f64(f32(1.0e-5)), c[:, 1])) * 0.5
    return None


def sampler_cases_of(name, rng, n_random):
    """{class: cases}.  The random draws of a primitive that takes acosf(1 - 2 r2) are two classes: the float32 rounding of 1 - 2 r2 (up
    to 2^-25) reaches the angle multiplied by 1 / sin(theta) = 1 / (2 sqrt(r2 (1 - r2))), on the device and in the oracle alike.  Where
    that factor is at most 4 — r2 (1 - r2) >= 1 / 64 — the class's error against float64 stays at a few float steps of 1, and the bar made
    of it notices a library call that is wrong at that size; the rest ("random, steep arc cosine": r2 towards 0 or 1, errors up to about
    2e-4 whatever the library does) would hide it and is held on its own."""
    sets = lobe_cases(rng, n_random) if name == "glossy_lobe" else sampler_cases(rng, n_random, disk=name == "sample_disk")
    r2 = polar_draw64(name, sets["random"])
    if r2 is not None:
        with np.errstate(invalid="ignore"):
            gentle = r2 * (1.0 - r2) >= 1.0 / 64.0  # (NaN: not gentle)
        rnd = sets.pop("random")
        sets = {"random": rnd[gentle], "random, steep arc cosine": rnd[~gentle], **sets}
    return sets


def oracle_sampler(lib, name, cases):
    """the primitive through the scalar export of an oracle library (tests/oracle.py: load() or variant()), case by case"""
    cases = np.ascontiguousarray(cases, f32)
    fn, width = getattr(lib, SAMPLERS[name][0]), SAMPLERS[name][2]
    out = np.zeros((len(cases), width), f32)
    base, obase, rows = cases.ctypes.data, out.ctypes.data, cases.tolist()
    stride = cases.strides[0]
    for i, row in enumerate(rows):
        if name == "glossy_lobe":
            fn(row[0], row[1], obase + 8 * i)
        elif name == "sample_disk":
            fn(row[0], row[1], base + stride * i + 8, row[5], obase + 12 * i)
        else:
            fn(row[0], row[1], base + stride * i + 8, obase + 12 * i)
    return out


def sampler_errors(name, cases, got):
    """(largest absolute error per output component over the cases where both sides hold a number, which cases are NaN in `got`)"""
    with np.errstate(all="ignore"):
        want = SAMPLERS[name][1](np.ascontiguousarray(cases, f32))
        err = np.abs(np.asarray(got, f32).astype(f64) - want)
    return np.nanmax(np.where(np.isnan(err), -1.0, err), axis=0), np.isnan(got).any(1)


def sampler_bar(oracle_module, name, cases):
    """twice the largest error among the plain oracle and its three one-ulp stand-ins on the same cases, per component; the plain oracle's
    own errors; and the cases where any of the four returns NaN"""
    plain, nan = sampler_errors(name, cases, oracle_sampler(oracle_module.load(), name, cases))
    worst = plain.copy()
    for v in STAND_INS:
        e, n = sampler_errors(name, cases, oracle_sampler(oracle_module.variant(v), name, cases))
        worst, nan = np.maximum(worst, e), nan | n
    return 2.0 * worst, plain, nan
