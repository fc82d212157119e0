"""Light baking (include/hiprz_light.h) restated in numpy, one rounding per operation like the device build (-ffp-contract=off): the frame,
the spot and the direct sample with the header's parenthesisation, the skip rule, the hash that picks a point's set, the invalid-point
rule, the per-lane sum over lights and rounds with its butterfly, and the disk table in float64.  Every function takes the arithmetic's
dtype: float32 is the device's, float64 the yardstick the float32 evaluation is measured against.  For tests/test_light_reference.py (CPU)
and tests/test_light_gpu.py, which holds the device's rays and weights to rays() in every byte and its texels to texels() over the query's
own verdicts.

MUTANTS (the `mutant` argument) are wrong on purpose, to prove the comparisons have teeth: "angle" tests the beam against the angle instead
of its cosine, "far" gives a spot ray the point's far_, "order" sums the lights in the other order, "skipped" counts skipped rays as
shadowed."""
import numpy as np

import bake_reference as BR
from rayzath_amd.bake import point_dtype
from rayzath_amd.light import INVALID, texel_dtype
from rayzath_amd.query import ray_dtype

F = np.float32
PI_F = F(3.14159265358979323846)
hash32, set_of, valid = BR.hash32, BR.set_of, BR.valid
MUTANTS = ("angle", "far", "order", "skipped")


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _magnitude(a):
    return np.sqrt(_dot(a, a))


def _normalized(a):
    one = a.dtype.type(1.0)
    return a * (one / _magnitude(a))[..., None]


def _similarity(a, b):
    one = a.dtype.type(1.0)
    return _dot(a, b) * ((one / _magnitude(a)) * (one / _magnitude(b)))


def colour_emission(spots, directs, dtype=F):
    """(L, 3): colour.c * emission of the lights in the bake's order, colour.c = u8 / 255"""
    out = [(l["color"][:3].astype(dtype) / dtype(255.0)) * dtype(l["emission"]) for l in list(spots) + list(directs)]
    return np.array(out, dtype).reshape(-1, 3)


def spot_sample(position, n, light, xy, dtype=F, mutant=None):
    """(w3 (n, K, 3), far (n, K), w (n, K)) before the skip rule: include/hiprz_light.h "A SPOT LIGHT"; position, n: (n, 3), xy: (n, K, 2)"""
    T = dtype
    lpos, ldir, size = light["position"].astype(T), light["direction"].astype(T), T(light["size"])
    cos_angle = T(light["angle"] if mutant == "angle" else light["cos_angle"])
    x, y = xy[..., 0:1].astype(T), xy[..., 1:2].astype(T)
    a = _normalized(lpos - position)
    t, bt = BR.frame(a)
    q = lpos + ((t[:, None] * x + bt[:, None] * y) * size)
    vPL = q - position[:, None]
    dPL = _magnitude(vPL)
    w3 = _normalized(vPL)
    c = _dot(n[:, None], w3)
    A = (size * size) * T(PI_F)
    d1 = dPL + T(1.0)
    inside = cos_angle < _similarity(-vPL, ldir)
    w = np.where((c > 0) & inside, c * (A / (d1 * d1)), T(0.0))
    return w3, dPL, w


def direct_sample(position, n, light, xy, far, dtype=F, mutant=None):
    """the same for include/hiprz_light.h "A DIRECT LIGHT"; far: (n,), the points'"""
    T = dtype
    ldir, ca = light["direction"].astype(T), T(light["cos_angular_size"])
    x, y = xy[..., 0].astype(T), xy[..., 1].astype(T)
    a = -ldir
    t, bt = BR.frame(a)
    r2 = x * x + y * y
    z = T(1.0) - r2 * (T(1.0) - ca)
    h = np.sqrt(np.fmax(T(0.0), T(1.0) - z * z))
    g = np.where(r2 > 0, h / np.sqrt(r2), T(0.0))
    xg, yg = (x * g)[..., None], (y * g)[..., None]
    d = (t * xg + bt * yg) + a * z[..., None]
    w3 = _normalized(d)
    c = _dot(n[:, None], w3)
    w = np.where(c > 0, c * ((T(2.0) * T(PI_F)) * (T(1.0) - ca)), T(0.0))
    return w3, np.broadcast_to(far[:, None].astype(T), w.shape), w


def samples(points, spots, directs, table, seed, dtype=F, mutant=None):
    """(w3 (n, L, K, 3), far (n, L, K), w (n, L, K), kept (n, L, K)) of 1-d `points` under `table` ((S, K, 2) float32) in arithmetic `dtype`,
    after the skip rule: a sample not kept has w3 = 0, far = the point's and w = +0"""
    p = np.ascontiguousarray(points).reshape(-1).view(point_dtype)
    table = np.asarray(table, F)
    S, K = table.shape[:2]
    ok = valid(p)
    T = dtype
    with np.errstate(all="ignore"):
        position, far = p["position"].astype(T), p["far"]
        n = _normalized(p["normal"].astype(T))
        xy = table[set_of(np.arange(len(p)), seed, S)]
        parts = [spot_sample(position, n, l, xy, T, mutant) + (l["emission"],) for l in spots]
        parts += [direct_sample(position, n, l, xy, far, T, mutant) + (l["emission"],) for l in directs]
        L = len(parts)
        w3, fars, w, kept = np.zeros((len(p), L, K, 3), T), np.zeros((len(p), L, K), T), np.zeros((len(p), L, K), T), np.zeros((len(p), L, K), bool)
        for l, (a, b, c, emission) in enumerate(parts):
            if mutant == "far" and l < len(spots):
                b = np.broadcast_to(far[:, None].astype(T), c.shape)
            keep = ok[:, None] & (c > 0) & (emission > 0) & np.isfinite(a).all(-1) & np.isfinite(b) & np.isfinite(c)
            w3[:, l], fars[:, l], w[:, l], kept[:, l] = np.where(keep[..., None], a, T(0.0)), np.where(keep, b, far[:, None].astype(T)), np.where(keep, c, T(0.0)), keep
    return w3, fars, w, kept


TO_END = 0xFFFFFFFF


def select(spots, directs, lights):
    """the (spots, directs) that `lights` selects — None: all, or (spot_first, spot_count, direct_first, direct_count) with a count of None
    or 0xFFFFFFFF for "to the end" — by include/hiprz_light.h "THE LIGHTS", restated; ValueError for a range outside the lights"""
    if lights is None:
        return spots, directs
    picked = []
    for have, first, count in ((spots, lights[0], lights[1]), (directs, lights[2], lights[3])):
        first = int(first)
        if first > len(have):
            raise ValueError("the range starts behind the last light")
        count = len(have) - first if count is None or int(count) == TO_END else int(count)
        if first + count > len(have):
            raise ValueError("the range ends behind the last light")
        picked.append(have[first:first + count])
    return tuple(picked)


def rays(points, spots, directs, table, seed, lights=None, mutant=None):
    """(rays (n, L, K) ray_dtype, weights (n, L, K) float32) hiprz_light_rays writes for 1-d `points`"""
    spots, directs = select(spots, directs, lights)
    p = np.ascontiguousarray(points).reshape(-1).view(point_dtype)
    w3, far, w, _ = samples(p, spots, directs, table, seed, F, mutant)
    out = np.zeros(w.shape, ray_dtype)
    out["origin"], out["near"] = p["position"][:, None, None, :], p["near"][:, None, None]
    out["direction"], out["far"] = w3, far
    return out, w


def texels(points, weights, words, ce, mutant=None):
    """the texels of `points` from the weights of their samples ((n, L, K) float32, as rays() or the device gives them), the occlusion word
    of every ray ((n, L, K), hiprz_query_occluded's) and colour * emission per light (colour_emission()): per lane the lights in order and
    the rounds in order, the butterfly, then * (1 / K); shadowed counts the occluded among the walked (w > 0); INVALID / +0 for an invalid
    point"""
    ok = valid(points).reshape(-1)
    weights = np.asarray(weights, F)
    n, L, K = weights.shape
    words = np.asarray(words).reshape(weights.shape) != 0
    walked = weights > 0
    lanes = min(K, 64)
    v = np.zeros((n, lanes, 3), F)
    order = range(L - 1, -1, -1) if mutant == "order" else range(L)
    for l in order:
        term = np.where((walked[:, l] & ~words[:, l])[..., None], ce[l].astype(F)[None, None, :] * weights[:, l][..., None], F(0.0)).astype(F)
        for r in range(K // lanes):
            v = v + term[:, lanes * r:lanes * (r + 1)]
    off = 1
    while off < lanes:
        v = v + v[:, np.arange(lanes) ^ off]
        off *= 2
    out = np.zeros(n, texel_dtype)
    count = (words & walked).sum((1, 2), dtype=np.uint32)
    if mutant == "skipped":
        count = count + (~walked).sum((1, 2), dtype=np.uint32)
    out["shadowed"] = np.where(ok, count, np.uint32(INVALID))
    out["light"] = v[:, 0] * (F(1.0) / F(K))
    out["light"][~ok] = 0.0
    return out


def disk_table(K, S):
    """hiprz_light_disk_samples in numpy float64, rounded to float32: (S, K, 2)"""
    k, s = np.arange(K, dtype=np.float64)[None, :], np.arange(S, dtype=np.float64)[:, None]
    r = np.sqrt((k + 0.5) / K)
    turn = k * 0.6180339887498949
    phi = 2.0 * np.pi * ((turn - np.floor(turn)) + s / S)
    return np.stack([r * np.cos(phi), r * np.sin(phi)], -1).astype(F)
