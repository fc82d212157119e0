"""Bounce baking (include/hiprz_gather.h) restated in numpy float32, one rounding per operation like the device build (-ffp-contract=off):
the chart id of a hit, the lookup of the texel under it, what a ray contributes, the fixed-order mean with its two counts, and compose.
The rays themselves are hiprz_bake.h's (tests/bake_reference.py).  For tests/test_gather_reference.py (CPU), which holds it to the same
rules in float64 and shows that its mutants differ from it, and tests/test_gather_gpu.py, which holds the device's samples to ids() over
the query's own hits and its texels to texels() over the emitted samples, bit for bit.

MUTANTS, each a wrong reading of the header that the tests must tell from the right one:
  swap    bx and by exchanged in the lookup (the weights of vertices 2 and 3)
  rint    the texel by rounding to nearest instead of floorf
  back    a back-face hit keeps its chart id (and so contributes)
  order   the K contributions added one after the other instead of per lane and by the butterfly"""
import numpy as np

from bake_reference import butterfly, valid
from rayzath_amd.gather import BACK, INVALID, INVALID_RAY, MAX_CHARTS, MISS, NONE, UNMAPPED, record_dtype, sample_dtype, texel_dtype
from rayzath_amd.query import HIT_EXTERNAL, HIT_FOUND, HIT_INVALID

F = np.float32
MUTANTS = ("swap", "rint", "back", "order")


def ids(flags, instance, source_index, base, n_charts, mutant=None):
    """hiprz_gather_sample::id from what hiprz_query_closest says of the same ray (hiprz_hit::flags, ::instance, ::source_index) and
    the chart map's bases: "THE CHART MAP" and the four codes"""
    flags, instance, source_index = np.asarray(flags), np.asarray(instance), np.asarray(source_index)
    base = np.asarray(base, np.uint32)
    found = (flags & HIT_FOUND) != 0
    b = base[np.where(found, instance, 0)].astype(np.uint64) if len(base) else np.full(flags.shape, NONE, np.uint64)
    chart = b + source_index.astype(np.uint64)
    out = np.where((b == NONE) | (chart >= n_charts), np.uint64(UNMAPPED), chart)
    if mutant != "back":
        out = np.where((flags & HIT_EXTERNAL) != 0, out, np.uint64(BACK))
    out = np.where(found, out, np.uint64(MISS))
    return np.where((flags & HIT_INVALID) != 0, np.uint64(INVALID_RAY), out).astype(np.uint32)


def uv(samples, charts, dtype=F, mutant=None):
    """(u, v, mapped) of every sample: "THE LOOKUP" up to the texel, in `dtype`; mapped: the sample has a chart id"""
    s = np.asarray(samples)
    mapped = s["id"] < MAX_CHARTS
    c = charts[np.where(mapped, s["id"], 0)] if len(charts) else np.zeros(s.shape, charts.dtype)
    bx, by = s["bx"].astype(dtype), s["by"].astype(dtype)
    if mutant == "swap":
        bx, by = by, bx
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        b1 = (one - bx) - by
        u = (c["u1"].astype(dtype) * b1 + c["u2"].astype(dtype) * bx) + c["u3"].astype(dtype) * by
        v = (c["v1"].astype(dtype) * b1 + c["v2"].astype(dtype) * bx) + c["v3"].astype(dtype) * by
    return u, v, mapped


def texel_of(u, v, W, H, mutant=None):
    """(x, y, finite): x = clamp(int(floorf(u * float(W))), 0, W - 1), y likewise; finite: neither u nor v is NaN or an infinity"""
    snap = np.rint if mutant == "rint" else np.floor
    with np.errstate(all="ignore"):
        finite = np.isfinite(u) & np.isfinite(v)
        fx = snap(np.where(finite, u, 0) * u.dtype.type(W))
        fy = snap(np.where(finite, v, 0) * v.dtype.type(H))
    return np.clip(fx, 0, W - 1).astype(np.int64), np.clip(fy, 0, H - 1).astype(np.int64), finite


def contributions(samples, charts, source, W, H, sky, mutant=None):
    """(values (..., 3) float32, read, missed) of every sample: "A RAY'S CONTRIBUTION" over the W x H source (16-byte records)"""
    s = np.asarray(samples)
    src = np.ascontiguousarray(source).reshape(-1).view(record_dtype)
    u, v, mapped = uv(s, charts, F, mutant)
    x, y, finite = texel_of(u, v, W, H, mutant)
    texel = src[y * W + x]
    read = mapped & finite & (texel["word"] != INVALID)
    missed = (s["id"] == MISS) | (s["id"] == INVALID_RAY)
    values = np.where(read[..., None], texel["rgb"], F(0.0))
    values = np.where(missed[..., None], np.asarray(sky, F), values).astype(F)
    return values, read, missed


def texels(points, samples, charts, source, W, H, sky, mutant=None):
    """the texels of 1-d `points` from their samples ((n, K) sample_dtype, as the device emits them): "THE RESULT" """
    ok = valid(points).reshape(-1)
    s = np.asarray(samples).reshape(len(ok), -1)
    K = s.shape[1]
    values, read, missed = contributions(s, charts, source, W, H, sky, mutant)
    out = np.zeros(len(ok), texel_dtype)
    if mutant == "order":
        total = np.zeros((len(ok), 3), F)
        for k in range(K):
            total = total + values[:, k]
    else:
        total = butterfly(values)
    out["mean"] = total * (F(1.0) / F(K))
    out["counts"] = read.sum(-1, dtype=np.uint32) | (missed.sum(-1, dtype=np.uint32) << np.uint32(16))
    out["mean"][~ok] = 0.0
    out["counts"][~ok] = INVALID
    return out


def compose(direct, indirect, albedo, emission):
    """out.c = (albedo.c * (direct.c + indirect.c)) + emission.c, the word of `direct`; indirect and emission may be None: +0"""
    d = np.ascontiguousarray(direct).view(record_dtype)
    zero = np.zeros(d.shape + (3,), F)
    g = zero if indirect is None else np.ascontiguousarray(indirect).view(record_dtype)["rgb"]
    e = zero if emission is None else np.ascontiguousarray(emission).view(record_dtype)["rgb"]
    a = np.ascontiguousarray(albedo).view(record_dtype)["rgb"]
    out = np.zeros(d.shape, record_dtype)
    with np.errstate(all="ignore"):
        out["rgb"] = (a * (d["rgb"] + g)) + e
    out["word"] = d["word"]
    return out


def make_samples(ids_, bx, by, t):
    out = np.zeros(np.shape(ids_), sample_dtype)
    out["id"], out["bx"], out["by"], out["t"] = ids_, bx, by, t
    return out
