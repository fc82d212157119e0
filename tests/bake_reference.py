"""Occlusion baking (include/hiprz_bake.h) restated in numpy float32, one rounding per operation like the device build (-ffp-contract=off):
normalized(), the frame, the rotation with the header's parenthesisation, the hash that picks a point's set, the invalid-point rule, the
butterfly sum of `bent`, and the cosine table in float64.  For tests/test_bake_reference.py (CPU) and tests/test_bake_gpu.py, which holds
the device's rays to rays() in every byte and its texels to texels() over the query's own verdicts."""
import numpy as np

from rayzath_amd.bake import INVALID, point_dtype, texel_dtype
from rayzath_amd.query import ray_dtype

F = np.float32
ONE = F(1.0)


def hash32(x):
    """hiprz_bake_hash on uint32 (computed in uint64 and masked: no overflow warnings)"""
    U = np.uint64
    x = np.atleast_1d(np.asarray(x, U)) & U(0xFFFFFFFF)
    x = x ^ (x >> U(16))
    x = (x * U(0x7feb352d)) & U(0xFFFFFFFF)
    x = x ^ (x >> U(15))
    x = (x * U(0x846ca68b)) & U(0xFFFFFFFF)
    x = x ^ (x >> U(16))
    return x.astype(np.uint32)


def set_of(i, seed, S):
    """the set of point i (array or scalar): hash(i ^ seed) % S"""
    return hash32(np.asarray(i, np.uint64) ^ np.uint64(seed)) % np.uint32(S)


def _length(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def normalized(v):
    """the device's normalized(): v * (1 / sqrt((x*x + y*y) + z*z)) on (..., 3) float32"""
    v = np.asarray(v, F)
    return v * (ONE / _length(v))[..., None]


def valid(points):
    """include/hiprz_query.h "AN INVALID RAY" under NORMALIZE, of the point as the ray along its normal"""
    p = np.ascontiguousarray(points).view(point_dtype)
    with np.errstate(all="ignore"):
        length = _length(p["normal"])
        rcp = ONE / length
        ok = np.isfinite(p["position"]).all(-1) & np.isfinite(p["normal"]).all(-1) & np.isfinite(p["near"]) & np.isfinite(p["far"])
        ok &= ~(p["near"] < 0) & (p["far"] > p["near"])
        ok &= (length > 0) & np.isfinite(length) & np.isfinite(rcp)
    return ok


def frame(n):
    """(t, bt) of unit normals n (..., 3) float32: include/hiprz_bake.h "THE FRAME" """
    n = np.asarray(n)
    one = n.dtype.type(1.0)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    s = np.copysign(one, nz)
    a = -one / (s + nz)
    b = (nx * ny) * a
    t = np.stack([one + ((s * nx) * nx) * a, s * b, (-s) * nx], -1)
    bt = np.stack([b, s + (ny * ny) * a, -ny], -1)
    return t, bt


def rotate(n, t, bt, l):
    """d.c = (t.c * l.x + bt.c * l.y) + n.c * l.z; n, t, bt: (..., 3), l: (..., K, 3) -> (..., K, 3)"""
    n, t, bt = n[..., None, :], t[..., None, :], bt[..., None, :]
    return (t * l[..., 0:1] + bt * l[..., 1:2]) + n * l[..., 2:3]


def rays(points, table, seed):
    """the rays hiprz_bake_rays writes for 1-d `points` under `table` ((S, K, 4) float32): (n, K) ray_dtype"""
    p = np.ascontiguousarray(points).reshape(-1).view(point_dtype)
    table = np.asarray(table, F)
    S, K = table.shape[:2]
    ok = valid(p)
    with np.errstate(all="ignore"):
        n = normalized(p["normal"])
        t, bt = frame(n)
        sets = set_of(np.arange(len(p)), seed, S)
        d = rotate(n, t, bt, table[sets][..., :3])
    d[~ok] = 0.0
    out = np.zeros((len(p), K), ray_dtype)
    out["origin"], out["near"], out["far"] = p["position"][:, None, :], p["near"][:, None], p["far"][:, None]
    out["direction"] = d
    return out


def butterfly(values):
    """the sum of (n, K, 3) float32 in the device's order: lane l = k % 64 adds rounds r = 0, 1, ... from +0, then v = v + v[lane ^ off] for
    off = 1, 2, ..., min(K, 64) / 2; the result is lane 0's"""
    values = np.asarray(values, F)
    K = values.shape[1]
    lanes = min(K, 64)
    v = np.zeros((values.shape[0], lanes, 3), F)
    for r in range(K // lanes):
        v = v + values[:, lanes * r:lanes * (r + 1)]
    off = 1
    while off < lanes:
        v = v + v[:, np.arange(lanes) ^ off]
        off *= 2
    return v[:, 0]


def texels(points, ray_array, words):
    """the texels of `points` from their rays ((n, K) ray_dtype, as rays() or the device gives them) and the occlusion word of every ray
    ((n, K), hiprz_query_occluded's): the count, and the butterfly sum of the unoccluded directions; INVALID / +0 for an invalid point"""
    ok = valid(points).reshape(-1)
    words = np.asarray(words).reshape(ray_array.shape)
    out = np.zeros(len(ok), texel_dtype)
    out["occluded"] = np.where(ok, words.sum(-1, dtype=np.uint32), np.uint32(INVALID))
    out["bent"] = butterfly(np.where((words != 0)[..., None], F(0.0), ray_array["direction"]))
    out["bent"][~ok] = 0.0
    return out


def cosine_table(K, S):
    """hiprz_bake_cosine_directions in numpy float64, rounded to float32: (S, K, 4)"""
    k, s = np.arange(K, dtype=np.float64)[None, :], np.arange(S, dtype=np.float64)[:, None]
    u = (k + 0.5) / K
    r = np.sqrt(u)
    turn = k * 0.6180339887498949
    phi = 2.0 * np.pi * ((turn - np.floor(turn)) + s / S)
    out = np.zeros((S, K, 4), np.float64)
    out[..., 0], out[..., 1], out[..., 2] = r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u) + 0.0 * s
    return out.astype(F)
