"""Probe fields (include/hiprz_field.h) restated in numpy float32, one rounding per operation like the device build (-ffp-contract=off):
the texel directions in float64, the octahedral texel of a direction, the moments of a visibility map over the rays and distances the
device (or an analytic scene) gives, the record with its words, and the lookup with its Chebyshev weights.  The rays are hiprz_bake.h's
(tests/bake_reference.py), the evaluation hiprz_probe.h's (tests/probe_reference.py).  For tests/test_field_reference.py (CPU) and
tests/test_field_gpu.py, which holds the device's records and results to visibility_records() and lookup() in every byte.

MUTANTS, each a wrong reading of the header that the tests must tell from the right one:
  descending  the K rays added in descending order
  c16         w = c^16, four squarings
  unclamped   r = t, not min(t, reach)
  nomean2     var = fabsf(mean2), the mean*mean left out
  corners     the eight corners taken in the order 7 .. 0
  nocrush     the w < 0.2 crush left out
  nofold      the fold of the lower hemisphere without its copysignf factors: every z < 0 direction lands in the ++ quadrant"""
import numpy as np

import bake_reference as BR
import probe_reference as PR
from rayzath_amd.bake import point_dtype
from rayzath_amd.field import INVALID, grid_dtype, params_dtype, result_dtype, vis_dtype
from rayzath_amd.probe import INVALID as PROBE_INVALID
from rayzath_amd.probe import sh_dtype
from rayzath_amd.query import HIT_EXTERNAL, HIT_FOUND

F = np.float32
VIS_MUTANTS = ("descending", "c16", "unclamped")
LOOKUP_MUTANTS = ("nomean2", "corners", "nocrush", "nofold")
MUTANTS = VIS_MUTANTS + LOOKUP_MUTANTS


def texel_directions64():
    """ "THE TEXEL DIRECTIONS" in float64: (64, 3), texel j = 8 * iy + ix"""
    iy, ix = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    ex, ey = (ix + 0.5) / 4.0 - 1.0, (iy + 0.5) / 4.0 - 1.0
    z = 1.0 - np.abs(ex) - np.abs(ey)
    x = np.where(z < 0, (1.0 - np.abs(ey)) * np.where(ex < 0, -1.0, 1.0), ex)
    y = np.where(z < 0, (1.0 - np.abs(ex)) * np.where(ey < 0, -1.0, 1.0), ey)
    d = np.stack([x, y, z], -1).reshape(64, 3)
    return d / np.sqrt((d * d).sum(-1, keepdims=True))


def texel_of(direction, mutant=None):
    """the texel j of float32 directions (..., 3): the header's encode with its total clamp"""
    d = np.asarray(direction, F)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(all="ignore"):
        s = (np.abs(x) + np.abs(y)) + np.abs(z)
        ex, ey = x / s, y / s
        if mutant == "nofold":
            sx = sy = F(1.0)
        else:
            sx, sy = np.copysign(F(1.0), ex), np.copysign(F(1.0), ey)
        fx = np.where(z < 0, (F(1.0) - np.abs(ey)) * sx, ex)
        fy = np.where(z < 0, (F(1.0) - np.abs(ex)) * sy, ey)
        tx = np.fmin(np.fmax(np.floor((fx * F(0.5) + F(0.5)) * F(8.0)), F(0.0)), F(7.0)).astype(np.int64)
        ty = np.fmin(np.fmax(np.floor((fy * F(0.5) + F(0.5)) * F(8.0)), F(0.0)), F(7.0)).astype(np.int64)
    return 8 * ty + tx


def moments(directions, r, reach, mutant=None):
    """ "THE MOMENTS": (n, 64, 2) float32 from the rays' directions (n, K, 3) and distances r (n, K), both float32"""
    d, r = np.asarray(directions, F), np.asarray(r, F)
    n, K = r.shape
    o = texel_directions64().astype(F)
    ox, oy, oz = o[None, :, 0], o[None, :, 1], o[None, :, 2]
    sw, s1, s2 = np.zeros((n, 64), F), np.zeros((n, 64), F), np.zeros((n, 64), F)
    for k in (range(K - 1, -1, -1) if mutant == "descending" else range(K)):
        dk, rk = d[:, k, None, :], r[:, k, None]
        c = np.maximum(F(0.0), (ox * dk[..., 0] + oy * dk[..., 1]) + oz * dk[..., 2])
        w = c * c
        for _ in range(3 if mutant == "c16" else 4):
            w = w * w
        sw = sw + w
        s1 = s1 + (w * rk)
        s2 = s2 + (w * (rk * rk))
    reach = F(reach)
    with np.errstate(all="ignore"):
        return np.stack([np.where(sw > 0, s1 / sw, reach), np.where(sw > 0, s2 / sw, reach * reach)], -1).astype(F)


def records(ok, directions, r, counts, reach, mutant=None):
    """the records of n probes: `ok` (n,) valid, moments of (directions, r), words = counts (n, 3) of front, back, missed and K"""
    n, K = np.asarray(r).shape
    out = np.zeros(n, vis_dtype)
    out["moments"] = moments(directions, r, reach, mutant)
    out["words"][:, :3], out["words"][:, 3] = counts, K
    out["moments"][~ok], out["words"][~ok] = 0.0, (0, 0, 0, INVALID)
    return out


def visibility_records(probes, rays, hits, reach, mutant=None):
    """the records hiprz_field_visibility writes for 1-d `probes` from their rays ((n, K) query.ray_dtype, bake_reference.rays() or the
    device's) and the closest hit of every ray ((n, K) query.hit_dtype, hiprz_query_closest's without NORMALIZE)"""
    found = (hits["flags"] & HIT_FOUND) != 0
    front = found & ((hits["flags"] & HIT_EXTERNAL) != 0)
    t = hits["t"].astype(F)
    r = np.where(found, t if mutant == "unclamped" else np.minimum(t, F(reach)), F(reach)).astype(F)
    counts = np.stack([front.sum(1), (found & ~front).sum(1), (~found).sum(1)], -1)
    return records(BR.valid(probes).reshape(-1), rays["direction"], r, counts, reach, mutant)


def point_valid(points):
    p = np.ascontiguousarray(points).view(point_dtype)
    n = p["normal"].astype(F)
    with np.errstate(all="ignore"):
        sq = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        return np.isfinite(p["position"]).all(-1) & np.isfinite(n).all(-1) & (sq >= F(0.99)) & (sq <= F(1.01))


def _length(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def visible(vis, P, p, n, bias, mutant=None):
    """the factor the visibility records `vis` (m,) of the probes at P (m, 3) give the points p with normals n: (m,) float32"""
    one = F(1.0)
    with np.errstate(all="ignore"):
        v = (p + (F(bias) * n)) - P
        dist = _length(v)
        u = P - p
        length = _length(u)
        uh = u / length[..., None]
        b = (((uh[..., 0] * n[..., 0] + uh[..., 1] * n[..., 1]) + uh[..., 2] * n[..., 2]) + one) * F(0.5)
        wb = np.where(length != 0, (b * b) + F(0.2), one)
        j = texel_of(v / dist[..., None], mutant)
        pair = vis["moments"][np.arange(len(vis)), j]
        mean, mean2 = pair[:, 0], pair[:, 1]
        var = np.abs(mean2) if mutant == "nomean2" else np.abs(mean2 - mean * mean)
        dd = dist - mean
        ch = var / (var + dd * dd)
        ch = np.where(dist > mean, (ch * ch) * ch, one)
        wb, ch = np.where(dist != 0, wb, one), np.where(dist != 0, ch, one)
        w = np.fmax(wb * ch, F(1.0e-6))
        if mutant != "nocrush":
            w = np.where(w < F(0.2), w * ((w * w) * F(25.0)), w)
    return w.astype(F)


def lookup(grid, probes, sh, vis, params, points, mutant=None):
    """the results hiprz_field_lookup writes for 1-d `points`: result_dtype (m,)"""
    grid, params = np.asarray(grid).reshape(()), np.asarray(params).reshape(())
    assert grid.dtype == grid_dtype and params.dtype == params_dtype
    probes, sh = np.ascontiguousarray(probes).reshape(-1).view(point_dtype), np.ascontiguousarray(sh).reshape(-1).view(sh_dtype)
    pts = np.ascontiguousarray(points).reshape(-1).view(point_dtype)
    m = len(pts)
    ok = point_valid(pts)
    p, n = np.where(ok[:, None], pts["position"], F(0.0)).astype(F), np.where(ok[:, None], pts["normal"], F(0.0)).astype(F)
    counts = [int(c) for c in grid["n"]]
    cell, frac = [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            g = (p[:, a] - grid["lo"][a]) / grid["step"][a] if counts[a] > 1 else np.zeros(m, F)
            g = np.fmin(np.fmax(g, F(0.0)), F(counts[a] - 1)).astype(F)
            i = np.minimum(np.floor(g).astype(np.int64), counts[a] - 2) if counts[a] > 1 else np.zeros(m, np.int64)
            cell.append(i), frac.append(g - i.astype(F))
    words = sh["sh"][:, 0, 3].view(np.uint32)
    usable = words != PROBE_INVALID
    if vis is not None:
        vis = np.ascontiguousarray(vis).reshape(-1).view(vis_dtype)
        usable = usable & (vis["words"][:, 3] != INVALID) & (vis["words"][:, 1] <= params["max_back"])
    acc, sw, counted = np.zeros((m, 3), F), np.zeros(m, F), np.zeros(m, np.uint32)
    for corner in (range(7, -1, -1) if mutant == "corners" else range(8)):
        idx, tri = [], None
        for a in range(3):
            up = (corner >> a) & 1
            idx.append(np.minimum(cell[a] + up, counts[a] - 1))
            wa = frac[a] if up else F(1.0) - frac[a]
            tri = wa if tri is None else tri * wa
        index = (idx[0] * counts[1] + idx[1]) * counts[2] + idx[2]
        w = tri
        if vis is not None:
            w = visible(vis[index], probes["position"][index].astype(F), p, n, params["bias"], mutant) * tri
        w = np.where(usable[index], w, F(0.0)).astype(F)
        with np.errstate(all="ignore"):
            E = PR.irradiance(sh["sh"][index][..., :3], n, F)
            E = np.where(usable[index][:, None], E, F(0.0)).astype(F)          # (a probe left out adds nothing, whatever its record holds)
            acc = np.where(usable[index][:, None], acc + (w[:, None] * E), acc)
            sw = np.where(usable[index], sw + w, sw)
        counted = counted + (usable[index] & (w > 0))
    out = np.zeros(m, result_dtype)
    good = ok & (sw > 0)
    with np.errstate(all="ignore"):
        out["rgb"] = np.where(good[:, None], acc / sw[:, None], F(0.0))
    out["word"] = np.where(good, counted, np.uint32(INVALID))
    return out


# --- the two rooms of the issue: axis-aligned, closed, 0.2 apart; probes 1 apart; analytic distances ---
ROOMS = (((-2.0, 0.0, -1.0), (-0.1, 2.0, 1.0)), ((0.1, 0.0, -1.0), (2.0, 2.0, 1.0)))
ROOM_LO, ROOM_HI, ROOM_SHAPE = (-1.5, 0.5, -0.5), (1.5, 1.5, 0.5), (4, 2, 2)
LEAK_POINTS = ((0.3, 1.0, 0.1), (0.15, 0.7, -0.3))


def room_distances(origin, direction):
    """the distance from origins (n, 3) inside one of ROOMS along directions (n, K, 3) to that room's wall, in float64: (n, K)"""
    o, d = np.asarray(origin, np.float64)[:, None, :], np.asarray(direction, np.float64)
    out = np.full(d.shape[:2], np.inf)
    for lo, hi in ROOMS:
        lo, hi = np.asarray(lo), np.asarray(hi)
        inside = ((o > lo) & (o < hi)).all(-1)
        with np.errstate(all="ignore"):
            t = np.where(d > 0, (hi - o) / d, np.where(d < 0, (lo - o) / d, np.inf)).min(-1)
        out = np.where(inside, t, out)
    return out


def two_rooms(K, reach=4.0, seed=0):
    """(grid, probes (4, 2, 2), sh, vis) of the issue's two rooms on the CPU: sh[0] = 1 in the first room and 0 in the second, the
    visibility records from the sphere table's rays and the analytic distances"""
    from rayzath_amd import field, probe
    probes = probe.grid(ROOM_LO, ROOM_HI, ROOM_SHAPE)
    flat = probes.reshape(-1)
    rays = BR.rays(flat, PR.sphere_table(K, 1), seed)
    t = room_distances(flat["position"], rays["direction"])
    assert np.isfinite(t).all()
    r = np.minimum(t.astype(F), F(reach))
    vis = records(np.ones(len(flat), bool), rays["direction"], r, np.stack([np.full(len(flat), K), np.zeros(len(flat), int), np.zeros(len(flat), int)], -1), reach)
    sh = np.zeros(len(flat), sh_dtype)
    sh["sh"][flat["position"][:, 0] < 0, 0, :3] = 1.0
    return field.grid_of(ROOM_LO, ROOM_HI, ROOM_SHAPE), probes, sh, vis
