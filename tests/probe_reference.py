"""Probe baking (include/hiprz_probe.h) restated in numpy, one rounding per operation like the device build (-ffp-contract=off): the basis,
the gathered term over the samples and rays the device emits, the light term's sampling without its cosine and its sum over verdicts, the
fixed-order sum with its butterfly, the record with its words, the sphere table in float64 and the evaluation.  Every function that does
arithmetic takes its dtype: float32 is the device's, float64 the yardstick the float32 evaluation is measured against (its sums are then
plain sums).  The rays are hiprz_bake.h's (tests/bake_reference.py), the contributions hiprz_gather.h's (tests/gather_reference.py), the
frame and the vector functions hiprz_light.h's (tests/light_reference.py).  For tests/test_probe_reference.py (CPU) and
tests/test_probe_gpu.py, which holds the device's records to gather_records() and light_records() in every byte.

MUTANTS, each a wrong reading of the header that the tests must tell from the right one:
  swap     B1 and B3 exchanged (d.y and d.x)
  b6       B6 without the - 1
  quarter  the 0.25f of the light term missing
  cosine   the cosine left in the light weight, with its c > 0 test
  order    the K terms added one after the other instead of per lane and by the butterfly"""
import numpy as np

import bake_reference as BR
import gather_reference as GR
import light_reference as LR
from rayzath_amd.bake import point_dtype
from rayzath_amd.probe import INVALID, sh_dtype

F = np.float32
PI_F = LR.PI_F
MUTANTS = ("swap", "b6", "quarter", "cosine", "order")
WEIGHTS = (1.0, 2.0, 2.0, 2.0, 15.0 / 4.0, 15.0 / 4.0, 5.0 / 16.0, 15.0 / 4.0, 15.0 / 16.0)
valid = BR.valid


def basis(d, mutant=None):
    """ "THE BASIS" on d (..., 3) in d's dtype: (..., 9)"""
    d = np.asarray(d)
    T = d.dtype.type
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    b1, b3 = (x, y) if mutant == "swap" else (y, x)
    b6 = T(3.0) * (z * z) if mutant == "b6" else (T(3.0) * (z * z)) - T(1.0)
    return np.stack([np.ones_like(x), b1, z, b3, x * y, y * z, b6, x * z, (x * x) - (y * y)], -1)


def fixed_sum(terms, mutant=None):
    """the sum over axis 1 of (n, K, ...) in the device's order, in the terms' dtype: lane j = k % 64 adds rounds r = 0, 1, ... from +0,
    then v = v + v[lane ^ off] for off = 1, 2, ..., min(K, 64) / 2; the result is lane 0's.  float64 terms: a plain sum."""
    terms = np.asarray(terms)
    if terms.dtype == np.float64:
        return terms.sum(1)
    K = terms.shape[1]
    if mutant == "order":
        total = np.zeros(terms.shape[:1] + terms.shape[2:], terms.dtype)
        for k in range(K):
            total = total + terms[:, k]
        return total
    lanes = min(K, 64)
    v = np.zeros((terms.shape[0], lanes) + terms.shape[2:], terms.dtype)
    for r in range(K // lanes):
        v = v + terms[:, lanes * r:lanes * (r + 1)]
    off = 1
    while off < lanes:
        v = v + v[:, np.arange(lanes) ^ off]
        off *= 2
    return v[:, 0]


def project(values, directions, dtype=F, mutant=None):
    """(n, 9, 3): per coefficient and colour the mean of values (n, K, 3) * B_b(directions (n, K, 3)) — acc = acc + (L.c * B_b) in the
    fixed order, then * (1 / K)"""
    T = dtype
    with np.errstate(all="ignore"):
        terms = np.asarray(values).astype(T)[:, :, None, :] * basis(np.asarray(directions).astype(T), mutant)[:, :, :, None]
        return fixed_sum(terms, mutant) * (T(1.0) / T(terms.shape[1]))


def invalid_records(n):
    out = np.zeros(n, sh_dtype)
    out["sh"][:, 0, 3] = np.array([INVALID], np.uint32).view(F)[0]
    return out


def gather_records(probes, samples, rays, charts, source, W, H, sky, mutant=None):
    """the records hiprz_probe_gather writes for 1-d `probes` from their samples ((n, K) gather.sample_dtype) and their rays ((n, K)
    query.ray_dtype, as bake_reference.rays() or the device gives them)"""
    ok = valid(probes).reshape(-1)
    s = np.asarray(samples).reshape(len(ok), -1)
    values, read, missed = GR.contributions(s, charts, source, W, H, sky)
    out = np.zeros(len(ok), sh_dtype)
    out["sh"][:, :, :3] = project(values, np.asarray(rays).reshape(s.shape)["direction"], F, mutant)
    counts = read.sum(-1, dtype=np.uint32) | (missed.sum(-1, dtype=np.uint32) << np.uint32(16))
    out["sh"][:, 0, 3] = counts.view(F)
    out[~ok] = invalid_records(int((~ok).sum()))
    return out


def gather_exact(samples, rays, charts, source, W, H, sky):
    """(mean (n, 9, 3), magnitude (n, 9)) in float64 from the same samples and rays: the same rules, the sum exact to float64; magnitude
    is mean over k and colours' maximum of |L.c * B_b|, what the summation bound is stated in"""
    s = np.asarray(samples)
    values, _, _ = GR.contributions(s, charts, source, W, H, sky)
    d = np.asarray(rays)["direction"].astype(np.float64)
    terms = values.astype(np.float64)[:, :, None, :] * basis(d)[:, :, :, None]
    return terms.mean(1), np.abs(terms).mean(1)


def light_samples(probes, spots, directs, table, seed, dtype=F, mutant=None):
    """(w3 (n, L, K, 3), far (n, L, K), w (n, L, K), kept (n, L, K)) of 1-d `probes` under the disk `table` ((S, K, 2) float32): "THE LIGHT
    TERM" up to the shadow ray, hiprz_light.h's rules with the cosine taken out.  A sample not kept has w3 = 0, far = the probe's, w = +0."""
    p = np.ascontiguousarray(probes).reshape(-1).view(point_dtype)
    table = np.asarray(table, F)
    S, K = table.shape[:2]
    ok = valid(p)
    T = dtype
    n_lights = len(spots) + len(directs)
    w3, fars, w, kept = np.zeros((len(p), n_lights, K, 3), T), np.zeros((len(p), n_lights, K), T), np.zeros((len(p), n_lights, K), T), np.zeros((len(p), n_lights, K), bool)
    with np.errstate(all="ignore"):
        position, far = p["position"].astype(T), p["far"]
        n = LR._normalized(p["normal"].astype(T))
        xy = table[BR.set_of(np.arange(len(p)), seed, S)]
        for l, light in enumerate(list(spots) + list(directs)):
            if l < len(spots):
                lpos, ldir, size, cos_angle = light["position"].astype(T), light["direction"].astype(T), T(light["size"]), T(light["cos_angle"])
                x, y = xy[..., 0:1].astype(T), xy[..., 1:2].astype(T)
                a = LR._normalized(lpos - position)
                t, bt = BR.frame(a)
                q = lpos + ((t[:, None] * x + bt[:, None] * y) * size)
                vPL = q - position[:, None]
                dPL = LR._magnitude(vPL)
                omega = LR._normalized(vPL)
                A = (size * size) * T(PI_F)
                d1 = dPL + T(1.0)
                inside = cos_angle < LR._similarity(-vPL, ldir)
                weight = np.where(inside, A / (d1 * d1), T(0.0))
                reach = dPL
            else:
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
                omega = LR._normalized(d)
                weight = np.broadcast_to((T(2.0) * T(PI_F)) * (T(1.0) - ca), z.shape)
                reach = np.broadcast_to(far[:, None].astype(T), z.shape)
            if mutant == "cosine":
                c = LR._dot(n[:, None], omega)
                weight = np.where(c > 0, c * weight, T(0.0))
            keep = ok[:, None] & (weight > 0) & (light["emission"] > 0) & np.isfinite(omega).all(-1) & np.isfinite(reach) & np.isfinite(weight)
            w3[:, l], fars[:, l] = np.where(keep[..., None], omega, T(0.0)), np.where(keep, reach, far[:, None].astype(T))
            w[:, l], kept[:, l] = np.where(keep, weight, T(0.0)), keep
    return w3, fars, w, kept


def light_rays(probes, spots, directs, table, seed, lights=None, mutant=None):
    """(rays (n, L, K) query.ray_dtype, weights (n, L, K) float32): the shadow rays the light term walks and their weights"""
    from rayzath_amd.query import ray_dtype
    spots, directs = LR.select(spots, directs, lights)
    p = np.ascontiguousarray(probes).reshape(-1).view(point_dtype)
    w3, far, w, _ = light_samples(p, spots, directs, table, seed, F, mutant)
    out = np.zeros(w.shape, ray_dtype)
    out["origin"], out["near"] = p["position"][:, None, None, :], p["near"][:, None, None]
    out["direction"], out["far"] = w3, far
    return out, w


def light_term(w3, weights, occluded, ce, dtype=F, mutant=None):
    """(n, 9, 3): the light term from the directions (n, L, K, 3) and weights (n, L, K) of the samples, the occlusion word of every ray
    and colour * emission per light (light_reference.colour_emission()): per lane the lights in order and the rounds in order, the
    butterfly, then * (1 / K)"""
    T = dtype
    weights = np.asarray(weights)
    n, L, K = weights.shape
    adds = (weights > 0) & (np.asarray(occluded).reshape(weights.shape) == 0)
    quarter = T(1.0) if mutant == "quarter" else T(0.25)
    with np.errstate(all="ignore"):
        P = (np.asarray(ce).astype(T)[None, :, None, :] * weights.astype(T)[..., None]) * quarter
        P = np.where(adds[..., None], P, T(0.0))
        terms = P[:, :, :, None, :] * basis(np.asarray(w3).astype(T), "swap" if mutant == "swap" else ("b6" if mutant == "b6" else None))[:, :, :, :, None]
        if T is np.float64:
            return terms.sum((1, 2)) * (1.0 / K)
        lanes = min(K, 64)
        # rounds within a light, lights one after the other: a sequence of L * (K / lanes) rounds of `lanes` lanes
        seq = terms.reshape(n, L * (K // lanes), lanes, 9, 3)
        if mutant == "order":
            seq = seq[:, ::-1]
        v = np.zeros((n, lanes, 9, 3), T)
        for r in range(seq.shape[1]):
            v = v + seq[:, r]
        off = 1
        while off < lanes:
            v = v + v[:, np.arange(lanes) ^ off]
            off *= 2
        return v[:, 0] * (T(1.0) / T(K))


def light_records(probes, w3, weights, occluded, ce, base=None, mutant=None):
    """the records hiprz_probe_light writes for 1-d `probes`: base.sh[b].c + light[b].c (+0 + light without `base`), sh[0].w of the base,
    sh[1].w the number of walked rays found occluded; the invalid record for an invalid probe or an invalid base record"""
    ok = valid(probes).reshape(-1)
    weights = np.asarray(weights, F)
    out = np.zeros(len(ok), sh_dtype)
    below = np.zeros(len(ok), sh_dtype) if base is None else np.ascontiguousarray(base).reshape(-1).view(sh_dtype)
    with np.errstate(all="ignore"):
        out["sh"][:, :, :3] = below["sh"][:, :, :3] + light_term(w3, weights, occluded, ce, F, mutant)
    out["sh"][:, 0, 3] = below["sh"][:, 0, 3]
    count = ((np.asarray(occluded).reshape(weights.shape) != 0) & (weights > 0)).sum((1, 2), dtype=np.uint32)
    out["sh"][:, 1, 3] = count.view(F)
    bad = ~ok | (below["sh"][:, 0, 3].view(np.uint32) == INVALID)
    out[bad] = invalid_records(int(bad.sum()))
    return out


def sphere_table(K, S):
    """hiprz_probe_sphere_directions in numpy float64, rounded to float32: (S, K, 4)"""
    k, s = np.arange(K, dtype=np.float64)[None, :], np.arange(S, dtype=np.float64)[:, None]
    z = np.broadcast_to(1.0 - 2.0 * (k + 0.5) / K, (S, K))
    r = np.sqrt(1.0 - z * z)
    turn = k * 0.6180339887498949
    phi = 2.0 * np.pi * ((turn - np.floor(turn)) + s / S)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z, np.zeros_like(z)], -1).astype(F)


def irradiance(coefficients, normals, dtype=np.float64):
    """E(n) of coefficients (..., 9, 3) for normals (..., 3): sum over b of w_b * sh[b].c * B_b(n), in `dtype` and in the header's order"""
    T = dtype
    c, B = np.asarray(coefficients).astype(T), basis(np.asarray(normals).astype(T))
    e = np.zeros(np.broadcast_shapes(c.shape[:-2], B.shape[:-1]) + (3,), T)
    for b in range(9):
        e = e + ((T(WEIGHTS[b]) * c[..., b, :]) * B[..., b, None])
    return e
