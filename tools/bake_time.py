#!/usr/bin/env python3
"""Device time of occlusion baking (include/hiprz_bake.h) beside the capability it replaces: hiprz_query_occluded over the SAME n*K rays,
already on the device as hiprz_bake_rays emits them (point-major: the coherence of the bake, and no reduction — both favour the query).
Medians of `--repeats`, HIP events on the context's stream, the two sides timed alternately on one context in one process.

    python tools/bake_time.py --configs C D --out profiles/r21/bake_time.json

Per config: n = 2^16 surface points from the first hits of the pixel rays (evenly spaced over the hit pixels), near_ 1e-3, far_ 1e3, the
cosine table with S = 4, K in 16, 64, 256.  `spread` is (max - min) / median of a series.  The bar: the bake is no slower than the query
by more than three times the larger of the two spreads.  Also, on the host's clock at K = 64: Context.bake_occlusion against the path a
caller had before — numpy rays, Context.occluded, a numpy reduction."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rayzath_amd import _hiprt, bake, query, scenes  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing  # noqa: E402
from rayzath_amd.scene import camera_struct, flatten  # noqa: E402

KS = (16, 64, 256)
SETS = 4
POINTS = 1 << 16


def series(ctx, fns, repeats):
    """the functions timed in turn, `repeats` rounds: one list of milliseconds per function"""
    a, b = _hiprt.Event(), _hiprt.Event()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            a.record(ctx.stream())
            fn()
            b.record(ctx.stream())
            out[k].append(b.ms_since(a))
    a.destroy(), b.destroy()
    return out


def stats(ms):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "spread": (max(ms) - min(ms)) / med}


def surface_points(ctx, n):
    rays = ctx.pixel_rays().reshape(-1)
    hits = ctx.trace(rays)
    found = np.flatnonzero(hits["flags"] & query.HIT_FOUND)
    pick = found[np.linspace(0, len(found) - 1, n).astype(np.int64)]
    r, h = rays[pick], hits[pick]
    return bake.points(r["origin"] + h["t"][:, None] * r["direction"], h["normal"], 1e-3, 1e3)


def numpy_rays(points, table, seed):
    """what a caller without the bake library writes on the host: the rays of every point in float32 (any frame will do for a caller; this
    one is the library's, so the answers can be compared)"""
    F = np.float32
    n = points["normal"] * (F(1) / np.sqrt((points["normal"] ** 2).sum(-1, dtype=F)))[:, None]
    s = np.copysign(F(1), n[:, 2])
    a = F(-1) / (s + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    t = np.stack([F(1) + s * n[:, 0] * n[:, 0] * a, s * b, -s * n[:, 0]], -1)
    bt = np.stack([b, s + n[:, 1] * n[:, 1] * a, -n[:, 1]], -1)
    x = (np.arange(len(points), dtype=np.uint64) ^ np.uint64(seed)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    sets = (x % np.uint64(table.shape[0])).astype(np.int64)
    l = table[sets]
    d = (t[:, None] * l[..., 0:1] + bt[:, None] * l[..., 1:2]) + n[:, None] * l[..., 2:3]
    out = np.zeros(l.shape[:2], query.ray_dtype)
    out["origin"], out["near"], out["far"], out["direction"] = points["position"][:, None], points["near"][:, None], points["far"][:, None], d
    return out


def measure(config, repeats, tree):
    preset = scenes.CONFIGS[config]
    world = preset["build"]()
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx = Context(0)
    ctx.set_tree(tree)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(preset["max_depth"], 8)).struct())
    points = surface_points(ctx, POINTS)
    n = len(points)
    b, q = ctx.bake(), ctx.query()
    d_points, d_texels = _hiprt.DeviceBuffer.of(points), _hiprt.DeviceBuffer(n * 16)
    out = {"config": config, "width": cam.width, "height": cam.height, "points": n, "sets": SETS, "tree": ctx.tree(), "repeats": repeats, "per_k": []}
    for K in KS:
        b.set_directions((K, SETS))
        d_rays, d_words = _hiprt.DeviceBuffer(n * K * 32), _hiprt.DeviceBuffer(n * K * 4)
        b.rays_device(d_points.ptr, n, d_rays.ptr), b.occlusion_device(d_points.ptr, n, d_texels.ptr), q.occluded_device(d_rays.ptr, n * K, d_words.ptr)
        ctx.sync()   # the table is placed, first launches are done
        baked, asked, emitted = series(ctx, [lambda: b.occlusion_device(d_points.ptr, n, d_texels.ptr), lambda: q.occluded_device(d_rays.ptr, n * K, d_words.ptr),
                                             lambda: b.rays_device(d_points.ptr, n, d_rays.ptr)], repeats)
        ctx.sync()
        texels, words = d_texels.download((n,), bake.texel_dtype), d_words.download((n, K), np.uint32)
        assert np.array_equal(texels["occluded"], words.sum(-1)), "the bake's counts are not the query's on the emitted rays"
        d_rays.free(), d_words.free()
        sb, sq = stats(baked), stats(asked)
        allowed = 3.0 * max(sb["spread"], sq["spread"])
        out["per_k"].append({"K": K, "rays": n * K, "occluded_rays": int(words.sum()), "bake": sb, "query_occluded": sq, "bake_rays": stats(emitted),
                             "bake_over_query": sb["median_ms"] / sq["median_ms"], "bar_allowed_excess": allowed,
                             "bar_met": sb["median_ms"] <= sq["median_ms"] * (1.0 + allowed),
                             "bytes_read_per_point": {"bake": 32, "query": 32 * K}, "bytes_written_per_point": {"bake": 16, "query": 4 * K}})
    d_points.free(), d_texels.free()
    # the host's clock, K = 64: the call against the path a caller had before
    K = 64
    table = bake.cosine_directions(K, SETS)
    host = {"bake": [], "rays_query_reduce": [], "of_which_numpy_rays": []}
    for _ in range(5):
        ctx.sync()
        t0 = time.perf_counter()
        texels = ctx.bake_occlusion(points, (K, SETS), 0)
        host["bake"].append((time.perf_counter() - t0) * 1.0e3)
        ctx.sync()
        t0 = time.perf_counter()
        rays = numpy_rays(points, table, 0)
        t1 = time.perf_counter()
        counts = ctx.occluded(rays.reshape(-1)).reshape(n, K).sum(-1)
        host["rays_query_reduce"].append((time.perf_counter() - t0) * 1.0e3)
        host["of_which_numpy_rays"].append((t1 - t0) * 1.0e3)
    out["host_call_k64_ms"] = {k: statistics.median(v) for k, v in host.items()}
    out["host_call_k64_counts_equal"] = bool(np.array_equal(counts, texels["occluded"]))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["C", "D"])
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--tree", type=int, default=3, help="hiprz_set_tree (3 = TREE_DEVICE_SAH: device-built trees)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for config in args.configs:
        lines.append(json.dumps(measure(config, args.repeats, args.tree)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
