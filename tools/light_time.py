#!/usr/bin/env python3
"""Device time of light baking (include/hiprz_light.h) beside the best route there was before it: hiprz_query_occluded over the SAME n*L*K
shadow rays, already on the device as hiprz_light_rays emits them (point-major: the coherence of the bake, no host copy and no reduction —
all of that favours the query; the skipped samples are flagged invalid there and are not walked by either side).  Medians of `--repeats`,
HIP events on the context's stream, the two sides timed alternately on one context in one process.

    python tools/light_time.py --configs E D --out profiles/r26/light_time.json

Per config: n = 2^16 surface points from the first hits of the pixel rays (evenly spaced over the hit pixels), near_ 1e-3, far_ 1e3, the disk
table with S = 4, K in 16, 64.  Config E bakes its own three spot lights and one direct light; config D has none, so the tool adds one
direct and two spot lights (E's, the room is the same).  `spread` is (max - min) / median of a series.  The bar: the bake is no slower than
the query by more than three times the larger of the two spreads.  A figure is kept only when the bake's `shadowed` equals the sum of the
query's words per point.  Also, on the host's clock at K = 16: Context.bake_light against the path a caller had before — numpy rays and
weights, Context.occluded, a numpy reduction."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import light_reference as LR  # noqa: E402  (the host route's rays: the float32 restatement, what a caller would have to write)
from rayzath_amd import _hiprt, bake, light, query, scenes  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing  # noqa: E402
from rayzath_amd.scene import DirectLight, SpotLight, camera_struct, flatten  # noqa: E402

KS = (16, 64)
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


def lit_world(config):
    world = scenes.CONFIGS[config]["build"]()
    if not world.spot_lights and not world.direct_lights:      # config D: E's first two spot lights and its direct light, in the same room
        world.add(SpotLight(position=(-1.2, 2.7, -1.0), direction=(0.4, -1.0, 0.5), color=(255, 240, 220, 255), size=0.15, emission=120.0, beam_angle=0.9))
        world.add(SpotLight(position=(1.2, 2.7, 0.5), direction=(-0.3, -1.0, 0.0), color=(220, 230, 255, 255), size=0.1, emission=90.0, beam_angle=0.7))
        world.add(DirectLight(direction=(0.3, -1.0, 0.8), color=(255, 250, 240, 255), emission=30.0, angular_size=0.05))
    return world


def measure(config, repeats, tree):
    world = lit_world(config)
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx = Context(0)
    ctx.set_tree(tree)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(scenes.CONFIGS[config]["max_depth"], 8)).struct())
    points = surface_points(ctx, POINTS)
    n, L = len(points), len(flat.spot_lights) + len(flat.direct_lights)
    h, q = ctx.light(), ctx.query()
    d_points, d_texels = _hiprt.DeviceBuffer.of(points), _hiprt.DeviceBuffer(n * 16)
    out = {"config": config, "width": cam.width, "height": cam.height, "points": n, "spot_lights": len(flat.spot_lights), "direct_lights": len(flat.direct_lights),
           "sets": SETS, "tree": ctx.tree(), "repeats": repeats, "per_k": []}
    for K in KS:
        h.set_samples((K, SETS))
        rays_n = n * L * K
        d_rays, d_weights, d_words = _hiprt.DeviceBuffer(rays_n * 32), _hiprt.DeviceBuffer(rays_n * 4), _hiprt.DeviceBuffer(rays_n * 4)
        h.rays_device(d_points.ptr, n, d_rays.ptr, d_weights.ptr), h.bake_device(d_points.ptr, n, d_texels.ptr), q.occluded_device(d_rays.ptr, rays_n, d_words.ptr)
        ctx.sync()   # the table is placed, first launches are done
        baked, asked, emitted = series(ctx, [lambda: h.bake_device(d_points.ptr, n, d_texels.ptr), lambda: q.occluded_device(d_rays.ptr, rays_n, d_words.ptr),
                                             lambda: h.rays_device(d_points.ptr, n, d_rays.ptr, d_weights.ptr)], repeats)
        ctx.sync()
        texels, words = d_texels.download((n,), light.texel_dtype), d_words.download((n, L * K), np.uint32)
        weights = d_weights.download((n, L * K), np.float32)
        assert np.array_equal(texels["shadowed"], words.sum(-1)), "the bake's shadowed counts are not the query's on the emitted rays"      # the gate: no figure without it
        d_rays.free(), d_weights.free(), d_words.free()
        sb, sq = stats(baked), stats(asked)
        allowed = 3.0 * max(sb["spread"], sq["spread"])
        out["per_k"].append({"K": K, "rays": rays_n, "walked_rays": int((weights > 0).sum()), "shadowed_rays": int(words.sum()), "bake": sb, "query_occluded": sq,
                             "light_rays": stats(emitted), "bake_over_query": sb["median_ms"] / sq["median_ms"], "bar_allowed_excess": allowed,
                             "bar_met": sb["median_ms"] <= sq["median_ms"] * (1.0 + allowed),
                             "bytes_read_per_point": {"bake": 32, "query": 32 * L * K}, "bytes_written_per_point": {"bake": 16, "query": 4 * L * K}})
    d_points.free(), d_texels.free()
    # the host's clock, K = 16: the call against the path a caller had before
    K = 16
    table = light.disk_samples(K, SETS)
    ce = LR.colour_emission(flat.spot_lights, flat.direct_lights)
    host = {"bake_light": [], "rays_query_reduce": [], "of_which_numpy_rays": []}
    for _ in range(3):
        ctx.sync()
        t0 = time.perf_counter()
        texels = ctx.bake_light(points, (K, SETS), 0)
        host["bake_light"].append((time.perf_counter() - t0) * 1.0e3)
        ctx.sync()
        t0 = time.perf_counter()
        rays, weights = LR.rays(points, flat.spot_lights, flat.direct_lights, table, 0)
        t1 = time.perf_counter()
        words = ctx.occluded(rays.reshape(-1)).reshape(rays.shape)
        summed = (np.where(words[..., None] != 0, np.float32(0), ce[None, :, None, :] * weights[..., None]).sum((1, 2), dtype=np.float32) / np.float32(K))
        host["rays_query_reduce"].append((time.perf_counter() - t0) * 1.0e3)
        host["of_which_numpy_rays"].append((t1 - t0) * 1.0e3)
    out["host_call_k16_ms"] = {k: statistics.median(v) for k, v in host.items()}
    out["host_call_k16_shadowed_equal"] = bool(np.array_equal(words.sum((1, 2)), texels["shadowed"]))
    out["host_call_k16_largest_light_difference"] = float(np.abs(summed - texels["light"]).max() / max(float(np.abs(texels["light"]).max()), 1e-30))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["E", "D"])
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
