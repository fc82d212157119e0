#!/usr/bin/env python3
"""Device time of the ray queries (include/hiprz_query.h) on the pixel rays of a BASELINE config, beside rz_guide_kernel (hiprz_render_guides)
walking the very same rays on the same context in the same run: medians of `--repeats`, HIP events on the context's stream, the two
kernels of a comparison timed alternately.

    python tools/query_time.py --configs C D --out profiles/r16/query_time.json

Per config: rz_query_closest_kernel and rz_query_occluded_kernel on pixel_rays() in pixel order and in a fixed random permutation (what
ray order is worth to a caller), rz_query_pixel_rays_kernel, and host-pointer calls of 2^20 rays on the host's clock.  `spread` is
(max - min) / median of a series.  HIPRZ_QUERY_LIB selects another build of the library (the workgroup-size comparison: --label)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rayzath_amd import _hiprt, query, scenes  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing  # noqa: E402
from rayzath_amd.scene import camera_struct, flatten  # noqa: E402


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


def measure(config, repeats, tree, label):
    preset = scenes.CONFIGS[config]
    world = preset["build"]()
    flat, cam = flatten(world), camera_struct(world.camera)
    W, H = cam.width, cam.height
    n = W * H
    ctx = Context(0)
    ctx.set_tree(tree)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(preset["max_depth"], 8)).struct())
    q = ctx.query()
    rays_host = ctx.pixel_rays().reshape(-1)
    rays = _hiprt.DeviceBuffer.of(rays_host)
    order = np.random.default_rng(20261019).permutation(n)
    shuffled = _hiprt.DeviceBuffer.of(rays_host[order])
    hits, occ, scratch = _hiprt.DeviceBuffer(n * 48), _hiprt.DeviceBuffer(n * 4), _hiprt.DeviceBuffer(n * 32)
    ctx.render_guides(), q.closest_device(rays.ptr, n, hits.ptr), q.occluded_device(rays.ptr, n, occ.ptr)  # allocations, first launches
    ctx.sync()
    guide, closest = series(ctx, [ctx.render_guides, lambda: q.closest_device(rays.ptr, n, hits.ptr)], repeats)
    found = int((hits.download((n,), query.hit_dtype)["flags"] & query.HIT_FOUND != 0).sum())
    occluded, closest_shuffled, occluded_shuffled, pixel_rays = series(ctx, [
        lambda: q.occluded_device(rays.ptr, n, occ.ptr), lambda: q.closest_device(shuffled.ptr, n, hits.ptr),
        lambda: q.occluded_device(shuffled.ptr, n, occ.ptr), lambda: q.pixel_rays_device(scratch.ptr)], repeats)
    assert int(occ.download((n,), np.uint32).sum()) == found
    m = min(n, 1 << 20)
    host = {"closest": [], "occluded": []}
    for _ in range(5):
        for name, fn in (("closest", ctx.trace), ("occluded", ctx.occluded)):
            ctx.sync()
            t0 = time.perf_counter()
            fn(rays_host[:m])
            host[name].append((time.perf_counter() - t0) * 1.0e3)
    for buf in (rays, shuffled, hits, occ, scratch):
        buf.free()
    got_tree = ctx.tree()
    ctx.close()
    g, c = stats(guide), stats(closest)
    allowed = 3.0 * max(g["spread"], c["spread"])
    return {"config": config, "width": W, "height": H, "rays": n, "found": found, "tree": got_tree, "label": label, "repeats": repeats,
            "library": os.path.basename(query.LIB_PATH),
            "guide_kernel": g, "closest": c, "closest_over_guide": c["median_ms"] / g["median_ms"], "bar_allowed_excess": allowed,
            "bar_met": c["median_ms"] <= g["median_ms"] * (1.0 + allowed),
            "occluded": stats(occluded), "closest_shuffled": stats(closest_shuffled), "occluded_shuffled": stats(occluded_shuffled),
            "shuffled_over_ordered_closest": statistics.median(closest_shuffled) / c["median_ms"],
            "shuffled_over_ordered_occluded": statistics.median(occluded_shuffled) / statistics.median(occluded),
            "pixel_rays": stats(pixel_rays), "host_rays": m, "closest_host_call_ms": statistics.median(host["closest"]),
            "occluded_host_call_ms": statistics.median(host["occluded"]),
            "bytes_per_ray": {"closest": 32 + 48, "occluded": 32 + 4, "guide": 32}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["C", "D"])
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--tree", type=int, default=4, help="hiprz_set_tree (4 = TREE_AUTO, what bench.py renders with)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    lines = []
    for config in args.configs:
        lines.append(json.dumps(measure(config, args.repeats, args.tree, args.label)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
