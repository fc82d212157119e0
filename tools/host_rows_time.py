#!/usr/bin/env python3
"""Host-array calls of the three ray libraries (Context.trace / occluded, plain and ordered, and Context.bake_occlusion at K = 64) on the
host's clock: what the host half of those libraries can move while the kernels stay as they are.  Config C, device-built trees, 2^20
pixel rays, 2^16 surface points, and 1 000 of either (where the call itself, not the walk, is most of the time); the calls timed in turn,
median and `spread` = (max - min) / median of `--repeats` each, one JSON line.

    python tools/host_rows_time.py --label this >> profiles/r22/host_rows.jsonl

HIPRZ_LIB / HIPRZ_QUERY_LIB / HIPRZ_ORDER_LIB / HIPRZ_BAKE_LIB select another build: run the two builds by turns, a process each."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rayzath_amd import bake, order, query, scenes  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing  # noqa: E402
from rayzath_amd.scene import camera_struct, flatten  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--repeats", type=int, default=15)
    args = ap.parse_args()
    preset = scenes.CONFIGS["C"]
    world = preset["build"]()
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx = Context(0)
    ctx.set_tree(3)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(preset["max_depth"], 8)).struct())
    rays = ctx.pixel_rays().reshape(-1)
    rays = rays[:min(len(rays), 1 << 20)].copy()
    hits = ctx.trace(rays)
    found = (hits["flags"] & query.HIT_FOUND) != 0
    r, h = rays[found], hits[found]
    at = np.linspace(0, len(h) - 1, 1 << 16).astype(int)
    points = bake.points(r["origin"][at] + h["t"][at, None] * r["direction"][at], h["normal"][at], 1e-3, 1e3)
    small = rays[:1000].copy()
    calls = {
        "query_closest": lambda: ctx.trace(rays), "query_occluded": lambda: ctx.occluded(rays),
        "order_closest": lambda: ctx.trace(rays, ordered=True), "order_occluded": lambda: ctx.occluded(rays, ordered=True),
        "bake_k64": lambda: ctx.bake_occlusion(points, (64, 4), 0),
        "query_closest_1000": lambda: ctx.trace(small), "order_occluded_1000": lambda: ctx.occluded(small, ordered=True),
        "bake_k64_1000": lambda: ctx.bake_occlusion(points[:1000], (64, 4), 0),
    }
    out = {"label": args.label, "rays": len(rays), "points": len(points), "repeats": args.repeats,
           "libs": [os.path.relpath(m.LIB_PATH, ROOT) for m in (query, order, bake)], "ms": {}}
    for fn in calls.values():
        fn()        # stagings grown, tables placed
    series = {k: [] for k in calls}
    for _ in range(args.repeats):
        for name, fn in calls.items():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            series[name].append((time.perf_counter() - t0) * 1.0e3)
    for name, ms in series.items():
        med = statistics.median(ms)
        out["ms"][name] = {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)}
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
