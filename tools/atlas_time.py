#!/usr/bin/env python3
"""Device time of bake atlases (include/hiprz_atlas.h) beside the bake they feed and the host path they replace.  Medians of `--repeats`,
HIP events on the context's stream, the steps timed in turn on one context in one process.

    python tools/atlas_time.py --out profiles/r25/atlas_time.json
    HIPRZ_ATLAS_LIB=<a libhiprz_atlas.so built with other ATLAS_DEFS> python tools/atlas_time.py --only-add --label helpers32

Per case — sphere charts of 224 triangles (generate_sphere(16)) and of 101 760 (generate_sphere(320)) in 1024^2 and 4096^2 atlases, placed
as the scaled sphere of a small world (a floor, a sphere of scale (2, 0.5, 3), a cube):
  add      hiprz_atlas_begin + hiprz_atlas_add over triangles already on the device: clear, cover and points kernels
  bake     hiprz_bake_occlusion at K = 64, S = 4 over the atlas's points into the handle's records
  dilate   two rings of hiprz_atlas_dilate on those records
  host     (--host, 1024^2 only) the same points made by tests/atlas_reference.py in numpy and uploaded, on the host's clock, once; the
           device's points and samples are compared with them byte for byte
`spread` is (max - min) / median of a series.  --only-add times the first step alone: for comparing launch shapes of the cover kernel."""
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
from rayzath_amd import _hiprt, atlas, bake  # noqa: E402
from rayzath_amd.engine import Context  # noqa: E402
from rayzath_amd.scene import Camera, Instance, Material, World, camera_struct, flatten, generate_cube, generate_plane, generate_sphere  # noqa: E402

K, SETS, RINGS = 64, 4, 2
NEAR, FAR = 1e-3, 1e3
SPHERE = 1      # the instance the charts are placed as


def world():
    w = World()
    grey = w.add(Material((200, 200, 200, 255), 0.0, 0.8, name="grey"))
    plane, sphere, cube = w.add(generate_plane(4)), w.add(generate_sphere(16)), w.add(generate_cube())
    w.add(Instance(plane, [grey], scale=(4, 1, 4), name="floor"))
    w.add(Instance(sphere, [grey], position=(0.6, 0.5, 0.4), rotation=(0, 0.6, 0), scale=(2, 0.5, 3), name="sphere"))
    w.add(Instance(cube, [grey], position=(-1.6, 0.5, -1.2), rotation=(0, 0.4, 0), scale=(1, 1, 1.5), name="cube"))
    w.camera = Camera(position=(0, 3, -8), resolution=(64, 48))
    w.camera.look_at((0, 0, 0))
    return w


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


def measure(ctx, flat, name, tris, size, repeats, only_add, host):
    a, b = ctx.atlas(), ctx.bake()
    n = size * size
    ctx.sync()
    d_tris = _hiprt.DeviceBuffer.of(tris)

    def add():
        a.begin(size, size)
        a.add_device(d_tris.ptr, len(tris), 0, SPHERE, NEAR, FAR)

    def baked():
        b.occlusion_device(a.points_device(), n, a.records_device(), 0)

    def dilated():
        a.dilate_device(a.records_device(), RINGS)

    out = {"charts": name, "triangles": len(tris), "atlas": size, "texels": n, "repeats": repeats}
    try:
        add()
        ctx.sync()      # the arrays are allocated, first launches are done
        if only_add:
            out["add"] = stats(series(ctx, [add], repeats)[0])
            return out
        baked(), dilated()
        ctx.sync()      # the table is placed, the scratch is allocated
        added, bakes, dilations = series(ctx, [add, baked, dilated], repeats)
        samples = a.read(points=False)[1]
        ring = a.read_records(bake.texel_dtype)[1]
        out.update(covered=int((samples["triangle"] != atlas.NONE).sum()), filled=int(((ring != 0) & (ring != atlas.NONE)).sum()), K=K, sets=SETS, rings=RINGS,
                   add=stats(added), bake=stats(bakes), dilate=stats(dilations))
        out["add_and_dilate_over_bake"] = (out["add"]["median_ms"] + out["dilate"]["median_ms"]) / out["bake"]["median_ms"]
        if host:
            import atlas_reference as AR
            ctx.sync()
            t0 = time.perf_counter()
            owner, want_samples, want_points = AR.build([(AR.placement_of(flat.instances[SPHERE]), tris)], size, size, NEAR, FAR)
            t1 = time.perf_counter()
            d_points = _hiprt.DeviceBuffer.of(want_points)
            t2 = time.perf_counter()
            points, samples = a.read()
            d_points.free()
            out["host"] = {"numpy_ms": (t1 - t0) * 1.0e3, "upload_ms": (t2 - t1) * 1.0e3, "points_equal": points.tobytes() == want_points.tobytes(),
                           "samples_equal": samples.tobytes() == want_samples.tobytes()}
        return out
    finally:
        d_tris.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[1024, 4096])
    ap.add_argument("--resolutions", nargs="+", type=int, default=[16, 320], help="generate_sphere resolutions: r*r - 2r triangles")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--only-add", action="store_true")
    ap.add_argument("--host", action="store_true", help="also the numpy path, for atlases of at most 1024^2")
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = world()
    flat, cam = flatten(w), camera_struct(w.camera)
    ctx = Context(0)
    ctx.set_tree(3)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.bake().set_directions((K, SETS))
    lines = []
    for r in args.resolutions:
        tris = atlas.charts(generate_sphere(r))
        for size in args.sizes:
            result = measure(ctx, flat, f"sphere {r}", tris, size, args.repeats, args.only_add, args.host and size <= 1024)
            result["label"], result["library"] = args.label, os.path.relpath(atlas.LIB_PATH, ROOT)
            lines.append(json.dumps(result))
            print(lines[-1], flush=True)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
