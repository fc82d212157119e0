#!/usr/bin/env python3
"""Device time of lightmap smoothing (include/hiprz_smooth.h), per iteration and as a share of the bakes it follows.  Medians of
`--repeats`, HIP events on the context's stream, the sides timed alternately on one context in one process.  With --other PATH a second
build of libhiprz_smooth.so (make SMOOTH_DEFS=..., the other form of the kernel) is timed in the same rounds.

    python tools/smooth_time.py --other /tmp/libhiprz_smooth_direct.so --out profiles/r31/smooth_time.json

PER ITERATION, on a synthetic atlas of 1024^2 and 4096^2 texels (flat charts of 252 x 252 texels with gutters of 4 between them, every
second chart a wall, a penumbra-like noisy light on them, all three stops on): calls of 1, 2 and 3 iterations with an output of their own
are timed in the same rounds; the time of the iteration at s = 1 is the first call's, at s = 2 and s = 4 the difference of the medians of
consecutive calls.  `share` is the algorithmic traffic of an iteration — 48 bytes read and 16 written per texel — over the time, as a
share of the 6.29 TB/s a float4 copy reaches on the MI355X (of 8 TB/s by its specification; the 1024^2 atlas, 64 MB of traffic, lives in the
256 MB Infinity Cache and may exceed it).  A figure is kept only when both builds agree in every byte and, at 1024^2, with the numpy
restatement (tests/smooth_reference.py), whose time on the host's clock is written beside the device's.

THE WHOLE CALL, on the atlases of tools/atlas_time.py (sphere charts of 101 760 triangles at 1024^2 and 4096^2, its world with a spot and a
direct light added): three iterations at smooth.params()'s defaults beside hiprz_light_bake at K = 16 and beside one bounce — compose,
dilate, hiprz_gather_texels at K = 64 — over the same points.  `spread` is (max - min) / median of a series."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import smooth_reference as SR  # noqa: E402  (the gate)
import atlas_time  # noqa: E402
from atlas_time import series, stats  # noqa: E402
from rayzath_amd import _hiprt, _satellite, atlas, bake, gather, smooth  # noqa: E402
from rayzath_amd.engine import Context  # noqa: E402
from rayzath_amd.scene import DirectLight, SpotLight, camera_struct, flatten, generate_sphere  # noqa: E402

HBM_COPY_TBS = 6.29
BYTES_PER_TEXEL = 64
STOPS = dict(radius=0.5, plane=0.02, sigma_colour=2.0)
TILE, GUTTER = 256, 4


class OtherSmooth(smooth.Smooth):
    """a smooth.Smooth on another build of the library"""

    def __init__(self, ctx_ptr, path):
        _satellite.Handle.__init__(self, _satellite.load(path, smooth.ENTRY_POINTS), "smooth", ctx_ptr)
        out = (smooth.U32 * 8)()
        self.lib.hiprz_smooth_layout(out)
        self.forms = list(out)[6:8]


def synthetic(size, seed=31):
    """(points, records) of a size x size atlas of flat charts with gutters, texels 1 / 64 apart in the world"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(size), np.arange(size))
    covered = (x % TILE < TILE - GUTTER) & (y % TILE < TILE - GUTTER)
    wall = ((x // TILE + y // TILE) % 2 == 1)
    points, records = np.zeros((size, size), bake.point_dtype), np.zeros((size, size), SR.record_dtype)
    u, v = (x / 64.0).astype(np.float32), (y / 64.0).astype(np.float32)
    points["position"][..., 0] = np.where(wall, 0.0, u)
    points["position"][..., 1] = np.where(wall, u, 0.0)
    points["position"][..., 2] = v
    points["normal"][..., 0], points["normal"][..., 1] = wall, ~wall
    points["near"], points["far"] = 1e-3, 1e3
    for name in ("position", "normal"):
        points[name][~covered] = 0.0
    points["near"][~covered] = points["far"][~covered] = 0.0
    shade = np.clip(np.sin(u * 0.7) * np.cos(v * 0.9) + 0.5, 0.0, 1.0)
    light = np.floor(shade * 4.0 + rng.random((size, size))) / 4.0          # the K + 1 values of a K = 4 bake
    records["rgb"] = (light[..., None] * np.array([1.0, 0.9, 0.8])).astype(np.float32)
    records["word"] = np.where(covered, rng.integers(0, 5, (size, size)), SR.INVALID)
    records["rgb"][~covered] = 0.0
    return points, records


def per_iteration(ctx, sides, size, repeats, gate):
    points, records = synthetic(size)
    n = size * size
    ctx.sync()
    d_points, d_records = _hiprt.DeviceBuffer.of(points), _hiprt.DeviceBuffer.of(records)
    d_out = {name: _hiprt.DeviceBuffer(n * 16) for name in sides}
    names, its = list(sides), (1, 2, 3)
    try:
        fns = [lambda s=sides[name], o=d_out[name], it=it: s.texels_device(d_points.ptr, d_records.ptr, size, size, smooth.params(it, **STOPS), o.ptr) for name in names for it in its]
        for fn in fns:
            fn()
        ctx.sync()      # the scratch is allocated, first launches are done
        timed = series(ctx, fns, repeats)
        ctx.sync()
        got = {name: d_out[name].download((size, size), SR.record_dtype) for name in names}       # the three-iteration call ran last
        for name in names[1:]:
            assert got[name].tobytes() == got[names[0]].tobytes(), "the two builds differ in some byte"
        out = {"atlas": size, "texels": n, "covered": int(SR.takes_part(points, records).sum()), "repeats": repeats, "stops": STOPS, "bytes_per_texel": BYTES_PER_TEXEL, "sides": {}}
        if gate:
            t0 = time.perf_counter()
            want = SR.smooth(points, records, iterations=3, **STOPS)
            out["numpy_ms"] = (time.perf_counter() - t0) * 1.0e3
            assert got[names[0]].tobytes() == want.tobytes(), "the device's records are not the restatement's"
            out["changed_texels"] = int((want["rgb"] != records["rgb"]).any(-1).sum())
        for k, name in enumerate(names):
            calls = [stats(timed[k * len(its) + j]) for j in range(len(its))]
            side = {"forms_s1_sN": sides[name].forms, "calls": {str(it): c for it, c in zip(its, calls)}, "iterations": {}}
            before = 0.0
            for it, c in zip(its, calls):
                ms = c["median_ms"] - before
                before = c["median_ms"]
                tbs = BYTES_PER_TEXEL * n / (ms * 1.0e-3) / 1.0e12
                side["iterations"][f"s={1 << (it - 1)}"] = {"ms": ms, "TB_per_s": tbs, "share_of_hbm_copy": tbs / HBM_COPY_TBS}
            out["sides"][name] = side
        if gate:
            out["numpy_over_device"] = out["numpy_ms"] / out["sides"][names[0]]["calls"]["3"]["median_ms"]
        return out
    finally:
        for b in [d_points, d_records, *d_out.values()]:
            b.free()


def whole_call(ctx, flat, tris, size, repeats):
    a, lt, g, s = ctx.atlas(), ctx.light(), ctx.gatherer(), ctx.smoother()
    n = size * size
    lt.set_samples((16, 4)), g.set_directions((64, 4)), g.set_charts(*gather.chart_tables([(atlas_time.SPHERE, tris)], len(flat.instances)))
    a.begin(size, size)
    a.add(tris, 0, atlas_time.SPHERE, atlas_time.NEAR, atlas_time.FAR)
    ctx.sync()
    albedo = _hiprt.DeviceBuffer.of(gather.records((0.7, 0.6, 0.5), (size, size)))
    direct, indirect, source = (_hiprt.DeviceBuffer(n * 16) for _ in range(3))
    points, params = a.points_device(), smooth.params()

    def lit():
        lt.bake_device(points, n, direct.ptr, 0, None)

    def bounce():
        g.compose_device(direct.ptr, None, albedo.ptr, None, source.ptr, n)
        a.dilate_device(source.ptr, atlas_time.RINGS)
        g.texels_device(points, n, source.ptr, size, size, indirect.ptr, 0, (0.0, 0.0, 0.0))

    def smoothed():
        s.texels_device(points, indirect.ptr, size, size, params)

    try:
        lit(), bounce(), smoothed()
        ctx.sync()
        timed = [stats(ms) for ms in series(ctx, [lit, bounce, smoothed], repeats)]
        ctx.sync()
        out = {"charts": "sphere 320", "triangles": len(tris), "atlas": size, "texels": n, "repeats": repeats, "light_K": 16, "gather_K": 64,
               "params": {k: params[k].item() for k in smooth.params_dtype.names}, "light_bake": timed[0], "one_bounce": timed[1], "smooth": timed[2]}
        out["smooth_over_light_bake"] = timed[2]["median_ms"] / timed[0]["median_ms"]
        out["smooth_over_one_bounce"] = timed[2]["median_ms"] / timed[1]["median_ms"]
        return out
    finally:
        for b in (albedo, direct, indirect, source):
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[1024, 4096])
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--other", default=None, help="a second build of libhiprz_smooth.so to time in the same rounds")
    ap.add_argument("--no-gate", action="store_true", help="skip the numpy restatement at 1024^2 (half a minute on the host)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = atlas_time.world()
    w.add(SpotLight(position=(1.5, 4.0, -1.0), direction=(-0.3, -1.0, 0.25), color=(255, 240, 220, 255), size=0.35, emission=60.0, beam_angle=0.8))
    w.add(DirectLight(direction=(-0.25, -1.0, 0.45), color=(255, 255, 240, 255), emission=4.0, angular_size=0.15))
    flat, cam = flatten(w), camera_struct(w.camera)
    ctx = Context(0)
    ctx.set_tree(3)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    sides = {"shipped": ctx.smoother()}
    sides["shipped"].forms = smooth.layout()[6:8]
    if args.other:
        sides["other"] = OtherSmooth(ctx._ctx, args.other)
    lines = []
    for size in args.sizes:
        lines.append(json.dumps({"per_iteration": per_iteration(ctx, sides, size, args.repeats, size <= 1024 and not args.no_gate)}))
        print(lines[-1], flush=True)
    tris = atlas.charts(generate_sphere(320))
    for size in args.sizes:
        lines.append(json.dumps({"whole_call": whole_call(ctx, flat, tris, size, args.repeats)}))
        print(lines[-1], flush=True)
    if args.other:
        sides["other"].close()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
