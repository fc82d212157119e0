#!/usr/bin/env python3
"""Device time of the baked view (include/hiprz_view.h) beside the best route there was before it: hiprz_query_closest over the SAME pixel
rays, already on the device as hiprz_query_pixel_rays writes them — no host copy, no chart lookup, no field and no shading, all of which
favours the query.  The baseline is never the view itself.  Medians of `--repeats`, HIP events on the context's stream, the sides timed
alternately on one context in one process.  With --other PATH a second build of libhiprz_view.so (make VIEW_DEFS=-DRZ_VIEW_ROWS, thread i
is pixel i; or -DRZ_VIEW_WAVES=4) is timed in the same rounds.

    python tools/view_time.py --configs D E --other /tmp/libhiprz_view_rows.so --out profiles/r34/view_time.json

Per config: the config's camera at 1920 x 1080; a 1024 x 1024 source in which every texel has a value; a chart map that covers EVERY
instance — one cell of a square grid per instance, one chart per mesh triangle with its UVs drawn inside the cell, so that neighbouring hits
on a triangle read neighbouring texels — viewed with the nearest and the bilinear filter (`atlas`); the same map with every fourth instance
taken out of it and a 16^3 field over the box of the camera's first hits — random records, the device's own visibility records (`mixed`).
`spread` is (max - min) / median of a series.  The bar: the atlas-only view is no slower than the query by more than three times the larger
of the two spreads; the ratio and the spreads are written down whichever way they fall.  A figure is kept only when the emitted samples
agree with the query's hits on every pixel (t in every byte, the ids tests/gather_reference.py derives from the hits), the timed view's
records are the restatement's (tests/view_reference.py) on every 97th pixel in every byte, and both builds agree in every byte.  Also, on
the host's clock, the numpy route for one frame: Context.pixel_rays, Context.trace, the chart lookup in numpy and Context.lookup_field for
the unmapped hits (no tone map) — the chart lookup as a cost proxy with bx = by = 0, since the hit record holds no barycentrics.

--end-to-end: the ratio of the mean luminance over ATLAS pixels between the baked view of Context.bake_bounce_atlas with 1, 2 and 3 bounces
and a path-traced frame of the same diffuse world (tests/gather_world.py's, 256 x 192) from Context.read_accum, with Context.noise's rms
beside it.  Reported without a bar."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gather_reference as GR  # noqa: E402  (the gate)
import view_reference as VR  # noqa: E402  (the gate)
from gather_time import lit_world, series, stats  # noqa: E402
from rayzath_amd import _hiprt, _satellite, bake, field, gather, probe, query, scenes, view  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing  # noqa: E402
from rayzath_amd.scene import camera_struct, flatten  # noqa: E402

SIZE = 1024
GRID = (16, 16, 16)
WIDTH, HEIGHT = 1920, 1080
GATE_STEP = 97
SKY = (0.1, 0.2, 0.4)


class OtherView(view.View):
    """a view.View on another build of the library"""

    def __init__(self, ctx_ptr, path):
        _satellite.Handle.__init__(self, _satellite.load(path, view.ENTRY_POINTS), "view", ctx_ptr)
        out = (C.c_uint32 * 8)()
        self.lib.hiprz_view_layout(out)
        self.rows = int(out[7])


def cell_chart_map(world, rng):
    """every instance mapped: a cell of a square grid per instance, one chart per mesh triangle, its UVs drawn inside the cell"""
    counts = [len(inst.mesh.tri_vertices) for inst in world.instances]
    side = int(np.ceil(np.sqrt(max(len(counts), 1))))
    base = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32)
    uv = np.zeros(int(sum(counts)), gather.chart_dtype)
    cell = np.repeat(np.arange(len(counts)), counts)
    for name in ("u1", "v1", "u2", "v2", "u3", "v3"):
        at = cell % side if name[0] == "u" else cell // side
        uv[name] = (at + 0.02 + 0.96 * rng.random(len(uv))) / side
    return base, uv


def measure(config, repeats, tree, other_path):
    world = lit_world(config)
    world.camera.width, world.camera.height = WIDTH, HEIGHT
    flat, cam = flatten(world), camera_struct(world.camera)
    assert (cam.width, cam.height) == (WIDTH, HEIGHT)
    ctx = Context(0)
    ctx.set_tree(tree)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(scenes.CONFIGS[config]["max_depth"], 8)).struct())
    n = WIDTH * HEIGHT
    rng = np.random.default_rng(34)
    base, uv = cell_chart_map(world, rng)
    partial = base.copy()
    partial[3::4] = gather.NONE
    source = gather.records(rng.uniform(0.0, 4.0, (SIZE, SIZE, 3)), (SIZE, SIZE))
    sides = {"shipped": ctx.viewer()}
    sides["shipped"].rows = view.layout()[7]
    if other_path:
        sides["other"] = OtherView(ctx._ctx, other_path)
    names = list(sides)
    q = ctx.query()
    d_rays, d_hits, d_source, d_samples = _hiprt.DeviceBuffer(n * 32), _hiprt.DeviceBuffer(n * 48), _hiprt.DeviceBuffer.of(source), _hiprt.DeviceBuffer(n * 16)
    q.pixel_rays_device(d_rays.ptr)
    q.closest_device(d_rays.ptr, n, d_hits.ptr)
    ctx.sync()
    rays, hits = d_rays.download((HEIGHT, WIDTH), query.ray_dtype), d_hits.download((HEIGHT, WIDTH), query.hit_dtype)
    found = (hits["flags"] & query.HIT_FOUND) != 0
    # the field: over the box of the first hits
    seen = (rays["origin"] + hits["t"][..., None] * rays["direction"])[found]
    lo, hi = seen.min(0), seen.max(0)
    lo, hi = lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo)
    probes = probe.grid(lo, hi, GRID, (0.0, 1.0, 0.0), 1e-3, 1e3).reshape(-1)
    grid = field.grid_of(lo, hi, GRID)
    sh = np.zeros(len(probes), probe.sh_dtype)
    sh["sh"][:, 0, :3] = rng.uniform(1.0, 2.0, (len(probes), 3))
    sh["sh"][:, 1:, :3] = rng.uniform(-0.3, 0.3, (len(probes), 8, 3))
    vis = ctx.bake_visibility(probes, (64, 4), 0, float(3.0 * grid["step"].max()))
    fparams = field.params(bias=0.25 * float(grid["step"].min()), max_back=16)
    d_probes, d_sh, d_vis = _hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer.of(sh), _hiprt.DeviceBuffer.of(vis)
    on_device = (grid, d_probes.ptr, d_sh.ptr, d_vis.ptr, len(probes), fparams)
    cases = {"atlas_nearest": (base, None, "nearest"), "atlas_bilinear": (base, None, "bilinear"), "mixed_bilinear": (partial, on_device, "bilinear")}
    out = {"config": config, "width": WIDTH, "height": HEIGHT, "pixels": n, "instances": len(flat.instances), "charts": len(uv), "source": [SIZE, SIZE], "grid": list(GRID),
           "tree": ctx.tree(), "repeats": repeats, "other": other_path, "rows_build": {name: sides[name].rows for name in names}, "hit_pixels": int(found.sum()), "cases": {}}
    material = flat.materials[np.where(found & (hits["material"] >= 0), hits["material"], 0)]
    color = (material["color"][..., :3].astype(np.float32) / np.float32(255.0)).astype(np.float32)
    plain_surface = (material["texture"] < 0) & (material["emission_map"] < 0) & (hits["material"] >= 0)          # the gate restates no texture fetch: those pixels are left out of it
    pick = np.zeros((HEIGHT, WIDTH), bool)
    pick.reshape(-1)[::GATE_STEP] = True
    asks = lambda: q.closest_device(d_rays.ptr, n, d_hits.ptr)
    for case, (b, f, filter) in cases.items():
        d_out = {name: _hiprt.DeviceBuffer(n * 16) for name in names}
        for v in sides.values():
            v.set_charts(b, uv)
        fns = [lambda v=sides[name], name=name: v.pixels_device(d_source.ptr, SIZE, SIZE, d_out[name].ptr, None, f, SKY, filter) for name in names]
        sides["shipped"].samples_device(d_samples.ptr)
        for fn in fns + [asks]:
            fn()
        ctx.sync()   # the chart map is placed, first launches are done
        timed = series(ctx, fns + [asks], repeats)
        ctx.sync()
        got = {name: d_out[name].download((HEIGHT, WIDTH), view.pixel_dtype) for name in names}
        samples = d_samples.download((HEIGHT, WIDTH), gather.sample_dtype)
        # the gate: no figure without it
        assert samples["t"].tobytes() == hits["t"].tobytes(), "the emitted samples' t is not the query's on the pixel rays"
        assert np.array_equal(samples["id"], GR.ids(hits["flags"], hits["instance"], hits["triangle"], b, len(uv))), "the emitted ids are not those of the query's hits"
        gate = pick & (plain_surface | (samples["id"] != gather.UNMAPPED))
        host_field = None if f is None else (grid, probes, sh, vis, fparams)
        want = VR.pixels(samples[gate], uv, source, SIZE, SIZE, SKY, view.FILTERS[filter], rays["origin"][gate], rays["direction"][gate], hits["normal"][gate], color[gate],
                         material["emission"][gate].astype(np.float32), field=host_field)
        assert got["shipped"][gate].tobytes() == want.tobytes(), f"{case}: the timed view is not the restatement's on the subsample"
        for name in names[1:]:
            assert got[name].tobytes() == got["shipped"].tobytes(), f"{case}: the two builds differ in some byte"
        st = {name: stats(ms) for name, ms in zip(names + ["query_closest"], timed)}
        row = {"gate_pixels": int(gate.sum()), "kinds": np.bincount(view.kind(got["shipped"]).reshape(-1), minlength=5).tolist(), **st}
        for name in names:
            allowed = 3.0 * max(st[name]["spread"], st["query_closest"]["spread"])
            row[name + "_over_query"] = st[name]["median_ms"] / st["query_closest"]["median_ms"]
            row[name + "_bar_allowed_excess"] = allowed
            row[name + "_bar_met"] = st[name]["median_ms"] <= st["query_closest"]["median_ms"] * (1.0 + allowed)
        out["cases"][case] = row
        for d in d_out.values():
            d.free()
    # the numpy route for one frame, on the host's clock: what a caller did before this library
    t0 = time.perf_counter()
    r = ctx.pixel_rays()
    t1 = time.perf_counter()
    h = ctx.trace(r)
    t2 = time.perf_counter()
    ids = GR.ids(h["flags"], h["instance"], h["triangle"], partial, len(uv))
    s = GR.make_samples(ids, h["u"] * 0, h["v"] * 0, h["t"])          # (the hit record holds texture coordinates, not barycentrics: the lookup's cost is what is timed)
    u, v, mapped = GR.uv(s, uv)
    x, y, _ = GR.texel_of(u, v, SIZE, SIZE)
    looked = source.reshape(-1)[y * SIZE + x]
    t3 = time.perf_counter()
    unmapped = ids == gather.UNMAPPED
    pts = bake.points((r["origin"] + h["t"][..., None] * r["direction"])[unmapped], h["normal"][unmapped])
    ctx.lookup_field(grid, probes, sh, pts, vis, fparams)
    t4 = time.perf_counter()
    out["numpy_route_host_clock_ms"] = {"pixel_rays": (t1 - t0) * 1e3, "trace": (t2 - t1) * 1e3, "chart_lookup_numpy": (t3 - t2) * 1e3, "lookup_field": (t4 - t3) * 1e3,
                                        "total": (t4 - t0) * 1e3, "unmapped_pixels": int(unmapped.sum()), "texels_read": int(looked.size)}
    for d in (d_rays, d_hits, d_source, d_samples, d_probes, d_sh, d_vis):
        d.free()
    for name in names[1:]:
        sides[name].close()
    ctx.close()
    return out


def end_to_end(passes, tree):
    """the mean luminance of the baked view over its ATLAS pixels against a path-traced frame of the same diffuse world"""
    import gather_world as GW
    from rayzath_amd.scene import Camera
    world = GW.world()
    world.camera = Camera(position=(0.5, 3.5, -6.0), resolution=(256, 192), fov=1.0, near_far=(1e-2, 1e3))
    world.camera.look_at((0.0, 0.5, 0.0))
    flat, cam = flatten(world), camera_struct(world.camera)
    parts = GW.parts(world)
    albedo = tuple(np.float32(c) / np.float32(255.0) for c in (200, 200, 200))
    luminance = lambda rgb: 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]
    rows = []
    for bounces in (1, 2, 3):
        ctx = Context(0)
        ctx.set_tree(tree)
        ctx.upload_scene(flat), ctx.upload_camera(cam)
        direct, indirect, ring = ctx.bake_bounce_atlas(parts, 256, 192, albedo, None, bounces, (256, 4), (16, 4), 0, 2, (0.0, 0.0, 0.0), 1e-3, 1e3)
        source = ctx.lit_source(direct, indirect, albedo, None, 2)
        charts = gather.chart_tables(parts, len(flat.instances))
        baked = ctx.view(source, 256, 192, charts, None, (0.0, 0.0, 0.0), "bilinear")
        lit = view.kind(baked) == view.ATLAS
        ctx.set_config(RenderConfig(tracing=Tracing(16, 8)).struct())
        ctx.set_variance(1)
        for _ in range(passes // 8):
            ctx.render(8)
        accum = ctx.read_accum()
        traced = accum[..., :3] / np.maximum(accum[..., 3:4], 1.0)
        summary, _ = ctx.noise()
        rows.append({"bounces": bounces, "atlas_pixels": int(lit.sum()), "baked_mean_luminance": float(luminance(baked["rgb"])[lit].mean()),
                     "traced_mean_luminance": float(luminance(traced)[lit].mean()), "ratio": float(luminance(baked["rgb"])[lit].mean() / luminance(traced)[lit].mean()),
                     "passes": int(ctx.pass_count()), "max_depth": 16, "noise_rms": float(summary.rms), "noise_tile_rms_max": float(summary.tile_rms_max)})
        ctx.close()
    return {"end_to_end": rows, "world": "tests/gather_world.py", "camera": [256, 192], "atlas": [256, 192], "K": 256, "light_K": 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["D", "E"])
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--tree", type=int, default=3, help="hiprz_set_tree (3 = TREE_DEVICE_SAH: device-built trees)")
    ap.add_argument("--other", default=None, help="a second build of libhiprz_view.so to time in the same rounds")
    ap.add_argument("--end-to-end", type=int, default=0, metavar="PASSES", help="also the end-to-end figure, the path-traced frame of PASSES passes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for config in args.configs:
        lines.append(json.dumps(measure(config, args.repeats, args.tree, args.other)))
        print(lines[-1], flush=True)
    if args.end_to_end:
        lines.append(json.dumps(end_to_end(args.end_to_end, args.tree)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
