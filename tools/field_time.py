#!/usr/bin/env python3
"""Device time of probe fields (include/hiprz_field.h) beside what the project already had for the same work.

The bake: hiprz_field_visibility beside hiprz_probe_samples over the SAME probes, direction table and seed — the same rays walked by the
same closest-hit walk, the baseline storing 16 bytes per ray, the bake running its 64 x K multiply-adds per probe and storing 528 bytes.
The lookup: hiprz_field_lookup, with and without visibility records, in points per second, beside probe.Field.irradiance in numpy on the
host for the same points, and as a share of the device's copy rate (a device-to-device hipMemcpyAsync of 256 MiB, bytes read plus bytes
written): the lookup moves at least 48 bytes per point, 32 in and 16 out.  With --other PATH a second build of libhiprz_field.so
(make FIELD_DEFS=-DRZ_FIELD_LOOKUP_WG=256, the lookup's other workgroup size) is timed in the same rounds.  Medians of `--repeats`, HIP
events on the context's stream, the sides timed alternately on one context in one process.

    python tools/field_time.py --configs E --other /tmp/libhiprz_field_wg256.so --out profiles/r32/field_time.json

Per config: 4 096 probes, a 16^3 grid over the box of the camera's first hits (the bake also over 32^3 = 32 768 probes of the same box), near_ 1e-3, far_ 1e3; the sphere table with K = 256, S = 4;
reach three grid steps; 2^20 points drawn from the box with random unit normals; records from Context.bake_probes over a source in which
every texel has a value.  A figure is kept only when the records of the first 256 probes are the restatement's (tests/field_reference.py)
over Context.bake_rays and Context.trace in every byte, the results of the first 4 096 points are the restatement's in every byte, and
both builds agree in every byte."""
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
import bake_reference as BR  # noqa: E402
import field_reference as FR  # noqa: E402  (the gate)
from gather_time import SIZE, atlas_parts, lit_world, series, stats, surface_points  # noqa: E402
from rayzath_amd import _hiprt, _satellite, bake, field, gather, probe  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing  # noqa: E402
from rayzath_amd import scenes  # noqa: E402
from rayzath_amd.scene import camera_struct, flatten  # noqa: E402

K, SETS = 256, 4
GRID = (16, 16, 16)
LARGE_GRID = (32, 32, 32)
POINTS = 1 << 20
GATE_PROBES, GATE_POINTS = 256, 4096
COPY_BYTES = 256 << 20


class OtherFielder(field.Fielder):
    """a field.Fielder on another build of the library"""

    def __init__(self, ctx_ptr, path):
        self.K = self.S = 0
        self.table = None
        _satellite.Handle.__init__(self, _satellite.load(path, field.ENTRY_POINTS), "field", ctx_ptr)
        out = (C.c_uint32 * 8)()
        self.lib.hiprz_field_layout(out)
        self.workgroup = int(out[7])


def copy_rate(ctx, repeats):
    """GB/s (read + written) of a device-to-device copy of COPY_BYTES on the context's stream"""
    rt = _hiprt.runtime()
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    a, b = _hiprt.DeviceBuffer(COPY_BYTES), _hiprt.DeviceBuffer(COPY_BYTES)
    fn = lambda: _hiprt._check(rt.hipMemcpyAsync(b.ptr, a.ptr, COPY_BYTES, 3, ctx.stream()), "hipMemcpyAsync")
    fn()
    ctx.sync()
    st = stats(series(ctx, [fn], repeats)[0])
    ctx.sync()
    a.free(), b.free()
    return {"bytes": COPY_BYTES, **st, "GBps": 2.0 * COPY_BYTES / (st["median_ms"] * 1.0e-3) / 1.0e9}


def bake_row(ctx, sides, prober, table, probes, d_probes, d_vis, reach, repeats):
    """every side's hiprz_field_visibility of the device probes beside hiprz_probe_samples, gated on the restatement"""
    names, n = list(sides), len(probes)
    d_samples = _hiprt.DeviceBuffer(n * K * 16)
    fns = [lambda f=sides[name], name=name: f.visibility_device(d_probes.ptr, n, d_vis[name].ptr, 0, reach) for name in names]
    fns.append(lambda: prober.samples_device(d_probes.ptr, n, d_samples.ptr, 0))
    for fn in fns:
        fn()
    ctx.sync()   # the tables are placed, first launches are done
    timed = series(ctx, fns, repeats)
    ctx.sync()
    vis = {name: d_vis[name].download((n,), field.vis_dtype) for name in names}
    sub = probes[:GATE_PROBES]
    rays = ctx.bake_rays(sub, 0, table)
    assert rays.tobytes() == BR.rays(sub, table, 0).tobytes()
    assert vis["shipped"][:GATE_PROBES].tobytes() == FR.visibility_records(sub, rays, ctx.trace(rays), reach).tobytes(), "the records are not the restatement's"
    for name in names[1:]:
        assert vis[name].tobytes() == vis["shipped"].tobytes(), "the two builds differ in some byte"
    st = {name: stats(ms) for name, ms in zip(names + ["probe_samples"], timed)}
    words = vis["shipped"]["words"]
    d_samples.free()
    return {"probes": n, "rays": n * K, "front": int(words[:, 0].sum()), "back": int(words[:, 1].sum()), "missed": int(words[:, 2].sum()), **st,
            **{name + "_over_probe_samples": st[name]["median_ms"] / st["probe_samples"]["median_ms"] for name in names}}


def measure(config, repeats, tree, other_path):
    world = lit_world(config)
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx = Context(0)
    ctx.set_tree(tree)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(scenes.CONFIGS[config]["max_depth"], 8)).struct())
    seen = surface_points(ctx, 1 << 14)["position"]
    lo, hi = seen.min(0), seen.max(0)
    lo, hi = lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo)
    probes = probe.grid(lo, hi, GRID, (0.0, 1.0, 0.0), 1e-3, 1e3)
    grid = field.grid_of(lo, hi, GRID)
    flat_probes = probes.reshape(-1)
    n = len(flat_probes)
    reach = float(3.0 * grid["step"].max())
    rng = np.random.default_rng(32)
    table = probe.sphere_directions(K, SETS)
    charts = gather.chart_tables(atlas_parts(world), len(flat.instances))
    source = gather.records(rng.uniform(0.0, 4.0, (SIZE, SIZE, 3)), (SIZE, SIZE))
    sh = ctx.bake_probes(probes, source, SIZE, SIZE, charts, (64, SETS), (16, SETS), 0, (0.1, 0.2, 0.4)).reshape(-1)
    sides = {"shipped": ctx.fielder()}
    sides["shipped"].workgroup = field.layout()[7]
    if other_path:
        sides["other"] = OtherFielder(ctx._ctx, other_path)
    names = list(sides)
    p = ctx.prober()
    p.set_directions(table)
    for f in sides.values():
        f.set_directions(table)
    out = {"config": config, "probes": n, "grid": list(GRID), "box": [lo.tolist(), hi.tolist()], "K": K, "sets": SETS, "reach": reach, "instances": len(flat.instances),
           "tree": ctx.tree(), "repeats": repeats, "other": other_path, "workgroups": {name: sides[name].workgroup for name in names}}

    # --- the bake beside hiprz_probe_samples: the field's own grid, and LARGE_GRID probes over the same box (a wave per probe: 4 096 probes
    # are 4 096 waves, fewer than the device holds at once, where the baseline's thread per ray makes K / 64 times as many) ---
    d_probes = _hiprt.DeviceBuffer.of(flat_probes)
    d_vis = {name: _hiprt.DeviceBuffer(n * field.vis_dtype.itemsize) for name in names}
    out["bake"] = bake_row(ctx, sides, p, table, flat_probes, d_probes, d_vis, reach, repeats)
    vis = {name: d_vis[name].download((n,), field.vis_dtype) for name in names}
    large = probe.grid(lo, hi, LARGE_GRID, (0.0, 1.0, 0.0), 1e-3, 1e3).reshape(-1)
    d_large = _hiprt.DeviceBuffer.of(large)
    d_large_vis = {name: _hiprt.DeviceBuffer(len(large) * field.vis_dtype.itemsize) for name in names}
    out["bake_large"] = {"grid": list(LARGE_GRID), **bake_row(ctx, sides, p, table, large, d_large, d_large_vis, reach, repeats)}
    for b in [d_large, *d_large_vis.values()]:
        b.free()

    # --- the lookup ---
    points = bake.points(rng.uniform(lo, hi, (POINTS, 3)), BR.normalized(rng.normal(size=(POINTS, 3))))
    params = field.params(bias=0.25 * float(grid["step"].min()), max_back=K // 4)
    d_sh, d_points = _hiprt.DeviceBuffer.of(sh), _hiprt.DeviceBuffer.of(points)
    d_out = {(name, v): _hiprt.DeviceBuffer(POINTS * 16) for name in names for v in (False, True)}
    keys = list(d_out)
    fns = [lambda f=sides[name], name=name, v=v: f.lookup_device(grid, d_probes.ptr, d_sh.ptr, d_vis[name].ptr if v else None, n, d_points.ptr, POINTS, d_out[(name, v)].ptr, params)
           for name, v in keys]
    for fn in fns:
        fn()
    ctx.sync()
    timed = series(ctx, fns, repeats)
    ctx.sync()
    results = {key: d_out[key].download((POINTS,), field.result_dtype) for key in keys}
    for v in (False, True):
        want = FR.lookup(grid, flat_probes, sh, vis["shipped"] if v else None, params, points[:GATE_POINTS])
        assert results[("shipped", v)][:GATE_POINTS].tobytes() == want.tobytes(), "the results are not the restatement's"
        for name in names[1:]:
            assert results[(name, v)].tobytes() == results[("shipped", v)].tobytes(), "the two builds differ in some byte"
    copy = copy_rate(ctx, repeats)
    t0 = time.perf_counter()
    host = probe.Field(lo, hi, GRID, sh).irradiance(points["position"], points["normal"])
    host_ms = (time.perf_counter() - t0) * 1.0e3
    good = results[("shipped", False)]["word"] != field.INVALID
    seen_by = results[("shipped", True)]["word"]
    worst = float(np.abs(results[("shipped", False)]["rgb"][good] - host[good]).max() / np.abs(host[good]).max())
    rows = {}
    for (name, v), ms in zip(keys, timed):
        s = stats(ms)
        rate = POINTS / (s["median_ms"] * 1.0e-3)
        rows[f"{name}_{'visibility' if v else 'plain'}"] = {**s, "points_per_second": rate, "GBps_at_48_bytes_per_point": rate * 48.0 / 1.0e9,
                                                           "share_of_copy_rate": rate * 48.0 / 1.0e9 / copy["GBps"]}
    out["lookup"] = {"points": POINTS, "bias": float(params["bias"]), "max_back": int(params["max_back"]), "copy": copy, **rows,
                     "numpy_field_irradiance_ms": host_ms, "numpy_points_per_second": POINTS / (host_ms * 1.0e-3), "plain_against_numpy_worst_relative_to_largest": worst,
                     "points_without_a_value_with_visibility": int((seen_by == field.INVALID).sum()), "counted_mean_with_visibility": float(seen_by[seen_by != field.INVALID].mean())}
    for b in [d_probes, d_sh, d_points, *d_vis.values(), *d_out.values()]:
        b.free()
    for name in names[1:]:
        sides[name].close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["E"])
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--tree", type=int, default=3, help="hiprz_set_tree (3 = TREE_DEVICE_SAH: device-built trees)")
    ap.add_argument("--other", default=None, help="a second build of libhiprz_field.so to time in the same rounds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for config in args.configs:
        lines.append(json.dumps(measure(config, args.repeats, args.tree, args.other)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
