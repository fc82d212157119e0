#!/usr/bin/env python3
"""Device time of probe baking (include/hiprz_probe.h) beside the parent's kernels on the same work: hiprz_gather_texels over the SAME points,
direction table, chart map and source for the gathered term (3 running sums per lane and one 16-byte store against 27 and nine), and
hiprz_light_bake over the same points and samples for the light term.  The baselines are never the code under test.  With --other PATH a
second build of libhiprz_probe.so (make PROBE_DEFS=..., the running sums held the other way) is timed in the same rounds.  Medians of
`--repeats`, HIP events on the context's stream, the sides timed alternately on one context in one process.

    python tools/probe_time.py --configs E D --other /tmp/libhiprz_probe_registers.so --out profiles/r30/probe_time.json

Per config: n = 32 768 probes, a 32^3 grid over the box of the camera's first hits, near_ 1e-3, far_ 1e3; the sphere table with S = 4, K in
64, 256; the light's disk table with K = 16; the `atlas` chart map of tools/gather_time.py over a 1024 x 1024 source in which every texel has
a value.  `spread` is (max - min) / median of a series.  The bar: a probe kernel is no slower than its baseline by more than three times the
larger of the two spreads; the ratio and the spreads are written down whichever way they fall.  A figure is kept only when the probe
samples are hiprz_gather_samples' in every byte and the records of the first 2 048 probes are the restatement's (tests/probe_reference.py)
over those samples and over Context.occluded's verdicts, in every byte, and when both builds agree in every byte.  Also, on the host's clock
for the configs of --field-configs: Context.bake_probe_field beside Context.bake_bounce_atlas at 1024 x 1024."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bake_reference as BR  # noqa: E402
import light_reference as LR  # noqa: E402
import probe_reference as PR  # noqa: E402  (the gate)
from gather_time import SIZE, atlas_parts, lit_world, series, stats, surface_points  # noqa: E402
from rayzath_amd import _hiprt, _satellite, gather, light, probe  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing  # noqa: E402
from rayzath_amd import scenes  # noqa: E402
from rayzath_amd.scene import camera_struct, flatten  # noqa: E402

KS = (64, 256)
LIGHT_K = 16
SETS = 4
GRID = (32, 32, 32)
GATE = 2048
SKY = (0.1, 0.2, 0.4)


class OtherProbe(probe.Probe):
    """a probe.Probe on another build of the library"""

    def __init__(self, ctx_ptr, path):
        self.K = self.S = self.LK = self.LS = 0
        self.table = self.disk = None
        _satellite.Handle.__init__(self, _satellite.load(path, probe.ENTRY_POINTS), "probe", ctx_ptr)


def bar(side, baseline):
    allowed = 3.0 * max(side["spread"], baseline["spread"])
    return {"ratio": side["median_ms"] / baseline["median_ms"], "bar_allowed_excess": allowed, "bar_met": side["median_ms"] <= baseline["median_ms"] * (1.0 + allowed)}


def measure(config, repeats, tree, other_path):
    world = lit_world(config)
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx = Context(0)
    ctx.set_tree(tree)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(scenes.CONFIGS[config]["max_depth"], 8)).struct())
    seen = surface_points(ctx, 1 << 14)["position"]
    lo, hi = seen.min(0), seen.max(0)
    probes = probe.grid(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), GRID, (0.0, 1.0, 0.0), 1e-3, 1e3).reshape(-1)
    n = len(probes)
    rng = np.random.default_rng(30)
    base, uv = gather.chart_tables(atlas_parts(world), len(flat.instances))
    source = gather.records(rng.uniform(0.0, 4.0, (SIZE, SIZE, 3)), (SIZE, SIZE))
    g, lt = ctx.gatherer(), ctx.light()
    sides = {"shipped": ctx.prober()}
    if other_path:
        sides["other"] = OtherProbe(ctx._ctx, other_path)
    g.set_charts(base, uv)
    disk = light.disk_samples(LIGHT_K, SETS)
    lt.set_samples(disk)
    for p in sides.values():
        p.set_charts(base, uv), p.set_samples(disk)
    d_probes, d_source, d_texels = _hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer.of(source), _hiprt.DeviceBuffer(n * 16)
    d_sh = {name: _hiprt.DeviceBuffer(n * 144) for name in sides}
    out = {"config": config, "probes": n, "grid": list(GRID), "box": [lo.tolist(), hi.tolist()], "instances": len(flat.instances), "charts": len(uv), "source": [SIZE, SIZE],
           "sets": SETS, "tree": ctx.tree(), "repeats": repeats, "lights": [len(flat.spot_lights), len(flat.direct_lights)], "other": other_path, "gather": [], "light": None}
    names = list(sides)
    ce = LR.colour_emission(flat.spot_lights, flat.direct_lights)
    for K in KS:
        table = probe.sphere_directions(K, SETS)
        g.set_directions(table)
        for p in sides.values():
            p.set_directions(table)
        fns = [lambda p=sides[name], name=name: p.gather_device(d_probes.ptr, n, d_source.ptr, SIZE, SIZE, d_sh[name].ptr, 0, SKY) for name in names]
        fns.append(lambda: g.texels_device(d_probes.ptr, n, d_source.ptr, SIZE, SIZE, d_texels.ptr, 0, SKY))
        for fn in fns:
            fn()
        ctx.sync()   # the tables are placed, first launches are done
        timed = series(ctx, fns, repeats)
        ctx.sync()
        # the gate: no figure without it
        records = {name: d_sh[name].download((n,), probe.sh_dtype) for name in names}
        texels = d_texels.download((n,), gather.texel_dtype)
        sub = probes[:GATE]
        samples = sides["shipped"].samples(sub, 0, ctx.sync)
        assert samples.tobytes() == g.samples(sub, 0, ctx.sync).tobytes(), "the probe samples are not hiprz_gather_samples'"
        want = PR.gather_records(sub, samples, BR.rays(sub, table, 0), uv, source, SIZE, SIZE, SKY)
        assert records["shipped"][:GATE].tobytes() == want.tobytes(), "the records are not the restatement's over the samples"
        assert records["shipped"]["sh"][:, 0, :3].tobytes() == texels["mean"].tobytes() and np.array_equal(probe.words(records["shipped"])[0], texels["counts"]), "B0 = 1: the gather's own texel"
        for name in names[1:]:
            assert records[name].tobytes() == records["shipped"].tobytes(), "the two builds differ in some byte"
        st = {name: stats(ms) for name, ms in zip(names + ["gather_texels"], timed)}
        counts = probe.words(records["shipped"])[0]
        row = {"K": K, "rays": n * K, "read": int((counts & 0xFFFF).sum()), "missed": int((counts >> 16).sum()), **st}
        for name in names:
            row[name + "_over_gather_texels"] = bar(st[name], st["gather_texels"])
        out["gather"].append(row)
    # the light term
    fns = [lambda p=sides[name], name=name: p.light_device(d_probes.ptr, n, d_sh[name].ptr, 0, None, None) for name in names]
    fns.append(lambda: lt.bake_device(d_probes.ptr, n, d_texels.ptr, 0, None))
    for fn in fns:
        fn()
    ctx.sync()
    timed = series(ctx, fns, repeats)
    ctx.sync()
    records = {name: d_sh[name].download((n,), probe.sh_dtype) for name in names}
    sub = probes[:GATE]
    rays, weights = PR.light_rays(sub, flat.spot_lights, flat.direct_lights, disk, 0)
    verdicts = ctx.occluded(rays.reshape(-1)).reshape(rays.shape)
    assert records["shipped"][:GATE].tobytes() == PR.light_records(sub, rays["direction"], weights, verdicts, ce).tobytes(), "the light records are not the restatement's"
    for name in names[1:]:
        assert records[name].tobytes() == records["shipped"].tobytes(), "the two builds differ in some byte"
    st = {name: stats(ms) for name, ms in zip(names + ["light_bake"], timed)}
    row = {"K": LIGHT_K, "rays": n * LIGHT_K * len(ce), "shadowed": int(probe.words(records["shipped"])[1].sum()), **st}
    for name in names:
        row[name + "_over_light_bake"] = bar(st[name], st["light_bake"])
    out["light"] = row
    for b in [d_probes, d_source, d_texels, *d_sh.values()]:
        b.free()
    for name in names[1:]:
        sides[name].close()
    ctx.close()
    return out


def measure_field(config, tree):
    world = lit_world(config)
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx = Context(0)
    ctx.set_tree(tree)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    parts = atlas_parts(world)
    seen = surface_points(ctx, 1 << 14)["position"]
    lo, hi = seen.min(0), seen.max(0)
    probes = probe.grid(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), GRID, (0.0, 1.0, 0.0), 1e-3, 1e3)
    clock = {"bake_bounce_atlas": [], "bake_probe_field": []}
    for _ in range(3):
        ctx.sync()
        t0 = time.perf_counter()
        atlas_only = ctx.bake_bounce_atlas(parts, SIZE, SIZE, (0.8, 0.8, 0.8), None, 1, (16, SETS), (16, SETS), 0, 2, (0.0, 0.0, 0.0), 1e-3, 1e3)
        clock["bake_bounce_atlas"].append((time.perf_counter() - t0) * 1.0e3)
        ctx.sync()
        t0 = time.perf_counter()
        field = ctx.bake_probe_field(parts, SIZE, SIZE, (0.8, 0.8, 0.8), None, 1, probes, (16, SETS), (16, SETS), 0, 2, (0.0, 0.0, 0.0), 1e-3, 1e3, None, (64, SETS))
        clock["bake_probe_field"].append((time.perf_counter() - t0) * 1.0e3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(atlas_only, field)), "the atlas of a probe field is bake_bounce_atlas's"
    up = probe.irradiance(field[3], np.array([0.0, 1.0, 0.0], np.float32))
    ctx.close()
    return {"config": config, "atlas": [SIZE, SIZE], "parts": len(parts), "probes": int(probes.size), "probe_K": 64, "K": 16, "light_K": 16, "bounces": 1,
            "host_clock_ms": {k: {"median": statistics.median(v), "all": v} for k, v in clock.items()}, "mean_irradiance_up": float(up.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["E", "D"])
    ap.add_argument("--field-configs", nargs="*", default=["E"])
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--tree", type=int, default=3, help="hiprz_set_tree (3 = TREE_DEVICE_SAH: device-built trees)")
    ap.add_argument("--other", default=None, help="a second build of libhiprz_probe.so to time in the same rounds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for config in args.configs:
        lines.append(json.dumps(measure(config, args.repeats, args.tree, args.other)))
        print(lines[-1], flush=True)
    for config in args.field_configs:
        lines.append(json.dumps(measure_field(config, args.tree)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
