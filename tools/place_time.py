#!/usr/bin/env python3
"""Device time of probe placement (include/hiprz_place.h) beside what the project already had for the same work.

hiprz_place_probes beside hiprz_probe_samples over the SAME rays: the baseline is launched once per evaluation the placement actually
made, the e-th launch over the probes as they stood at their e-th evaluation, a probe that had stopped before made invalid (its rays are
then 16-byte stores of a code, no walk) so that every other probe keeps its index and with it its set of directions.  The baseline
stores 16 bytes per ray and decides nothing; the placement keeps the loop, the selections and the moves in one kernel and stores 64 bytes
per probe.  And beside the host loop it replaces: tests/place_reference.py's place() over Context.trace — the rays made in numpy, a host
round trip of rays and hits per evaluation, the selections in numpy — timed by the host's clock, once.  Medians of `--repeats`, HIP
events on the context's stream, the two device sides timed alternately on one context in one process.

    python tools/place_time.py --configs E --out profiles/r33/place_time.json

Per config: 4 096 probes, a 16^3 grid over the box of the camera's first hits, and 32 768, 32^3 over the same box; near_ 1e-3, far_ 1e3;
the sphere table with K = 256, S = 4; iterations 4, max_back K / 4, max_offset 0.45 of the grid's step, min_front a quarter of the
smallest step and reach three of the largest.  A figure is kept only when the moved probes and the records are the restatement's in every
byte — all of them: the host loop that is timed is the gate."""
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
import place_reference as PL  # noqa: E402  (the gate, and the host loop)
from gather_time import atlas_parts, lit_world, series, stats, surface_points  # noqa: E402
from rayzath_amd import _hiprt, field, gather, place, probe  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing  # noqa: E402
from rayzath_amd import scenes  # noqa: E402
from rayzath_amd.scene import camera_struct, flatten  # noqa: E402

K, SETS = 256, 4
GRIDS = ((16, 16, 16), (32, 32, 32))
ITERATIONS = 4


class Stood(list):
    """the trail of place(): where every probe stood at an evaluation and whether it was still moving, without the rays"""

    def append(self, item):
        rays, live = item
        super().append((rays["origin"][:, 0].copy(), live))


def row(ctx, placer, prober, table, probes, params, repeats):
    n = len(probes)
    # the host loop: the gate, the evaluations the placement makes and where every probe stands at each
    trail = Stood()
    t0 = time.perf_counter()
    want_probes, want = PL.place(probes, table, 0, params, PL.trace_caster(ctx.trace), trail=trail)
    host_ms = (time.perf_counter() - t0) * 1.0e3
    stood = []
    for position, live in trail:
        at = probes.copy()
        at["position"] = position
        at["normal"][~live] = 0.0
        stood.append(at)
    d_probes, d_moved, d_records = _hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer(n * 32), _hiprt.DeviceBuffer(n * 32)
    d_stood, d_samples = [_hiprt.DeviceBuffer.of(at) for at in stood], _hiprt.DeviceBuffer(n * K * 16)

    def baseline():
        for d in d_stood:
            prober.samples_device(d.ptr, n, d_samples.ptr, 0)

    fns = [lambda: placer.probes_device(d_probes.ptr, n, d_moved.ptr, d_records.ptr, 0, params), baseline]
    for fn in fns:
        fn()
    ctx.sync()   # the tables are placed, first launches are done
    timed = series(ctx, fns, repeats)
    ctx.sync()
    moved, records = d_moved.download((n,), probes.dtype), d_records.download((n,), place.record_dtype)
    assert records.tobytes() == want.tobytes() and moved.tobytes() == want_probes.tobytes(), "the placement is not the restatement's"
    for b in [d_probes, d_moved, d_records, d_samples, *d_stood]:
        b.free()
    st = {"place": stats(timed[0]), "probe_samples": stats(timed[1])}
    state, word = place.state(records), records["word"]
    live_counts = [int(live.sum()) for _, live in trail]
    return {"probes": n, "evaluations": len(trail), "probes_per_evaluation": live_counts, "rays_walked": int(sum(live_counts)) * K,
            "states": np.bincount(state[state != place.INVALID], minlength=3).tolist(), "stuck": int(((word & place.STUCK) != 0).sum()),
            "moves": np.bincount(place.moves(records), minlength=ITERATIONS + 1).tolist(), **st,
            "place_over_probe_samples": st["place"]["median_ms"] / st["probe_samples"]["median_ms"], "host_loop_ms": host_ms,
            "host_loop_over_place": host_ms / st["place"]["median_ms"]}


def measure(config, repeats, tree):
    world = lit_world(config)
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx = Context(0)
    ctx.set_tree(tree)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(scenes.CONFIGS[config]["max_depth"], 8)).struct())
    seen = surface_points(ctx, 1 << 14)["position"]
    lo, hi = seen.min(0), seen.max(0)
    lo, hi = lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo)
    table = probe.sphere_directions(K, SETS)
    placer, prober = ctx.placer(), ctx.prober()
    placer.set_directions(table), prober.set_directions(table)
    prober.set_charts(*gather.chart_tables(atlas_parts(world), len(flat.instances)))
    out = {"config": config, "box": [lo.tolist(), hi.tolist()], "K": K, "sets": SETS, "iterations": ITERATIONS, "instances": len(flat.instances), "tree": ctx.tree(),
           "repeats": repeats, "grids": []}
    for shape in GRIDS:
        grid = field.grid_of(lo, hi, shape)
        params = place._params(place.params_for(grid, 0.25 * float(grid["step"].min()), 3.0 * float(grid["step"].max()), ITERATIONS), K)
        probes = probe.grid(lo, hi, shape, (0.0, 1.0, 0.0), 1e-3, 1e3).reshape(-1)
        out["grids"].append({"grid": list(shape), "min_front": float(params["min_front"]), "reach": float(params["reach"]), "max_offset": params["max_offset"].tolist(),
                             "max_back": int(params["max_back"]), **row(ctx, placer, prober, table, probes, params, repeats)})
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["E"])
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
