#!/usr/bin/env python3
"""Device time of bounce baking (include/hiprz_gather.h) beside the best route there was before it: hiprz_query_closest over the SAME n*K
hemisphere rays, already on the device as hiprz_bake_rays emits them (point-major: the coherence of the gather, no host copy, no lookup and
no reduction — all of that favours the query).  The baseline is never the gather itself.  Medians of `--repeats`, HIP events on the
context's stream, the two sides timed alternately on one context in one process.

    python tools/gather_time.py --configs E D --out profiles/r27/gather_time.json

Per config: n = 2^16 surface points from the first hits of the pixel rays (evenly spaced over the hit pixels), near_ 1e-3, far_ 1e3, the
cosine table with S = 4, K in 16, 64.  Two chart maps over a 1024 x 1024 source in which every texel has a value, both mapping EVERY
instance, so that each front-face hit reads a texel: `random`, one chart per mesh triangle with UVs drawn at random — neighbouring hits
read texels anywhere in the 16 MB source, the most work a gather can have — and `atlas`, the mesh's own UVs scaled into a cell per
instance, as an atlas lays charts out: neighbouring hits read neighbouring texels.  `spread` is
(max - min) / median of a series.  The bar: the gather is no slower than the query by more than three times the larger of the two spreads;
the ratio and the spreads are written down whichever way they fall.  A figure is kept only when the emitted samples agree with the query's
hits on every ray: t in every byte, and the ids tests/gather_reference.py derives from the hits.  Also, on the host's clock for the
configs of --atlas-configs: Context.bake_bounce_atlas (one bounce, K = 16) against the direct-only Context.bake_light_atlas at 1024 x 1024 over the
instances whose meshes carry UVs, each scaled into a cell of its own."""
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
import gather_reference as GR  # noqa: E402  (the ids of the query's hits: the gate)
from rayzath_amd import _hiprt, atlas, bake, gather, query, scenes  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing  # noqa: E402
from rayzath_amd.scene import DirectLight, SpotLight, camera_struct, flatten  # noqa: E402

KS = (16, 64)
SETS = 4
POINTS = 1 << 16
SIZE = 1024


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


def full_chart_map(world, rng):
    """every instance mapped: one chart per mesh triangle, UVs drawn from [0, 1]^2"""
    counts = [len(inst.mesh.tri_vertices) for inst in world.instances]
    base = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32)
    uv = np.zeros(int(sum(counts)), gather.chart_dtype)
    for name in ("u1", "v1", "u2", "v2", "u3", "v3"):
        uv[name] = rng.random(len(uv))
    return base, uv


def measure(config, repeats, tree):
    world = lit_world(config)
    flat, cam = flatten(world), camera_struct(world.camera)
    assert len(flat.instances) == len(world.instances)
    ctx = Context(0)
    ctx.set_tree(tree)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(scenes.CONFIGS[config]["max_depth"], 8)).struct())
    points = surface_points(ctx, POINTS)
    n = len(points)
    rng = np.random.default_rng(27)
    maps = {"random": full_chart_map(world, rng), "atlas": gather.chart_tables(atlas_parts(world), len(flat.instances))}
    source = gather.records(rng.uniform(0.0, 4.0, (SIZE, SIZE, 3)), (SIZE, SIZE))
    g, b, q = ctx.gatherer(), ctx.bake(), ctx.query()
    d_points, d_texels, d_source = _hiprt.DeviceBuffer.of(points), _hiprt.DeviceBuffer(n * 16), _hiprt.DeviceBuffer.of(source)
    out = {"config": config, "width": cam.width, "height": cam.height, "points": n, "instances": len(flat.instances), "charts": {k: len(v[1]) for k, v in maps.items()}, "source": [SIZE, SIZE],
           "sets": SETS, "tree": ctx.tree(), "repeats": repeats, "per_k": []}
    for name, K in [(name, K) for K in KS for name in maps]:
        base, uv = maps[name]
        g.set_charts(base, uv)
        g.set_directions((K, SETS)), b.set_directions((K, SETS))
        rays_n = n * K
        d_rays, d_hits, d_samples = _hiprt.DeviceBuffer(rays_n * 32), _hiprt.DeviceBuffer(rays_n * 48), _hiprt.DeviceBuffer(rays_n * 16)
        gathers = lambda: g.texels_device(d_points.ptr, n, d_source.ptr, SIZE, SIZE, d_texels.ptr)
        asks = lambda: q.closest_device(d_rays.ptr, rays_n, d_hits.ptr)
        emits = lambda: g.samples_device(d_points.ptr, n, d_samples.ptr)
        b.rays_device(d_points.ptr, n, d_rays.ptr), gathers(), asks(), emits()
        ctx.sync()   # the tables are placed, first launches are done
        gathered, asked, emitted = series(ctx, [gathers, asks, emits], repeats)
        ctx.sync()
        texels, hits = d_texels.download((n,), gather.texel_dtype), d_hits.download((n, K), query.hit_dtype)
        samples = d_samples.download((n, K), gather.sample_dtype)
        # the gate: no figure without it
        assert samples["t"].tobytes() == hits["t"].tobytes(), "the emitted samples' t is not the query's on the bake's rays"
        assert np.array_equal(samples["id"], GR.ids(hits["flags"], hits["instance"], hits["triangle"], base, len(uv))), "the emitted ids are not those of the query's hits"
        assert texels.tobytes() == GR.texels(points, samples, uv, source, SIZE, SIZE, (0.0, 0.0, 0.0)).tobytes(), "the texels are not the restatement's over the samples"
        d_rays.free(), d_hits.free(), d_samples.free()
        sg, sq = stats(gathered), stats(asked)
        allowed = 3.0 * max(sg["spread"], sq["spread"])
        found = (hits["flags"] & query.HIT_FOUND) != 0
        out["per_k"].append({"K": K, "chart_map": name, "rays": rays_n, "hits": int(found.sum()), "front_hits": int((samples["id"] < gather.MAX_CHARTS).sum()),
                             "back_hits": int((samples["id"] == gather.BACK).sum()), "gather": sg, "query_closest": sq, "gather_samples": stats(emitted),
                             "gather_over_query": sg["median_ms"] / sq["median_ms"], "bar_allowed_excess": allowed,
                             "bar_met": sg["median_ms"] <= sq["median_ms"] * (1.0 + allowed),
                             "bytes_read_per_point": {"gather": 32, "query": 32 * K}, "bytes_written_per_point": {"gather": 16, "query": 48 * K}})
    d_points.free(), d_texels.free(), d_source.free()
    ctx.close()
    return out


def atlas_parts(world):
    """(instance, charts) of every instance whose mesh carries a UV per vertex, each scaled into a cell of its own of a square grid"""
    have = []
    for i, inst in enumerate(world.instances):
        try:
            have.append((i, atlas.charts(inst.mesh)))
        except ValueError:
            pass
    side = int(np.ceil(np.sqrt(max(len(have), 1))))
    parts = []
    for k, (i, tris) in enumerate(have):
        cx, cy = k % side, k // side
        for v in (1, 2, 3):
            u = np.clip(tris[f"u{v}"], 0.0, 1.0)
            w = np.clip(tris[f"v{v}"], 0.0, 1.0)
            tris[f"u{v}"], tris[f"v{v}"] = (cx + 0.02 + 0.96 * u) / side, (cy + 0.02 + 0.96 * w) / side
        parts.append((i, tris))
    return parts


def measure_atlas(config, tree):
    world = lit_world(config)
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx = Context(0)
    ctx.set_tree(tree)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    parts = atlas_parts(world)
    clock = {"bake_light_atlas": [], "bake_bounce_atlas": []}
    for _ in range(3):
        ctx.sync()
        t0 = time.perf_counter()
        lit, _, ring = ctx.bake_light_atlas(parts, SIZE, SIZE, (16, SETS), 0, 2, 1e-3, 1e3)
        clock["bake_light_atlas"].append((time.perf_counter() - t0) * 1.0e3)
        ctx.sync()
        t0 = time.perf_counter()
        direct, indirect, ring2 = ctx.bake_bounce_atlas(parts, SIZE, SIZE, (0.8, 0.8, 0.8), None, 1, (16, SETS), (16, SETS), 0, 2, (0.0, 0.0, 0.0), 1e-3, 1e3)
        clock["bake_bounce_atlas"].append((time.perf_counter() - t0) * 1.0e3)
    assert direct.tobytes() == lit.tobytes() and ring.tobytes() == ring2.tobytes(), "the direct light of a bounce bake is bake_light_atlas's"
    covered = ring == 0
    ctx.close()
    return {"config": config, "atlas": [SIZE, SIZE], "parts": len(parts), "covered_texels": int(covered.sum()), "bounces": 1, "K": 16, "light_K": 16,
            "host_clock_ms": {k: {"median": statistics.median(v), "all": v} for k, v in clock.items()},
            "mean_indirect_over_mean_direct": float(indirect["mean"][covered].mean() / max(float(direct["light"][covered].mean()), 1e-30))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["E", "D"])
    ap.add_argument("--atlas-configs", nargs="*", default=["E"])
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--tree", type=int, default=3, help="hiprz_set_tree (3 = TREE_DEVICE_SAH: device-built trees)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for config in args.configs:
        lines.append(json.dumps(measure(config, args.repeats, args.tree)))
        print(lines[-1], flush=True)
    for config in args.atlas_configs:
        lines.append(json.dumps(measure_atlas(config, args.tree)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
