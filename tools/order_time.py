#!/usr/bin/env python3
"""Device time of the ordered ray queries (include/hiprz_order.h) beside the caller-order queries (include/hiprz_query.h) on the pixel rays
of a BASELINE config in a fixed random permutation — the incoherent batch — and in pixel order: medians of `--repeats`, HIP events on the
context's stream, the variants of a comparison timed alternately on one context in one process.

    python tools/order_time.py --configs C D --out profiles/r18/order_time.json

Per config, for closest hit and for occlusion:
  (a) hiprz_query_*           on the permuted rays — the baseline, the kernel the order has to beat
  (b) hiprz_order_*           on the permuted rays — keys, sort and walk in one call
  (c) the stages of (b)       rz_order_keys_kernel + sort (hiprz_order_permutation), of which the sort alone (hiprz_sort_u32_device on keys
                              copied back before every run, the copy outside the timed window), and the walk alone (d)
  (d) hiprz_order_*_by        with a kept permutation
  (e) both libraries          on the rays in pixel order: what ordering costs a caller whose rays were coherent already
`spread` is (max - min) / median of a series.  The bar: (b) faster than (a) by more than three times the larger of the two spreads.  The
results of (b), (d) and (e) are compared with (a)'s bytes before anything is timed."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rayzath_amd import _hiprt, order, query, scenes  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing  # noqa: E402
from rayzath_amd.scene import camera_struct, flatten  # noqa: E402


def series(ctx, fns, repeats, before=None):
    """the functions timed in turn, `repeats` rounds: one list of milliseconds per function; before[k], if any, runs outside k's window"""
    a, b = _hiprt.Event(), _hiprt.Event()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            if before and before[k]:
                before[k]()
            a.record(ctx.stream())
            fn()
            b.record(ctx.stream())
            out[k].append(b.ms_since(a))
    a.destroy(), b.destroy()
    return out


def stats(ms):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "spread": (max(ms) - min(ms)) / med}


def verdict(a, b):
    """the project's bar: b faster than a by more than three times the larger spread"""
    allowed = 3.0 * max(a["spread"], b["spread"])
    gain = 1.0 - b["median_ms"] / a["median_ms"]
    return {"speedup": a["median_ms"] / b["median_ms"], "gain": gain, "bar_required_gain": allowed, "bar_met": gain > allowed}


def measure(config, repeats, tree):
    preset = scenes.CONFIGS[config]
    world = preset["build"]()
    flat, cam = flatten(world), camera_struct(world.camera)
    n = cam.width * cam.height
    ctx = Context(0)
    ctx.set_tree(tree)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(preset["max_depth"], 8)).struct())
    q, o = ctx.query(), ctx.order()
    rays_host = ctx.pixel_rays().reshape(-1)
    shuffle = np.random.default_rng(20261019).permutation(n)        # tools/query_time.py's permutation
    pixel, shuffled = _hiprt.DeviceBuffer.of(rays_host), _hiprt.DeviceBuffer.of(rays_host[shuffle])
    hits, occ, ref_hits, ref_occ = _hiprt.DeviceBuffer(n * 48), _hiprt.DeviceBuffer(n * 4), _hiprt.DeviceBuffer(n * 48), _hiprt.DeviceBuffer(n * 4)
    keys, keys_work, perm, perm_scratch = (_hiprt.DeviceBuffer(n * 4) for _ in range(4))
    rt = _hiprt.runtime()
    rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    # results first: every variant that is timed below writes (a)'s bytes
    q.closest_device(shuffled.ptr, n, ref_hits.ptr), q.occluded_device(shuffled.ptr, n, ref_occ.ptr)
    o.permutation_device(shuffled.ptr, n, perm.ptr, keys.ptr)
    ctx.sync()
    want_hits, want_occ = ref_hits.download((n,), query.hit_dtype), ref_occ.download((n,), np.uint32)
    keys_host, perm_host = keys.download((n,), np.uint32), perm.download((n,), np.uint32)
    assert np.array_equal(perm_host, np.argsort(keys_host, kind="stable").astype(np.uint32))
    for name, run in (("fused", lambda: (o.closest_device(shuffled.ptr, n, hits.ptr), o.occluded_device(shuffled.ptr, n, occ.ptr))),
                      ("kept order", lambda: (o.closest_device(shuffled.ptr, n, hits.ptr, perm_ptr=perm.ptr), o.occluded_device(shuffled.ptr, n, occ.ptr, perm_ptr=perm.ptr)))):
        rt.hipMemset(hits.ptr, 0xAB, n * 48), rt.hipMemset(occ.ptr, 0xAB, n * 4)
        run()
        ctx.sync()
        assert hits.download((n,), query.hit_dtype).tobytes() == want_hits.tobytes(), f"{config}: {name}: the ordered hits are not the caller-order hits"
        assert np.array_equal(occ.download((n,), np.uint32), want_occ), f"{config}: {name}: the ordered occlusion is not the caller-order occlusion"
    found = int((want_hits["flags"] & query.HIT_FOUND != 0).sum())
    q.closest_device(pixel.ptr, n, hits.ptr), o.closest_device(pixel.ptr, n, ref_hits.ptr)
    ctx.sync()
    assert hits.download((n,), query.hit_dtype).tobytes() == ref_hits.download((n,), query.hit_dtype).tobytes()

    def restore_keys():
        rt.hipMemcpyAsync(keys_work.ptr, keys.ptr, n * 4, 3, ctx.stream())       # device to device, on the timed stream, before the window

    def sort_alone():
        rc = ctx.lib.hiprz_sort_u32_device(ctx._ctx, keys_work.ptr, n, 24, perm_scratch.ptr, None)
        assert rc == 0

    out = {"config": config, "width": cam.width, "height": cam.height, "rays": n, "found": found, "tree": ctx.tree(), "repeats": repeats,
           "distinct_keys": int(len(np.unique(keys_host))), "rays_moved_by_the_order": int((perm_host != np.arange(n)).sum()),
           "libraries": [os.path.basename(query.LIB_PATH), os.path.basename(order.LIB_PATH)]}
    kinds = {"closest": (q.closest_device, o.closest_device, hits), "occluded": (q.occluded_device, o.occluded_device, occ)}
    for kind, (plain, ordered, dst) in kinds.items():
        a, b, d = series(ctx, [lambda: plain(shuffled.ptr, n, dst.ptr), lambda: ordered(shuffled.ptr, n, dst.ptr),
                               lambda: ordered(shuffled.ptr, n, dst.ptr, perm_ptr=perm.ptr)], repeats)
        e_plain, e_ordered = series(ctx, [lambda: plain(pixel.ptr, n, dst.ptr), lambda: ordered(pixel.ptr, n, dst.ptr)], repeats)
        r = {"a_query_shuffled": stats(a), "b_order_shuffled": stats(b), "d_order_by_kept_permutation": stats(d),
             "e_query_pixel_order": stats(e_plain), "e_order_pixel_order": stats(e_ordered)}
        r["b_against_a"] = verdict(r["a_query_shuffled"], r["b_order_shuffled"])
        r["d_against_a"] = verdict(r["a_query_shuffled"], r["d_order_by_kept_permutation"])
        gap = r["a_query_shuffled"]["median_ms"] - r["e_query_pixel_order"]["median_ms"]
        r["share_of_the_gap_to_pixel_order_closed_by_b"] = (r["a_query_shuffled"]["median_ms"] - r["b_order_shuffled"]["median_ms"]) / gap if gap > 0 else None
        r["order_over_query_in_pixel_order"] = r["e_order_pixel_order"]["median_ms"] / r["e_query_pixel_order"]["median_ms"]
        out[kind] = r
    keys_and_sort, sort_only = series(ctx, [lambda: o.permutation_device(shuffled.ptr, n, perm_scratch.ptr), sort_alone], repeats, before=[None, restore_keys])
    out["c_keys_and_sort"] = stats(keys_and_sort)
    out["c_sort_alone"] = stats(sort_only)
    out["c_keys_kernel_by_difference_ms"] = out["c_keys_and_sort"]["median_ms"] - out["c_sort_alone"]["median_ms"]
    out["c_walk"] = "d_order_by_kept_permutation of each kind"
    for buf in (pixel, shuffled, hits, occ, ref_hits, ref_occ, keys, keys_work, perm, perm_scratch):
        buf.free()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["C", "D"])
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
