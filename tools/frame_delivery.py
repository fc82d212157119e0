#!/usr/bin/env python3
"""What it costs to hand every frame to the host: bench.py's protocol (one context, one stream — or, with --streams N, the frame's tiles
over N streams of GPU 0, whose present goes through the head's staging —, renderFirstPass, warm-up, then timed
rounds of exactly --steps steps of 8 passes between sync fences, the loops alternating from round to round, median per loop) for

  render     render(8) + tone map                                            bench's `value`
  sync       render(8) + tone map + read_rgba8 + read_depth + ray_cast        what the hosts did per camera and call before hiprz_present
  pipelined  render(8) + present + read_frame(previous)                       frame N travels to pinned memory while N+1 renders

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RPP = 8


def measure(config, steps, warmup, rounds, streams=1):
    from rayzath_amd import scenes
    from rayzath_amd.engine import TREE_AUTO, Context, RenderConfig, Tracing
    from rayzath_amd.scene import camera_struct, flatten

    preset = scenes.CONFIGS[config]
    world = preset["build"]()
    flat, cam = flatten(world), camera_struct(world.camera)
    W, H = cam.width, cam.height
    x, y = W // 2, H // 2
    ctx = Context([0] * streams if streams > 1 else 0)
    ctx.set_tree(TREE_AUTO)
    ctx.upload_scene(flat)
    ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(preset["max_depth"], RPP)).struct())

    def render():
        ctx.render(RPP)
        ctx.tonemap()

    def sync():
        ctx.render(RPP)
        ctx.tonemap()
        ctx.read_rgba8(), ctx.read_depth(), ctx.ray_cast(x, y)

    def pipelined():
        ctx.render(RPP)
        seq = ctx.present(x, y)
        if seq > 1:
            ctx.read_frame(seq - 1)

    loops = {"render": render, "sync": sync, "pipelined": pipelined}
    ctx.render(1)
    for fn in loops.values():
        for _ in range(warmup):
            fn()
    ctx.sync()
    times = {k: [] for k in loops}
    names = list(loops)
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                loops[name]()
            ctx.sync()
            times[name].append(time.perf_counter() - t0)
    ctx.close()
    out = {}
    for name, t in times.items():
        med = sorted(t)[len(t) // 2]
        out[name] = {"Mrays_per_s": steps * RPP * W * H / med / 1e6, "ms_per_step": med / steps * 1e3, "rounds_s": t}
    for name in ("sync", "pipelined"):
        out[name]["vs_render"] = out[name]["Mrays_per_s"] / out["render"]["Mrays_per_s"]
    out["frame"] = f"{W}x{H}"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="B,C,E")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=1, help="contexts-with-a-stream on GPU 0 that share the frame (hiprz_create_multi)")
    ap.add_argument("--out")
    args = ap.parse_args()
    result = {"protocol": f"{args.rounds} alternating rounds of {args.steps} steps x {RPP} passes per loop, median round; one context, {args.streams} stream(s)",
              "configs": {c: measure(c, args.steps, args.warmup, args.rounds, args.streams) for c in args.configs.split(",")}}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
