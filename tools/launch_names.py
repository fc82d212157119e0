#!/usr/bin/env python3
"""A fixed matrix of small contexts whose launches cover the launch plan's variants (rayzath_amd/csrc/hiprz_plan.cpp): pipelines 0 / 1 / 2,
staged and not, flat and deep worlds, lights and none, textures and none, reference and device-built trees, the compat integrator,
counted and uncounted renders, the walk orders, HIPRZ_SHADOW_PACKET and HIPRZ_BATCH_SEGMENTS.  Every context renders 2 passes, then 4
twice; one launch of the self-test kernel (hiprz_selftest with 1 case per thread) closes it, so a kernel trace of the run

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/launch_names.py

splits into contexts at rz_selftest_div_kernel.  Two builds of the library (HIPRZ_LIB) select the same kernels when, per context, the
multisets of (kernel name, grid, workgroup, LDS bytes) of the two traces are equal: `launch_names.py --compare A.csv B.csv`.
"""
import collections
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (scene, settings): scene = name of a builder below; settings: env = HIPRZ_* read at context creation, then setters by name
MATRIX = [
    ("cornell", {}),
    ("cornell", {"pipeline": 0}),
    ("cornell", {"pipeline": 1}),
    ("cornell", {"lds_scene": 0}),
    ("cornell", {"env": {"HIPRZ_BATCH_SEGMENTS": "3"}}),
    ("cornell", {"env": {"HIPRZ_BATCH_SEGMENTS": "1"}}),
    ("cornell", {"counted": True}),
    ("cornell", {"pipeline": 1, "traversal_mode": 1, "xcd_swizzle": True}),
    ("sphere", {"pipeline": 0, "traversal_mode": 1}),
    ("sphere", {"walk_order": 0}),
    ("room", {}),
    ("room", {"walk_order": 0}),
    ("room", {"walk_order": 2, "counted": True}),
    ("room", {"counted": True}),
    ("room", {"env": {"HIPRZ_SHADOW_PACKET": "1"}}),
    ("room", {"env": {"HIPRZ_SHADOW_PACKET": "0"}}),
    ("room", {"mode": 31}),
    ("room", {"mode": 63}),
    ("room", {"mode": 63, "pipeline": 0}),
    ("room", {"tree": 3}),
    ("dark room", {}),
    ("dark room", {"pipeline": 1}),
    ("dark room", {"tree": 3, "pipeline": 2}),
    ("dark room", {"pipeline": 2, "counted": True}),
    ("maps", {}),
    ("dark maps", {}),
    ("dark maps", {"pipeline": 2, "walk_order": 0}),
]
SEPARATOR = "rz_selftest_div_kernel"


def worlds():
    from rayzath_amd import scenes

    def dark(world):
        world.spot_lights.clear(), world.direct_lights.clear()
        world.material.emission = 1.0
        return world

    return {"cornell": lambda: scenes.cornell_box(96, 64), "sphere": lambda: scenes.cornell_sphere(96, 64, 12),
            "room": lambda: scenes.living_room(160, 96, 9), "dark room": lambda: dark(scenes.living_room(160, 96, 9)),
            "maps": lambda: scenes.shading_inputs_scene(160, 96), "dark maps": lambda: scenes.shading_inputs_scene(160, 96, lights=False)}


def run():
    from rayzath_amd.engine import Context, RenderConfig, Tracing
    from rayzath_amd.scene import camera_struct, flatten
    build, flat = worlds(), {}
    for name, settings in MATRIX:
        if name not in flat:
            world = build[name]()
            flat[name] = (flatten(world), camera_struct(world.camera))
        for key, value in settings.get("env", {}).items():
            os.environ[key] = value
        ctx = Context(0)
        for key in settings.get("env", {}):
            del os.environ[key]
        for key, value in settings.items():
            if key not in ("env", "counted"):
                getattr(ctx, "set_" + key)(value)
        ctx.upload_scene(flat[name][0]), ctx.upload_camera(flat[name][1]), ctx.set_config(RenderConfig(tracing=Tracing(4, 8)).struct())
        render = ctx.render_counted if settings.get("counted") else ctx.render
        for n in (2, 4, 4):
            render(n)
        ctx.sync()
        print(f"{name} {settings}: pipeline {ctx.pipeline()}, mode {ctx.traversal_mode()}, graph captures {ctx.graph_captures()}")
        ctx.selftest(1)
        ctx.close()


def contexts_of(path):
    """the trace's dispatches by start time, cut at the separator: a list of Counters of (kernel, grid, workgroup, LDS)"""
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    out, now = [], collections.Counter()
    for r in rows:
        if SEPARATOR in r["Kernel_Name"]:
            out.append(now)
            now = collections.Counter()
        else:
            size = lambda stem: tuple(int(r[f"{stem}_{axis}"]) for axis in "XYZ") if f"{stem}_X" in r else (int(r[stem]),)
            now[(r["Kernel_Name"], size("Grid_Size"), size("Workgroup_Size"), int(r["LDS_Block_Size"]))] += 1
    return out


def compare(a, b):
    ca, cb = contexts_of(a), contexts_of(b)
    assert len(ca) == len(cb) == len(MATRIX), f"{len(ca)} and {len(cb)} contexts in the traces, {len(MATRIX)} in the matrix"
    dispatches = differences = 0
    for (name, settings), x, y in zip(MATRIX, ca, cb):
        dispatches += sum(x.values())
        odd = (x - y) + (y - x)
        differences += sum(odd.values())
        print(f"{name} {settings}: {sum(x.values())} dispatches, {len(x)} distinct, {sum(odd.values())} differences")
        for key, count in odd.items():
            print("   ", count, "x", key)
    print(f"dispatches compared {dispatches}, differences {differences}")
    return 1 if differences else 0


if __name__ == "__main__":
    sys.exit(compare(sys.argv[2], sys.argv[3]) if len(sys.argv) == 4 and sys.argv[1] == "--compare" else run())
