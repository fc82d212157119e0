#!/usr/bin/env python3
"""Diagnostic (library built with -DRZ_PHASE_STATS, loaded through HIPRZ_LIB): for every kind of step of the MODE 3 walk, how many
times a WAVE executed it and with how many active lanes — i.e. where the trace kernel's VALU instructions go."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rayzath_amd import scenes
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.scene import camera_struct, flatten
NAMES = ["world node box test", "instance box test", "instance entry (to local)", "mesh node box test", "triangle test", "mesh walk round",
         "round on one lane per visit"]   # (the one-leaf binned walk: a round whose octets would not fit the workgroup)
# sample_direction (counted in the unit of the kernel that shades — the split pipeline's shade kernel here): the merged sampler's glossy
# branch, and inside it the powf / acosf / sincosf sequence (RZ_MIRROR_LOBE_CONST: lanes of roughness +-0 take constants instead)
LOBE_NAMES = {7: "lobe sampler entered", 8: "general glossy sequence"}
# binned_visit of the one-leaf walk (the trace unit's counters): the pair iterations behind a visit's first on a lane that holds the
# visit alone, the waves that reach such an iteration with the lanes that hold such a visit then (k), by k, and the dealt trips
DEAL_NAMES = {9: "later pair, lone-lane visit", 10: "waves with later pairs (k)", 11: "  of those with k <= 12", 12: "  with k 13 - 25",
              13: "  with k > 25", 14: "dealt trip"}
# closest_hit_flat ahead of its rounds: the lanes whose first candidate is a mesh of one leaf of at most 4 triangles (FlatWorld::small) and
# the lanes whose first candidate is anything else; then the first binned round, and how often it is on one lane per visit
FIRST_NAMES = {15: "first candidate: small leaf", 16: "first candidate: other", 17: "first binned round", 18: "  on one lane per visit"}
for cfgname in sys.argv[1:] or ["D"]:
    preset = scenes.CONFIGS[cfgname]
    w = preset["build"]()
    ctx = Context(0)
    if cfgname in ("A", "B"):
        ctx.set_traversal_mode(2), ctx.set_pipeline(1)   # workgroup-binned walk: same step kinds, "round" = one binning round
    else:
        ctx.set_traversal_mode(3), ctx.set_pipeline(1), ctx.set_ray_sort(int(os.environ.get('PHASE_RAY_SORT', '0')))
    ctx.set_tree(int(os.environ.get('PHASE_TREE', '4')))   # 4: the Engine hosts' default trees
    ctx.upload_scene(flatten(w)); ctx.upload_camera(camera_struct(w.camera)); ctx.set_config(RenderConfig(tracing=Tracing(preset["max_depth"], 8)).struct())
    out = (C.c_uint64 * 40)()
    ctx.render(9); ctx.sync(); ctx.lib.hiprz_read_phase_stats(out)
    if hasattr(ctx.lib, "hiprz_read_shadow_phase_stats"): ctx.lib.hiprz_read_shadow_phase_stats(out)
    ctx.render(1); ctx.sync(); ctx.lib.hiprz_read_phase_stats(out)
    waves = ((w.camera.width + 31) // 32) * ((w.camera.height + 7) // 8) * 4
    print(f"config {cfgname}: one pass, {waves} waves")
    for k, name in enumerate(NAMES):
        n, lanes = out[2 * k], out[2 * k + 1]
        print(f"  {name:28s} wave executions {n:12d} ({n / waves:8.1f} per wave)  lanes {lanes:13d}  mean active lanes {lanes / max(n, 1):5.1f}")
    if cfgname in ("A", "B"):
        for k, name in {**DEAL_NAMES, **FIRST_NAMES}.items():
            n, lanes = out[2 * k], out[2 * k + 1]
            print(f"  {name:28s} wave executions {n:12d} ({n / waves:8.3f} per wave)  lanes {lanes:13d}  mean active lanes {lanes / max(n, 1):5.1f}")
    if hasattr(ctx.lib, "hiprz_read_shadow_phase_stats"):   # the shade unit's counters of the SAME pass (read and cleared)
        ctx.lib.hiprz_read_shadow_phase_stats(out)
        for k, name in LOBE_NAMES.items():
            n, lanes = out[2 * k], out[2 * k + 1]
            print(f"  {name:28s} wave executions {n:12d} ({n / waves:8.3f} per wave)  lanes {lanes:13d}  mean active lanes {lanes / max(n, 1):5.1f}")
    if hasattr(ctx.lib, "hiprz_read_shadow_phase_stats") and os.environ.get("PHASE_SHADOW"):   # library built with -DRZ_PHASE_STATS in the shade unit too
        ctx.lib.hiprz_read_shadow_phase_stats(out); ctx.render(1); ctx.sync(); ctx.lib.hiprz_read_shadow_phase_stats(out)
        print("  shadow rays, wave-level walk (any_hit_packet):")
        for k, name in enumerate(NAMES[:5]):
            n, lanes = out[2 * k], out[2 * k + 1]
            print(f"  {name:28s} wave executions {n:12d} ({n / waves:8.1f} per wave)  lanes {lanes:13d}  mean active lanes {lanes / max(n, 1):5.1f}")
    ctx.close()
