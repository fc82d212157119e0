"""rayzath_amd/csrc/hiprz_plan.cpp — which kernel instantiation every launch selects, with which grid and how much LDS — run WITHOUT a
GPU.  The unit and tests/launch_plan_shim.cpp are compiled with g++ under ASan, UBSan and libstdc++'s assertions into a program of
their own, which turns a file of PlanInputs records into a file of LaunchPlan records (a sanitizer abort fails one test, and nothing
built with a sanitizer is loaded into this process).

1. The plans equal, field by field, a numpy restatement of the rules as commit a709859 stated them in hiprz_api.hip and the launch
   units (each block below names the function it restates).  Inputs: the full cross product of the axes that decide pipeline, staging,
   deferral and the per-wave resident kernel (CROSS, with the boundary values of each), and beside every row of it a draw of the
   remaining axes (DRAWN: environment knobs, the scene's sizes) such that every pair of values of two different axes occurs.  The test
   asserts that coverage, and that every enumerator of every variant record is produced.
2. Invariants that do not depend on the restatement.
3. libhiprz.so holds exactly the kernels the library of a709859 held (tests/golden/launch_plan/kernels_a709859.txt) and the one
   kernel added since, which no launch plan selects: rz_selftest_math_kernel (hiprz_selftest_math.hip, a self-test entry point).
4. The kernel instantiations the uncounted plans of (1) name (kernel_identities) are the committed list
   tests/golden/launch_plan/identities.txt — what tests/test_packaging_sweep_gpu.py has to reach on the device.  The list is written by
   write_identities: run test_plan_against_the_parents_rules_and_invariants with HIPRZ_WRITE_IDENTITIES=1 after a rule changed on purpose.
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS"]
KIB = 1024
INTEGRATOR = 63 & ~32                                    # kIntegratorFlags
DEFER, NONE, PLAIN, COMPAT, COMPAT_DEFER = 4, 5, 6, 8, 9   # RZ_SHADOW_*
COOP_LDS, PARK, BINNED_FIXED, TOP_NODE = 8 * KIB, 8 * KIB, 15 * KIB, 36
WRM = 1920                                               # the HIPRZ_WAVE_RESIDENT_MAX whose boundary the tile counts straddle

INPUT_FIELDS = ["pipeline_setting", "traversal_mode", "lds_scene_override", "walk_order", "sort_rays", "sort_bits", "shadow_sort", "shadow_packet",
                "defer_shadow_rays", "nolight_kernels", "trace_waves", "batch_waves", "batch_segments",
                "wave_resident_max", "xcd_swizzle", "heavy_first", "mode_flags", "spot_samples", "direct_samples",
                "have_scene", "scene_tree", "lds_scene", "hot_bytes", "stack_entries", "world_stack_entries", "mesh_stack_entries",
                "n_instances", "n_lights", "n_textures", "n_nodes", "top_count", "flat_world", "have_camera", "n_local_tiles"]
inputs_dtype = np.dtype([(name, "<i4" if k < 13 else "<u4") for k, name in enumerate(INPUT_FIELDS)])   # hiprz::PlanInputs
TRACE = ["family", "waves", "one_leaf", "mode", "lds_scene", "grid", "block", "lds", "top_n"]
SHADE = ["active", "lds_scene", "shadow", "grid", "block", "lds", "top_n", "follow", "follow_grid", "follow_block", "follow_lds", "follow_top_n"]
FUSED = ["family", "mode", "lds_scene", "grid", "block", "lds"]
BATCH = ["family", "mode", "lds_scene", "shading", "five", "one_leaf", "grid", "block", "units", "lds", "park_offset", "segment_cap"]
HEAD = ["pipeline", "reported_mode", "walk_mode", "lds_scene", "blob", "tile_grid", "wave_grid", "stack_lds", "walk_lds", "sort_enabled", "sort_bits",
        "shadow_sort", "defer_shadows", "nee_quads", "wave_resident", "heavy_units"]
PLAN_FIELDS = HEAD + [f"{rec}.{f}" for rec, fields in (("trace", TRACE), ("shade", SHADE), ("fused", FUSED), ("batch", BATCH)) for f in fields]
plan_dtype = np.dtype([(name, "<u4") for name in PLAN_FIELDS])                                          # hiprz::LaunchPlan

# kernel families of hiprz_plan.hpp
TRACE_COMPAT, TRACE_COOP, TRACE_SKIP, TRACE_WORKGROUP = 1, 2, 3, 4
PACKET, PACKET_COLOUR, COOP3_COLOUR, COOP4, SKIP4, SKIP6 = 1, 2, 3, 4, 5, 6
FUSED_COMPAT, FUSED_PASS = 1, 2
BATCH_WAVE, BATCH_WORKGROUP = 1, 2

# hot_bytes by what the two LDS tests compare it with: resolve_pipeline's `hot + stack * 1024 + 15 KiB + 8 KiB <= 40 KiB` and
# use_lds_scene's `hot + stack * 1024 <= 160 KiB` — the values are `room - stack_entries * 1024`
HOT_ROOM = [17 * KIB, 17 * KIB + 1, 160 * KIB, 160 * KIB + 1]
CROSS = {   # full cross product
    "pipeline_setting": [-1, 0, 1, 2], "traversal_mode": [-1, 1, 2, 3], "lds_scene_override": [-1, 0, 1], "walk_order": [0, 1, 2],
    "mode_flags": [0, 32, 59, 63], "scene_tree": [0, 3], "lds_scene": [0, 1], "n_lights": [0, 2], "hot_room": HOT_ROOM,
    "n_local_tiles": [0, 1, WRM // 4 - 1, WRM // 4, WRM // 4 + 1, 511, 512, 2560, 2561, 8192, (32 << 16) // 256 + 1],
    "sort_rays": [-1, 0, 1], "spot_samples": [15, 16], "defer_shadow_rays": [0, 1]}
DRAWN = {   # one value per row, every pair of values present
    "sort_bits": [0, 8, 16, 24], "shadow_sort": [0, 1], "shadow_packet": [-1, 0, 1], "nolight_kernels": [0, 1], "trace_waves": [0, 4, 5, 6],
    "batch_waves": [0, 4], "batch_segments": [0, 1, 3], "wave_resident_max": [0, WRM, 1 << 30], "xcd_swizzle": [0, 1], "heavy_first": [0, 1],
    "have_scene": [0, 1], "stack_entries": [2, 12], "world_stack_entries": [1, 3], "mesh_stack_entries": [2, 3], "n_instances": [0, 15, 16],
    "n_textures": [0, 3], "n_nodes": [32768, 32769], "top_count": [100, 171, 273, 683], "flat_world": [0, 1], "have_camera": [0, 1]}
AXES = list(CROSS) + list(DRAWN)
VALUES = {**CROSS, **DRAWN}
CHUNK_AXES = ["pipeline_setting", "traversal_mode"]   # one run of the program per pair of these


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_shim")
    cmd = ["g++", *FLAGS, "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(CSRC, "hiprz_plan.cpp"),
           os.path.join(ROOT, "tests", "launch_plan_shim.cpp"), "-o", out]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    return out


def plans_of(program, records, counted):
    directory = os.path.dirname(program)
    src, dst = os.path.join(directory, "inputs.bin"), os.path.join(directory, "plans.bin")
    np.ascontiguousarray(records).tofile(src)
    proc = subprocess.run([program, src, dst, str(int(counted))], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert proc.stdout.split() == [str(inputs_dtype.itemsize), str(plan_dtype.itemsize), str(len(records))]
    return np.fromfile(dst, dtype=plan_dtype)


def chunk(fixed, seed):
    """the rows of the cross product with the CHUNK_AXES at `fixed`, as (records, value indices per axis)"""
    free = [a for a in CROSS if a not in CHUNK_AXES]
    grids = np.meshgrid(*[np.arange(len(CROSS[a])) for a in free], indexing="ij")
    n = grids[0].size
    index = {a: g.reshape(-1).astype(np.int64) for a, g in zip(free, grids)}
    for a, k in zip(CHUNK_AXES, fixed):
        index[a] = np.full(n, k, np.int64)
    rng = np.random.default_rng(seed)
    for a in DRAWN:
        index[a] = rng.integers(0, len(DRAWN[a]), n)
    rec = np.zeros(n, inputs_dtype)
    for a in AXES:
        if a != "hot_room":
            rec[a] = np.asarray(VALUES[a], np.int64)[index[a]].astype(rec[a].dtype)
    rec["hot_bytes"] = np.asarray(HOT_ROOM)[index["hot_room"]] - rec["stack_entries"].astype(np.int64) * 1024
    rec["direct_samples"] = 15
    return rec, index


def restate(r, counted):
    """The rules of a709859 over records `r` -> dict of plan fields (int64 arrays)."""
    i = {k: r[k].astype(np.int64) for k in INPUT_FIELDS}
    lights = i["n_lights"] != 0
    integrator = (i["mode_flags"] & INTEGRATOR) != 0
    rebuilt = i["scene_tree"] != 0
    nolight = i["nolight_kernels"] != 0
    tm, tiles = i["traversal_mode"], i["n_local_tiles"]
    # use_lds_scene
    staged = np.where((i["lds_scene_override"] == 0) | rebuilt | integrator, False,
                      np.where(i["lds_scene_override"] == 1, i["hot_bytes"] + i["stack_entries"] * 1024 <= 160 * KIB, i["lds_scene"] != 0))
    # resolve_pipeline
    dark_capable = (i["have_scene"] != 0) & ~staged & ~lights & nolight & (i["walk_order"] != 0) & ((tm == -1) | (tm == 3))
    small_dark = dark_capable & (i["have_camera"] != 0) & (tiles != 0) & (((tiles * 4) & 0xFFFFFFFF) <= i["wave_resident_max"])
    lds40 = i["hot_bytes"] + i["stack_entries"] * 1024 + BINNED_FIXED + 8 * KIB
    mode_ok = (tm == -1) | (tm == 1) | (tm == 2)
    auto = np.where((i["have_scene"] != 0) & (i["lds_scene"] != 0) & (i["lds_scene_override"] != 0) & mode_ok & (lds40 <= 40 * KIB), 2, 1)
    ps = i["pipeline_setting"]
    pipeline = np.where(integrator, np.where(ps == 0, 0, 1),
                        np.where(rebuilt, np.where(dark_capable & ((ps == 2) | ((ps < 0) & small_dark)), 2, 1),
                                 np.where(ps >= 0, ps, np.where(small_dark, 2, auto))))
    # wave_resident
    wave_resident = (pipeline == 2) & ~staged & ~lights & nolight & (i["walk_order"] != 0) & ((tm == -1) | (tm == 3))
    # effective_mode
    reported = np.where(rebuilt | integrator, 3, np.where(tm >= 0, tm, np.where((i["lds_scene"] == 0) & (pipeline == 1), 3,
                                                                                 np.where(i["mesh_stack_entries"] <= 2, 2, 1))))
    # defer_shadows
    samples = i["spot_samples"] + i["direct_samples"]
    defer = (i["defer_shadow_rays"] != 0) & (pipeline == 1) & ~staged & lights & (samples <= 30)
    # sort_enabled, effective_sort_bits, make_frame
    sorting = (pipeline == 1) & (i["sort_rays"] != 0) & ((i["sort_rays"] == 1) | (~staged & (reported >= 3) & ((i["n_instances"] >= 16) | (i["n_nodes"] <= 32768))))
    bits = np.where(i["sort_bits"] > 0, i["sort_bits"], np.where(~lights & (tiles * 256 <= (32 << 16)), 16, 24))
    shadow_sorting = sorting & (i["shadow_sort"] != 0) & (pipeline == 1) & defer
    units = np.where(pipeline == 2, np.where(wave_resident, tiles * 4, tiles), 0)
    heavy = np.where((i["heavy_first"] != 0) & (not counted), units, 0)
    # pass_geometry
    tile_grid = np.where(i["xcd_swizzle"] != 0, (tiles + 7) // 8 * 8, tiles)
    wave_grid = tiles * 4
    blob = np.where(staged, i["hot_bytes"], 0)
    walk = np.where((reported >= 3) & (staged | ((pipeline != 1) & ~wave_resident)), 1, reported)
    stack_lds = i["stack_entries"] * 1024
    walk_lds = np.where(walk == 2, BINNED_FIXED + (i["world_stack_entries"] + i["mesh_stack_entries"]) * 1024, np.where(walk == 1, stack_lds, 0))
    out = dict(pipeline=pipeline, reported_mode=reported, walk_mode=walk, lds_scene=staged, blob=blob, tile_grid=tile_grid, wave_grid=wave_grid,
               stack_lds=stack_lds, walk_lds=walk_lds, sort_enabled=sorting, sort_bits=bits, shadow_sort=shadow_sorting, defer_shadows=defer,
               nee_quads=4 + 2 * samples, wave_resident=wave_resident, heavy_units=heavy)
    split_kernels = (pipeline == 1) | wave_resident                       # launch_pass
    front = ((i["walk_order"] == 2) if counted else (i["walk_order"] != 0)) | rebuilt
    big = np.where(i["trace_waves"] > 0, i["trace_waves"] >= 6, i["n_nodes"] > 32768)
    skip_top = np.minimum(i["top_count"], np.where(big, 170, 272))
    one_leaf = (i["n_instances"] != 0) & (i["flat_world"] != 0)
    flat4 = staged & (i["flat_world"] != 0)

    def put(rec, launched, **fields):
        for name, value in fields.items():
            out[f"{rec}.{name}"] = np.where(launched, value, 0)

    # launch_trace_t
    coop = ~integrator & (walk == 3) & front
    skip = ~integrator & (walk == 3) & ~front
    wg = ~integrator & (walk != 3)
    waves = np.where(i["trace_waves"] > 0, i["trace_waves"], np.where(i["n_nodes"] > 32768, 5, 4))
    coop_waves = np.where(waves == 5, 5, np.where(waves >= 6, 6, 4))
    put("trace", split_kernels,
        family=np.select([integrator, coop, skip], [TRACE_COMPAT, TRACE_COOP, TRACE_SKIP], TRACE_WORKGROUP),
        waves=np.select([coop, skip], [coop_waves, np.where(big, 6, 4)], 0),
        one_leaf=coop & one_leaf & (coop_waves != 6),
        mode=np.where(wg, np.where(walk == 2, np.where(flat4, 4, 2), 1), 0), lds_scene=wg & staged,
        grid=np.where(wg, tile_grid, wave_grid), block=np.where(wg, 256, 64),
        lds=np.select([wg, skip], [blob + walk_lds, skip_top * TOP_NODE], COOP_LDS), top_n=np.where(skip, skip_top, 0))
    # shadow_beams, launch_shade_t
    beams = shadow_sorting & (i["shadow_packet"] != 0) & ((i["shadow_packet"] > 0) | (tiles * 256 >= 8192 * i["n_instances"])) & (not counted)
    colour = (i["mode_flags"] & 4) != 0
    dark = ~lights & nolight
    compat_defer = integrator & lights & defer
    plain = ~integrator & dark & (i["n_textures"] == 0)
    none = ~integrator & dark & (i["n_textures"] != 0)
    inline1 = ~integrator & ~dark & staged
    deferred = ~integrator & ~dark & ~staged & lights & defer
    inline3 = ~integrator & ~dark & ~staged & ~(lights & defer)
    shade_top = np.minimum(i["top_count"], 682)
    follow = np.select([compat_defer & colour & beams, compat_defer & colour, compat_defer & beams, compat_defer,
                        deferred & beams, deferred & front, deferred & big, deferred],
                       [PACKET_COLOUR, COOP3_COLOUR, PACKET, COOP4, PACKET, COOP4, SKIP6, SKIP4], 0)
    skips = (follow == SKIP4) | (follow == SKIP6)
    put("shade", split_kernels, active=1, lds_scene=(plain | none | inline1) & staged,
        shadow=np.select([compat_defer, integrator, plain, none, inline1, deferred], [COMPAT_DEFER, COMPAT, PLAIN, NONE, 1, DEFER], 3),
        grid=tile_grid, block=256, lds=np.select([plain | none, inline1, inline3], [blob, blob + stack_lds, shade_top * TOP_NODE], 0),
        top_n=np.where(inline3, shade_top, 0), follow=follow, follow_grid=np.where(follow != 0, wave_grid, 0), follow_block=np.where(follow != 0, 64, 0),
        follow_lds=np.select([follow == 0, follow == PACKET, follow == PACKET_COLOUR, skips], [0, 2048, 3072, skip_top * TOP_NODE], COOP_LDS),
        follow_top_n=np.where(skips, skip_top, 0))
    # launch_fused_t
    put("fused", ~split_kernels, family=np.where(integrator, FUSED_COMPAT, FUSED_PASS),
        mode=np.where(integrator, 0, np.where(walk == 2, np.where(flat4, 4, 2), 1)), lds_scene=~integrator & staged, grid=tile_grid, block=256,
        lds=np.where(integrator, 0, blob + np.where(walk == 2, walk_lds + 4096, walk_lds)))
    # launch_batch_t
    reference_counters = bool(counted) & (i["walk_order"] != 2) & ~rebuilt
    wave = wave_resident & ~reference_counters
    b_mode = np.where(wave_resident & reference_counters, 1, walk)
    b_walk_lds = np.where(wave_resident & reference_counters, stack_lds, walk_lds)
    b_lds = blob + b_walk_lds + PARK
    b_plain = dark & (i["n_textures"] == 0)
    five = (b_lds * 5 <= 160 * KIB) & (tile_grid > 2 * 5 * 256) & (i["batch_waves"] != 4)
    put("batch", pipeline == 2, family=np.where(wave, BATCH_WAVE, BATCH_WORKGROUP),
        mode=np.where(wave, 3, np.where(b_mode == 2, np.where(flat4, 4, 2), 1)), lds_scene=~wave & staged,
        shading=np.where(b_plain, PLAIN, np.where(dark | wave, NONE, 1)), five=~wave & b_plain & five, one_leaf=wave & one_leaf,
        grid=np.where(wave, wave_grid, tile_grid), block=np.where(wave, 64, 256), units=np.where(wave, wave_grid, tile_grid),
        lds=np.where(wave, COOP_LDS, b_lds), park_offset=np.where(wave, 0, b_walk_lds),
        segment_cap=np.where(wave, 1, np.where(i["batch_segments"] > 0, i["batch_segments"], np.where(b_plain & five, 2, 1))))
    return {k: np.asarray(v).astype(np.int64) & 0xFFFFFFFF for k, v in out.items()}


def outside_the_lds_invariant(r, p):
    """Where "every launch's dynamic LDS <= 160 KiB" is not asserted: records no upload produces (lds_scene is set only for a blob with
    hot + stack columns + 15 KiB <= 52 KiB, hiprz_scene.hip), and the known break of the rules as they are:
    hiprz_set_lds_scene(1) admits a blob by `hot + stack columns <= 160 KiB` alone, and the launches add their workspace to it — a forced
    staging is left out only where the blob plus the largest workspace a launch can add (binned walk or stack columns, + the 8 KiB park)
    goes beyond 160 KiB; a forced staging that fits with it is held to the invariant like any other."""
    hot, stack = r["hot_bytes"].astype(np.int64), r["stack_entries"].astype(np.int64) * 1024
    binned = BINNED_FIXED + (r["world_stack_entries"].astype(np.int64) + r["mesh_stack_entries"]) * 1024
    forced_beyond = (r["lds_scene_override"] == 1) & (p["lds_scene"] != 0) & (hot + np.maximum(binned, stack) + PARK > 160 * KIB)
    return ((r["lds_scene"] != 0) & (hot + stack + BINNED_FIXED > 52 * KIB)) | forced_beyond


def lds_fields():
    return ["trace.lds", "shade.lds", "shade.follow_lds", "fused.lds", "batch.lds"]


def check_invariants(r, p):
    staged, split, resident = p["lds_scene"] != 0, p["pipeline"] == 1, p["wave_resident"] != 0
    lights, samples = r["n_lights"] != 0, r["spot_samples"] + r["direct_samples"]
    flags, rebuilt = (r["mode_flags"] & INTEGRATOR) != 0, r["scene_tree"] != 0

    def implies(a, b, what):
        bad = np.flatnonzero(a & ~b)
        assert bad.size == 0, f"{what}: {bad.size} records, first {r[bad[0]]} -> {p[bad[0]]}"

    implies(p["defer_shadows"] != 0, split & ~staged & lights & (samples <= 30), "deferral => split, not staged, lights, samples <= 30")
    implies(p["shadow_sort"] != 0, (p["sort_enabled"] != 0) & (p["defer_shadows"] != 0), "shadow sort => sort and deferral")
    implies(resident, (p["pipeline"] == 2) & ~lights & ~staged, "wave-resident => pipeline 2, no lights, not staged")
    for field in ("walk_mode", "trace.mode", "fused.mode"):
        implies(p[field] == 3, ~staged & (split | resident), f"{field} 3 => not staged, split or wave-resident")
    implies((p["batch.mode"] == 3), ~staged & resident & (p["batch.family"] == BATCH_WAVE), "batch mode 3 => the per-wave kernel")
    implies(flags, (p["pipeline"] <= 1) & ~staged, "integrator flags => pipeline 0 or 1, not staged")
    # (with an integrator flag the rules as they are let hiprz_set_pipeline(0) through: test_rebuilt_trees_never_fused)
    implies(rebuilt & ~flags, (p["pipeline"] == 1) | (p["pipeline"] == 2), "rebuilt trees => pipeline 1 or 2")
    implies(p["batch.five"] != 0, (p["batch.shading"] == PLAIN) & (p["batch.lds"].astype(np.int64) * 5 <= 160 * KIB), "five-wave batch => plain, 5 x LDS <= 160 KiB")
    known = outside_the_lds_invariant(r, p)
    for field in lds_fields():
        implies((p[field] > 160 * KIB) & ~known, np.zeros(len(r), bool), f"{field} <= 160 KiB")


# What names a kernel instantiation in a plan: per launch, the record that says whether the launch is made and the fields the launchers
# dispatch on (hiprz_launch_*.hip) — grids, LDS sizes and tree-top counts are launch arguments, not instantiations.
IDENTITY_FIELDS = {
    "trace": ("trace.family", ["trace.family", "trace.waves", "trace.one_leaf", "trace.mode", "trace.lds_scene"]),
    "shade": ("shade.active", ["shade.lds_scene", "shade.shadow"]),
    "follow": ("shade.follow", ["shade.follow"]),
    "fused": ("fused.family", ["fused.family", "fused.mode", "fused.lds_scene"]),
    "batch": ("batch.family", ["batch.family", "batch.mode", "batch.lds_scene", "batch.shading", "batch.five", "batch.one_leaf", "batch.segment_cap"]),
}
IDENTITIES = os.path.join(ROOT, "tests", "golden", "launch_plan", "identities.txt")


def kernel_identities(plan_record):
    """The kernel instantiations the plan(s) launch, as a set of tuples: ("trace", family, waves, one_leaf, mode, lds_scene),
    ("shade", lds_scene, shadow), ("follow", follow), ("fused", family, mode, lds_scene),
    ("batch", family, mode, lds_scene, shading, five, one_leaf, segment_cap > 1); a launch the plan does not make is left out.
    `plan_record`: one record or an array of plan_dtype, or the raw uint32 words of Context.launch_plan()."""
    p = np.atleast_1d(np.asarray(plan_record))
    if p.dtype != plan_dtype:
        p = np.ascontiguousarray(p, dtype=np.uint32).view(plan_dtype)
    out = set()
    for kind, (launched, fields) in IDENTITY_FIELDS.items():
        rows = p[p[launched] != 0]
        if not len(rows):
            continue
        columns = [(rows[f] > 1) if f == "batch.segment_cap" else rows[f] for f in fields]
        for row in np.unique(np.stack(columns, axis=1).astype(np.int64), axis=0):
            out.add((kind, *(int(v) for v in row)))
    return out


def identity_line(identity):
    return " ".join(str(v) for v in identity)


def read_identities():
    """tests/golden/launch_plan/identities.txt: every identity an uncounted plan of the input space below holds, one per line, sorted"""
    with open(IDENTITIES) as f:
        return {(w[0], *(int(v) for v in w[1:])) for w in (line.split() for line in f) if w}


def write_identities(identities):
    with open(IDENTITIES, "w") as f:
        f.write("".join(identity_line(i) + "\n" for i in sorted(identities)))


def test_plan_against_the_parents_rules_and_invariants(program):
    identities = set()
    seen_value = {a: np.zeros(len(VALUES[a]), bool) for a in AXES}
    seen_pair = {(a, b): np.zeros(len(VALUES[a]) * len(VALUES[b]), bool) for a in AXES for b in DRAWN if a != b}
    produced = {f: set() for f in PLAN_FIELDS if f.split(".")[-1] in ("family", "follow", "shadow", "shading", "mode", "waves", "pipeline", "reported_mode", "walk_mode")}
    total = 0
    for seed, fixed in enumerate(itertools.product(*[range(len(CROSS[a])) for a in CHUNK_AXES])):
        r, index = chunk(fixed, seed)
        total += len(r)
        for a in AXES:
            seen_value[a][index[a]] = True
        for (a, b), seen in seen_pair.items():
            seen[index[a][::5] * len(VALUES[b]) + index[b][::5]] = True
        for counted in (False, True):
            p = plans_of(program, r, counted)
            assert p.tobytes() == plans_of(program, r, counted).tobytes(), "the same input twice gives other bytes"
            want = restate(r, counted)
            for field in PLAN_FIELDS:
                bad = np.flatnonzero(p[field] != want[field])
                assert bad.size == 0, f"{field} (counted {counted}): {bad.size} of {len(r)} differ, first: {r[bad[0]]} gives {p[field][bad[0]]}, the parent's rules {want[field][bad[0]]}"
            check_invariants(r, p)
            if not counted:
                identities |= kernel_identities(p)
            for field, values in produced.items():
                values.update(np.unique(p[field]).tolist())
    assert total == int(np.prod([len(v) for v in CROSS.values()]))
    for a in AXES:
        assert seen_value[a].all(), f"axis {a}: value never used"
    for (a, b), seen in seen_pair.items():
        assert seen.all(), f"axes {a} x {b}: a pair of values never used"
    expect = {"pipeline": {0, 1, 2}, "reported_mode": {1, 2, 3}, "walk_mode": {1, 2, 3},
              "trace.family": {0, 1, 2, 3, 4}, "trace.waves": {0, 4, 5, 6}, "trace.mode": {0, 1, 2, 4},
              "shade.shadow": {0, 1, 3, DEFER, NONE, PLAIN, COMPAT, COMPAT_DEFER}, "shade.follow": {0, 1, 2, 3, 4, 5, 6},
              "fused.family": {0, 1, 2}, "fused.mode": {0, 1, 2, 4},
              "batch.family": {0, 1, 2}, "batch.mode": {0, 1, 2, 3, 4}, "batch.shading": {0, 1, NONE, PLAIN}}
    assert produced == expect
    # the instantiations the uncounted plans name: the universe tests/test_packaging_sweep_gpu.py has to reach (or exempt with a reason)
    if os.environ.get("HIPRZ_WRITE_IDENTITIES"):
        write_identities(identities)
    want = read_identities()
    assert identities == want, (f"not in identities.txt: {sorted(identities - want)[:5]}, no longer produced: {sorted(want - identities)[:5]} "
                                "(HIPRZ_WRITE_IDENTITIES=1 writes the list again)")


PINNED = dict(pipeline_setting=2, traversal_mode=-1, lds_scene_override=1, walk_order=1, sort_rays=-1, shadow_sort=1, shadow_packet=-1, defer_shadow_rays=1,
              nolight_kernels=1, wave_resident_max=1 << 30, heavy_first=1, spot_samples=1, direct_samples=1, have_scene=1, lds_scene=0,
              hot_bytes=160 * KIB - 8 * KIB - 2 * KIB + 1, stack_entries=2, world_stack_entries=1, mesh_stack_entries=3, n_instances=1, n_lights=1,
              n_nodes=3, top_count=3, have_camera=1, n_local_tiles=1)


@pytest.mark.xfail(strict=True, reason="use_lds_scene: a forced staging (hiprz_set_lds_scene(1)) admits a blob by hot + stack columns <= 160 KiB alone; "
                                       "the resident batch kernel adds its 8 KiB park (DESIGN.md §9)")
def test_forced_staging_fits_lds(program):
    """The smallest input at which the rule breaks: pipeline 2, a stack walk of 2 entries, a blob one byte beyond 160 KiB - 2 KiB - 8 KiB:
    the batch kernel asks for 160 KiB + 1 B."""
    r = np.zeros(1, inputs_dtype)
    for k, v in PINNED.items():
        r[k] = v
    p = plans_of(program, r, False)
    assert p["lds_scene"][0] == 1 and p["batch.family"][0] == BATCH_WORKGROUP
    print("batch.lds", p["batch.lds"][0])
    assert all(p[f][0] <= 160 * KIB for f in lds_fields())


@pytest.mark.xfail(strict=True, reason="resolve_pipeline: the integrator flags are looked at before the scene's trees, so hiprz_set_pipeline(0) "
                                       "puts rebuilt trees under the fused compat kernel (DESIGN.md §9)")
def test_rebuilt_trees_never_fused(program):
    """The smallest input at which "rebuilt trees => pipeline 1 or 2" breaks: one integrator flag, pipeline setting 0."""
    r = np.zeros(1, inputs_dtype)
    for k, v in PINNED.items():
        r[k] = v
    r["pipeline_setting"], r["lds_scene_override"], r["scene_tree"], r["mode_flags"] = 0, -1, 1, 1
    p = plans_of(program, r, False)
    print("pipeline", p["pipeline"][0])
    assert p["pipeline"][0] in (1, 2)


def test_rebuilt_trees_fused_is_what_the_rules_give(program):
    """the reason test_rebuilt_trees_never_fused fails: that input resolves to pipeline 0, and without the integrator flag to 1"""
    r = np.zeros(2, inputs_dtype)
    for k, v in PINNED.items():
        r[k] = v
    r["pipeline_setting"], r["lds_scene_override"], r["scene_tree"], r["mode_flags"] = 0, -1, 1, [1, 0]
    p = plans_of(program, r, False)
    assert p["pipeline"].tolist() == [0, 1] and p["fused.family"][0] == FUSED_COMPAT


def test_forced_staging_one_byte_less_fits(program):
    r = np.zeros(1, inputs_dtype)
    for k, v in PINNED.items():
        r[k] = v
    r["hot_bytes"] -= 1
    p = plans_of(program, r, False)
    assert p["lds_scene"][0] == 1 and p["batch.lds"][0] == 160 * KIB


def kernel_names(library):
    """the kernels' host stubs as tools/check_kernels.py reads them"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return set(module.host_stubs(library))


def test_kernel_set_is_the_parents():
    library = os.path.join(CSRC, "libhiprz.so")
    if not os.path.exists(library):
        pytest.skip("libhiprz.so is not built")
    with open(os.path.join(ROOT, "tests", "golden", "launch_plan", "kernels_a709859.txt")) as f:
        want = set(f.read().split())
    got = kernel_names(library)
    assert len(want) == 279
    added = {"_Z23rz_selftest_math_kerneljPKfjjPfj"}  # hiprz_selftest_math: evaluates hiprz_device.hpp's arithmetic, renders nothing
    assert not (added & want)
    assert got == want | added, f"missing {sorted((want | added) - got)[:3]}, new {sorted(got - want - added)[:3]}"
