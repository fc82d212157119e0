"""Probe placement on the GPU (include/hiprz_place.h: libhiprz_place.so, Context.place_probes / bake_probe_field(place=)).  The moved
probes and their records are held to the numpy float32 restatement (tests/place_reference.py) bit for bit, the restatement casting the
rays of tests/bake_reference.py from wherever it has the probe through Context.trace.  Trees 0 (reference) and 3 (device SAH).

THE WORLD is tests/gather_world.py's, THE PROBES tests/test_field_gpu.py's 67 points of free space with random frame axes, the middle one
spoiled, the first seven replaced by probes put inside and against the world's solids (SOLIDS).

  1 placement     K in 64 (one round), 128 (the selections carried over two), S in 1, 3, n in 1, 5, 67, iterations in 0, 1, 4: every
                  moved probe and record == the restatement; INSIDE, NEAR, CLEAR, STUCK (by the box and by the open direction), a move
                  and a distance capped at the reach all occur; records past n untouched, the in-place call and the call without
                  records give the same probes; every mutant caught on the device's output.
  2 ties          a table that stores every direction twice (k and k + 64): equal keys but for k on the device.
  3 two rooms     the (5, 2, 2) grid whose four middle probes stand in the 0.2 gap, baked end to end with and without place=.
  4 equality      bake_probe_field(place=) == its steps, place=None == the call without the keyword; a placement after
                  update_instances == a fresh context's; the refusals in the header's order; the C++ Engine delivers Python's bytes.

MEASURED ON MI355X: the nine cases in 1.5 s beside the session's build fixture.  Per tree, case 1: over the twelve n = 67 placements 623
CLEAR, 133 NEAR and 36 INSIDE records, 42 of them STUCK, 50 / 10 / 7 / 23 probes with 1 / 2 / 3 / 4 moves, every probe and record bit-equal
to the restatement, the five mutants caught.  Case 3, both trees alike: the four gap probes end NEAR after 4 moves at offsets of 0.29
along x, within 6e-8 of the analytic rooms'; 244 points count 853 probes unplaced and 1 092 placed; behind the wall the unplaced plain
blend and the placed weighted blend both read 0 (the bar holds trivially on this grid); the mirrored points in the lit room read 0.999847
and 0.999847 unplaced, 0.999847 and 0.757259 placed."""
import os
import subprocess

import numpy as np
import pytest

import bake_reference as BR
import field_reference as FR
import gather_world as GW
import place_reference as PL
import test_field_gpu as TF
from rayzath_amd import _abi, _hiprt, bake, field, gather, place, probe, scene_io
from rayzath_amd._lib import HiprzError
from rayzath_amd.engine import Context
from rayzath_amd.scene import flatten

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
TREES = (0, 3)
F = np.float32
N = TF.N
REACH = TF.REACH     # 2.0, below the world's size: some hits lie beyond it and are capped
PARAMS = dict(min_front=0.25, reach=REACH, max_offset=(0.3, 0.3, 0.3))
SOLIDS = (((0.2, 1.2, 0.0), (0.0, 1.0, 0.0)),        # the cube's centre: its faces are too far for the box — INSIDE and STUCK
          ((0.2, 1.38, 0.0), (1.0, 0.2, 0.0)),       # under the cube's top face: out through it
          ((-1.6, 0.9, -0.8), (0.0, 0.0, 1.0)),      # under the sphere's top
          ((1.5, -0.05, 1.5), (0.3, 1.0, 0.1)),      # under the floor, which has a back
          ((-0.5, 0.04, -2.0), (0.0, 1.0, 0.0)),     # on the floor: NEAR, up along its most open ray
          ((2.49, 0.05, 0.0), (0.7, -0.714, 0.0)),   # at the floor's edge, its axis over the edge: the most open ray points past the floor
          ((-1.0, 0.75, 0.9), (0.0, 0.0, -1.0)))     # before the wall


def _probes(n=N, spoil=True):
    out = TF._probes(N, spoil=False)
    for i, (position, axis) in enumerate(SOLIDS):
        out["position"][i], out["normal"][i] = position, axis
    out = out[:n].copy()
    if spoil and n >= 3:
        out["normal"][n // 2] = 0.0
    return out


def _params(K, iterations=4, **changes):
    return place.params(**{**PARAMS, "iterations": iterations, "max_back": K // 4, **changes})


def _is_the_invalid_record(record):
    return record["word"] == place.INVALID and not any(record[name].view(np.uint32).any() for name in ("offset", "front", "back", "n_back", "n_front"))


def _counting(cast, reach, seen):
    """`cast` that also counts the rays it answers and the hits beyond the reach"""
    def counted(rays):
        found, front, t = cast(rays)
        seen["rays"] += rays.size
        seen["capped"] += int((found & (t > F(reach))).sum())
        return found, front, t
    return counted


# =====================================================================================================================
# 1. the moved probes and the records are the restatement's over the device's own hits
# =====================================================================================================================
@pytest.mark.parametrize("tree", TREES)
def test_placement_bit_for_bit(built, tree):
    ctx, world, flat = TF._context(tree)
    try:
        caught = {m: False for m in PL.MUTANTS}
        seen = {"rays": 0, "capped": 0}
        cast = _counting(PL.trace_caster(ctx.trace), REACH, seen)
        words = []
        for K in (64, 128):
            for S in (1, 3):
                table = probe.sphere_directions(K, S)
                for n in (1, 5, N):
                    probes, seed = _probes(n), 20261021 + K
                    ok = BR.valid(probes)
                    for iterations in (0, 1, 4):
                        params = _params(K, iterations)
                        what = f"tree {tree} K {K} S {S} n {n} iterations {iterations}"
                        trail = []
                        want_probes, want = PL.place(probes, table, seed, params, cast, trail=trail)
                        moved, records = ctx.place_probes(probes, table, seed, params)
                        assert moved.dtype == probes.dtype and moved.shape == (n,) and records.dtype == place.record_dtype and records.shape == (n,)
                        assert records.tobytes() == want.tobytes(), f"{what}: {int((records.view(np.uint32) != want.view(np.uint32)).sum())} words of the records differ from the restatement"
                        assert moved.tobytes() == want_probes.tobytes(), f"{what}: the moved probes differ from the restatement"
                        # the first evaluation's rays are the bake's for the probes as given
                        assert trail[0][0].tobytes() == BR.rays(probes, table, seed).tobytes()
                        assert (place.moves(records) <= iterations).all() and (np.abs(records["offset"]) <= params["max_offset"]).all()
                        if n >= 3:
                            assert _is_the_invalid_record(records[n // 2])
                            assert moved[n // 2].tobytes() == probes[n // 2].tobytes(), "an invalid probe is copied unchanged"
                        still = place.moves(records) == 0
                        assert moved[still].tobytes() == probes[still].tobytes() and not records["offset"][still].view(np.uint32).any(), "a probe that made no move keeps every byte"
                        if iterations == 0:
                            assert still.all() and not (records["word"] & place.STUCK)[ok].any(), "iterations = 0 only classifies"
                        if n == N:
                            words.append(records["word"][ok])
                        if n == N and iterations == 4:
                            for m in caught:
                                got = PL.place(probes, table, seed, params, cast, m)
                                caught[m] |= got[0].tobytes() != moved.tobytes() or got[1].tobytes() != records.tobytes()
                            # the device-pointer call into guarded buffers: records and probes past n are untouched; in place; without records
                            ctx.sync()
                            guard = np.full((n + 2) * 8, 0xABABABAB, np.uint32)
                            bufs = [_hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer.of(guard), _hiprt.DeviceBuffer.of(guard)]
                            try:
                                ctx.placer().probes_device(bufs[0].ptr, n, bufs[1].ptr, bufs[2].ptr, seed, params)
                                ctx.sync()
                                back = [b.download(guard.shape, np.uint32) for b in bufs[1:]]
                            finally:
                                for b in bufs:
                                    b.free()
                            assert back[0][:n * 8].tobytes() == moved.tobytes() and (back[0][n * 8:] == 0xABABABAB).all(), f"{what}: the moved probes of the device-pointer call"
                            assert back[1][:n * 8].tobytes() == records.tobytes() and (back[1][n * 8:] == 0xABABABAB).all(), f"{what}: the records of the device-pointer call"
                            there, its = ctx.placer().probes_through_device(probes, seed, params, ctx.sync, in_place=True)
                            assert there.tobytes() == moved.tobytes() and its.tobytes() == records.tobytes(), f"{what}: out_probes_device == probes_device"
                            bare, none = ctx.placer().probes_through_device(probes, seed, params, ctx.sync, records=False)
                            assert none is None and bare.tobytes() == moved.tobytes(), f"{what}: a null out_records_device"
                            assert ctx.placer().probes(probes, seed, params, records=False)[0].tobytes() == moved.tobytes(), f"{what}: the host call without records"
        word = np.concatenate(words)
        state, stuck = word & place.STATE_MASK, (word & place.STUCK) != 0
        for name, value in (("CLEAR", place.CLEAR), ("NEAR", place.NEAR), ("INSIDE", place.INSIDE)):
            assert (state == value).any(), f"no probe is {name}"
        assert (stuck & (state == place.INSIDE)).any() and (stuck & (state == place.NEAR)).any(), "STUCK by the box and by the open direction"
        assert ((word >> 16) >= 2).any(), "no probe moved twice"
        assert seen["capped"] > 0, "no hit beyond the reach: the cap is not exercised"
        assert all(caught.values()), caught
        print(f"tree {tree}: {seen['rays']} rays cast by the restatement, {seen['capped']} hits capped at the reach; states over the n = {N} cases: "
              f"{np.bincount(state, minlength=3).tolist()}, {int(stuck.sum())} stuck, moves {np.bincount(word >> 16).tolist()}; mutants caught: {sorted(caught)}")
    finally:
        ctx.close()


# =====================================================================================================================
# 2. ties on the device: every direction stored twice
# =====================================================================================================================
def test_a_table_that_stores_every_direction_twice(built):
    ctx, world, flat = TF._context(3)
    try:
        half = probe.sphere_directions(64, 3)
        table = np.concatenate([half, half], axis=1)          # (3, 128, 4): k and k + 64 identical
        probes, params = _probes(), _params(128)
        cast = PL.trace_caster(ctx.trace)
        moved, records = ctx.place_probes(probes, table, 5, params)
        want_probes, want = PL.place(probes, table, 5, params, cast)
        assert records.tobytes() == want.tobytes() and moved.tobytes() == want_probes.tobytes()
        # every ray has its twin: the counts are even, and the placement is the half table's with twice the counts
        ok = BR.valid(probes)
        assert not (records["n_back"][ok] % 2).any() and not (records["n_front"][ok] % 2).any() and records["n_front"][ok].any()
        single_probes, single = ctx.place_probes(probes, half, 5, _params(128, max_back=16))     # max_back 32 of 128 is 16 of 64
        assert single_probes.tobytes() == moved.tobytes(), "ties go to the lowest k: the twin at k + 64 never wins"
        assert single["offset"].tobytes() == records["offset"].tobytes() and np.array_equal(single["word"], records["word"])
        assert np.array_equal(2 * single["n_back"], records["n_back"]) and np.array_equal(2 * single["n_front"], records["n_front"])
        assert (place.moves(records) > 0).any()
        # the mutant that lets the highest k win picks the twin: the same direction, so only a selection among DIFFERENT rays of equal
        # r shows it — O among the rays capped at the reach
        got = PL.place(probes, table, 5, params, cast, "ties_high")
        assert got[1].tobytes() != records.tobytes()
    finally:
        ctx.close()


# =====================================================================================================================
# 3. the two rooms end to end
# =====================================================================================================================
NEXT_TO_THE_GAP = ((0.3, 1.0, 0.1), (0.15, 0.7, -0.3), (0.5, 1.2, 0.2), (-0.3, 1.0, 0.1), (-0.15, 0.7, -0.3), (-0.5, 0.8, -0.2))
INSIDE_A_ROOM = ((-1.0, 1.0, 0.0), (-1.2, 0.8, 0.3), (1.0, 1.0, 0.0), (1.3, 1.2, -0.2))


@pytest.mark.parametrize("tree", TREES)
def test_the_two_rooms_placed_end_to_end(built, tree):
    world, parts, source = TF._two_room_world()
    ctx, _, flat = TF._context(tree, world)
    try:
        K = 64
        grid, probes, table, params = PL.gap_scene(K, 1)
        in_gap = probes["position"][..., 0] == 0.0
        assert in_gap.sum() == 4
        ctx.placer().set_directions((K, 1)), ctx.fielder().set_directions((K, 1))
        # the atlas's source is the emission: albedo 0, no light in the world — the first room's half holds 1
        args = (parts, 16, 8, (0.0, 0.0, 0.0), source, 1, probes, (64, 1), (16, 1), 0, 2, (0.0, 0.0, 0.0), TF.NEAR, TF.FAR, None, (64, 1), False)
        plain_sh, plain_vis = ctx.bake_probe_field(*args, visibility=4.0)[3:]
        assert (plain_vis["words"][in_gap][:, 1] > params["max_back"]).all(), "the gap probes see back faces"
        assert not plain_vis["words"][~in_gap][:, 1].any()
        baked = ctx.bake_probe_field(*args, visibility=4.0, place=params)
        assert len(baked) == 7
        sh, vis, moved, records = baked[3:]
        assert moved.shape == probes.shape and records.shape == probes.shape and records.dtype == place.record_dtype
        state = place.state(records)
        assert (state != place.INSIDE).all(), "a probe is still INSIDE"
        assert (np.abs(records["offset"]) <= params["max_offset"]).all() and (np.abs(moved["position"][in_gap][:, 0]) > 0.1).all()
        assert moved[~in_gap].tobytes() == probes[~in_gap].tobytes() and (records["word"][~in_gap] == place.CLEAR).all()
        assert not vis["words"][..., 1].any(), "no moved probe sees a back face"
        # the restatement over the device's hits, and over the analytic rooms: the same states, offsets within float32's reach of the walls
        want_probes, want = PL.place(probes.reshape(-1), table, 0, params, PL.trace_caster(ctx.trace))
        assert records.tobytes() == want.tobytes() and moved.tobytes() == want_probes.tobytes()
        analytic = PL.place(probes.reshape(-1), table, 0, params, PL.room_caster())[1]
        print(f"tree {tree}: offsets differ from the analytic rooms' by at most {np.abs(analytic['offset'] - records['offset'].reshape(-1, 3)).max():.2e}")
        look = field.params(bias=0.0, max_back=K // 4)
        near_gap, inside, leak = (bake.points(p, (0.0, 1.0, 0.0)) for p in (NEXT_TO_THE_GAP, INSIDE_A_ROOM, FR.LEAK_POINTS))
        everywhere = bake.points(np.random.default_rng(33).uniform((-1.9, 0.1, -0.9), (1.9, 1.9, 0.9), (256, 3)), (0.0, 1.0, 0.0))
        everywhere = everywhere[np.abs(everywhere["position"][:, 0]) > 0.1]          # not in the gap itself
        # next to the gap the unplaced field loses the gap probes
        before, after = ctx.lookup_field(grid, probes, plain_sh, near_gap, plain_vis, look), ctx.lookup_field(grid, moved, sh, near_gap, vis, look)
        assert (before["word"] != field.INVALID).all() and (after["word"] != field.INVALID).all()
        assert (before["word"] <= 4).all() and (before["word"] < after["word"]).all(), (before["word"], after["word"])
        before, after = ctx.lookup_field(grid, probes, plain_sh, everywhere, plain_vis, look), ctx.lookup_field(grid, moved, sh, everywhere, vis, look)
        had = before["word"] != field.INVALID
        assert (after["word"][had] != field.INVALID).all(), "a point lost its value to the placement"
        assert after["word"][had].sum() >= before["word"][had].sum(), "fewer probes take part after the placement"
        # the leak bar of test_the_two_rooms_end_to_end, the plain blend taken on the unplaced field
        plain = ctx.lookup_field(grid, probes, plain_sh, leak)["rgb"][:, 0]
        weighted = ctx.lookup_field(grid, moved, sh, leak, vis, field.params(bias=0.0))["rgb"][:, 0]
        lit_side = bake.points([(-p[0], p[1], p[2]) for p in FR.LEAK_POINTS], (0.0, 1.0, 0.0))
        lit = [ctx.lookup_field(grid, pr, s, lit_side, v, look)["rgb"][:, 0] for pr, s, v in ((probes, plain_sh, plain_vis), (moved, sh, vis))]
        for i, p in enumerate(FR.LEAK_POINTS):
            print(f"tree {tree} point {p}: unplaced plain {plain[i]:.6f} placed weighted {weighted[i]:.3e}; mirrored in the lit room: unplaced weighted {lit[0][i]:.6f} placed weighted {lit[1][i]:.6f}")
        print(f"tree {tree}: offsets of the gap probes {records['offset'][in_gap].tolist()}, states {state[in_gap].tolist()}, moves {place.moves(records)[in_gap].tolist()}; "
              f"probes counted over {int(had.sum())} points: {int(before['word'][had].sum())} unplaced, {int(after['word'][had].sum())} placed")
        assert (weighted <= plain / 100.0).all(), "the placed, weighted blend leaks more than 1/100 of the unplaced plain one"
        both = [ctx.lookup_field(grid, pr, s, inside, v, look)["rgb"] for pr, s, v in ((probes, plain_sh, plain_vis), (moved, sh, vis))]
        assert np.abs(both[0] - both[1]).max() <= 1e-3, "inside a room, away from the wall, the placed and the unplaced field differ"
        assert (both[0][:2] > 0.9).all() and not both[0][2:].any()
    finally:
        ctx.close()


# =====================================================================================================================
# 4. equality and delivery
# =====================================================================================================================
def test_a_placed_probe_field_is_its_steps_and_none_is_the_call_without(built):
    seed, rings, directions, samples, sky = 4, 2, (64, 3), (16, 3), (0.01, 0.02, 0.03)
    ctx, world, flat = TF._context(3)
    try:
        parts = GW.parts(world)
        albedo = gather.records((0.7, 0.6, 0.5), (TF.H, TF.W))
        emission = gather.records((0.0, 0.0, 0.0), (TF.H, TF.W))
        emission["rgb"][2:20, 2:10] = (0.0, 0.5, 0.0)
        lo, hi, shape = (-2.0, 0.05, -2.0), (2.0, 2.05, 2.0), (5, 3, 5)          # the lowest layer 0.05 above the floor: NEAR
        probes = probe.grid(lo, hi, shape)
        params = place.params_for(field.grid_of(lo, hi, shape), 0.25, REACH)
        args = (parts, TF.W, TF.H, albedo, emission, 1, probes, directions, samples, seed, rings, sky, TF.NEAR, TF.FAR, None, (64, 2))
        # place=None: the call without the keyword, with and without visibility
        want = ctx.bake_probe_field(*args)
        got = ctx.bake_probe_field(*args, place=None)
        assert len(want) == len(got) == 4 and all(g.tobytes() == w.tobytes() and g.dtype == w.dtype and g.shape == w.shape for g, w in zip(got, want))
        want5 = ctx.bake_probe_field(*args, visibility=REACH)
        got5 = ctx.bake_probe_field(*args, visibility=REACH, place=None)
        assert len(want5) == len(got5) == 5 and all(g.tobytes() == w.tobytes() for g, w in zip(got5, want5))
        assert all(g.tobytes() == w.tobytes() for g, w in zip(want5[:4], want))
        # place=params: the steps one by one (the placer and the fielder hold (64, 2) from here on)
        moved, records = ctx.place_probes(probes, (64, 2), seed, params)
        assert moved.shape == probes.shape and (place.moves(records) > 0).any() and (records["word"] != place.INVALID).all()
        assert (place.moves(records)[:, 0] > 0).all(), "the layer on the floor moves up"
        sh = ctx.bake_probe_field(*args[:6], moved, *args[7:])[3]
        vis = ctx.bake_visibility(moved, (64, 2), seed, REACH)
        got7 = ctx.bake_probe_field(*args, visibility=REACH, place=params)
        assert len(got7) == 7 and all(g.tobytes() == w.tobytes() for g, w in zip(got7[:3], want[:3])), "the atlas does not depend on the probes"
        for name, g, w in (("sh", got7[3], sh), ("vis", got7[4], vis), ("moved probes", got7[5], moved), ("records", got7[6], records)):
            assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"bake_probe_field(place=): {name} differ from the steps"
        assert got7[3].tobytes() != want[3].tobytes(), "the probes are baked where they were, not where they were moved to"
        got6 = ctx.bake_probe_field(*args, place=params)
        assert len(got6) == 6 and all(g.tobytes() == w.tobytes() for g, w in zip(got6, got7[:4] + got7[5:]))
    finally:
        ctx.close()


def test_a_placement_sees_update_instances(built):
    probes, seed = _probes(), 13
    params = _params(64)
    ctx, world, flat = TF._context(3)
    moved_world = GW.world(moved=True)
    try:
        before = ctx.place_probes(probes, (64, 3), seed, params)
        ctx.update_instances(flatten(moved_world).instances)
        after = ctx.place_probes(probes, None, seed, params)
        assert after[1].tobytes() != before[1].tobytes() and after[0].tobytes() != before[0].tobytes(), "the placement does not see the moved cube"
    finally:
        ctx.close()
    fresh, _, _ = TF._context(3, moved_world)
    try:
        again = fresh.place_probes(probes, (64, 3), seed, params)
        assert again[0].tobytes() == after[0].tobytes() and again[1].tobytes() == after[1].tobytes(), "a placement after update_instances differs from a fresh context's"
    finally:
        fresh.close()


def test_refusals_in_the_headers_order(built):
    ctx = Context(0)
    try:
        probes = _probes(5)
        pl = ctx.placer()
        good = _params(64)
        bad = good.copy()
        bad["reach"] = 0.0
        dev = 16          # a device address that is never read: every call below is refused or empty

        def refused(code, text, call, *args, **kwargs):
            with pytest.raises(HiprzError) as e:
                call(*args, **kwargs)
            assert e.value.code == code and text in str(e.value), (code, text, str(e.value))

        refused(_abi.ERR_INVALID, "null pointer", pl.probes_device, None, 1, dev, dev, 0, bad)
        refused(_abi.ERR_INVALID, "null pointer", pl.probes_device, dev, 1, None, dev, 0, bad)
        refused(_abi.ERR_STATE, "no direction table", pl.probes_device, dev, 2 ** 40, dev, None, 0, bad)
        refused(_abi.ERR_STATE, "no direction table", pl.probes, probes, 0, good)
        with pytest.raises(HiprzError):
            pl.set_directions(probe.sphere_directions(32, 2))                          # K < 64
        with pytest.raises(ValueError):
            pl.set_directions((16, 2))
        with pytest.raises(HiprzError):
            pl.set_directions(np.zeros((1, 64, 4), F))
        refused(_abi.ERR_STATE, "no direction table", pl.probes, probes, 0, good)     # what was set before stays: nothing
        pl.set_directions((64, 2))
        refused(_abi.ERR_INVALID, "n*K is 2^31 or more", pl.probes_device, dev, 2 ** 25, dev, None, 0, bad)
        refused(_abi.ERR_INVALID, "reach", pl.probes_device, dev, 2 ** 25 - 1, dev, None, 0, bad)
        for changes in (dict(min_front=np.nan), dict(reach=np.inf), dict(max_offset=(0.1, -1.0, 0.1)), dict(iterations=17), dict(reserved=1)):
            worse = good.copy()
            for k, v in changes.items():
                worse[k] = v
            refused(_abi.ERR_INVALID, list(changes)[0], pl.probes, probes, 0, worse)
        moved, records = pl.probes(probes[:0], 0, good)
        assert moved.shape == (0,) and records.shape == (0,), "n == 0 is OK without a scene"
        refused(_abi.ERR_STATE, "", pl.probes, probes, 0, good)                       # no scene: whatever hiprz_device_view refuses
        with pytest.raises(TypeError):
            ctx.place_probes(probes)
    finally:
        ctx.close()


def test_cpp_engine_places(built, tmp_path):
    exe = str(tmp_path / "place_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "place_delivery_check.cpp"), "-o", exe,
                    "-L", CSRC, "-lhiprz_host", "-lhiprz_place", "-lhiprz", "-Wl,-rpath," + CSRC], check=True)
    scene_path = str(tmp_path / "place.json")
    world = GW.world()
    scene_io.save_scene_json(world, scene_path)
    loaded = scene_io.load_scene_file(scene_path)
    K, S, seed = 128, 3, 20261021
    probes, params = _probes(), _params(K)
    ctx = Context(0)
    try:
        ctx.upload_scene(loaded.flat), ctx.upload_camera(loaded.camera)
        moved, records = ctx.place_probes(probes, (K, S), seed, params)
    finally:
        ctx.close()
        loaded.close()
    assert (place.moves(records) > 0).any() and records["word"][N // 2] == place.INVALID
    files = {name: str(tmp_path / (name + ".bin")) for name in ("probes", "params", "out")}
    probes.tofile(files["probes"]), params.reshape(1).tofile(files["params"])
    r = subprocess.run([exe, scene_path, files["probes"], files["params"], files["out"], str(K), str(S), str(seed)], capture_output=True, text=True, timeout=120)
    print("\n" + r.stdout[-2000:])
    assert r.returncode == 0 and "PLACE DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert open(files["out"], "rb").read() == moved.tobytes(), "Engine::placeProbes differs from Context.place_probes"
    assert open(files["out"] + ".records", "rb").read() == records.tobytes(), "the records of Engine::placeProbes differ from Context.place_probes"
