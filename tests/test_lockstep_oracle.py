"""The lockstep comparison (tests/lockstep.py) and its generated scenes (tests/generated_scenes.py), proven on the CPU: the generator's
conditions, the calibration of the rule that tests/test_lockstep_gpu.py holds the device to, and that the rule catches every mutant oracle
(oracle/Makefile: one deliberate rare-case bug each) standing in for the device.  Run with -s for the tables."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import generated_scenes as G
import lockstep
import oracle
from lockstep import OracleDevice, bad
from rayzath_amd.engine import COMPAT_SCATTERING

COMPAT_MODES = (0, 31, 63)   # the integrators tests/test_lockstep_gpu.py sweeps: the CPU engine's, and the CUDA-compat flags without / with reprojection
MUTANTS = ("wrap_trunc", "slot_wrap", "slot_last", "abs_scale", "spot_angle", "sky_uv", "ior_one")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _renderer(seed, lib=None, mode=0):
    flat, cam, cfg = G.flat_scene(seed)[:3]
    return oracle.OracleRenderer(flat, cam, cfg, lib=lib, mode=mode)


@pytest.fixture(scope="module")
def frames(built):
    """per seed: first-pass hit share, and whether accumulator and state are finite after 8 free-running passes of the oracle"""
    out = {}
    for seed in G.SEEDS:
        ref = _renderer(seed)
        ref.render(1, threads=1)
        hit = float((ref.depth < G.flat_scene(seed)[1].near_far[1]).mean())
        ref.render(G.PASSES - 1, threads=1)
        finite = bool(np.isfinite(ref.accum).all() and all(np.isfinite(v).all() for v in ref.state.values()))
        out[seed] = dict(hit=hit, finite=finite, accum=ref.accum)
        ref.close()
    return out


def test_sweep_has_sixty_scenes_that_the_validator_accepts(built):
    from rayzath_amd import _lib
    lib = _lib.load()
    assert len(G.SEEDS) >= 60 and len(set(G.SEEDS)) == len(G.SEEDS)
    for seed in G.SEEDS:
        msg = C.create_string_buffer(256)
        assert lib.hiprz_validate_scene(C.byref(G.flat_scene(seed)[0].struct), msg, 256) == 0, (seed, msg.value.decode())


def test_derived_scenes_have_no_lights_and_no_maps(built):
    """generated_scenes.DERIVED: "dark" scenes keep their maps and lose their lights, "bare" scenes lose both; the validator accepts them,
    the oracle's frames stay finite, and they are what SEEDS lacks: a scene without lights that has no map either"""
    from rayzath_amd import _lib
    lib = _lib.load()
    assert not [s for s in G.SEEDS if not len(G.flat_scene(s)[0].textures) and not len(G.flat_scene(s)[0].spot_lights) + len(G.flat_scene(s)[0].direct_lights)]
    for key in G.DERIVED:
        flat, original = G.flat_scene(key)[0], G.flat_scene(key[1])[0]
        msg = C.create_string_buffer(256)
        assert lib.hiprz_validate_scene(C.byref(flat.struct), msg, 256) == 0, (key, msg.value.decode())
        assert len(flat.spot_lights) == len(flat.direct_lights) == 0 and len(flat.instances) == len(original.instances), key
        assert (len(flat.textures) == 0) if key[0] == "bare" else (len(flat.textures) == len(original.textures) > 0), key
        ref = _renderer(key)
        ref.render(G.PASSES, threads=1)
        assert np.isfinite(ref.accum).all() and all(np.isfinite(v).all() for v in ref.state.values()), key
        ref.close()


def test_cameras_see_the_objects(frames):
    """at least 70 % of the scenes with instances have a first-pass hit share of at least 0.1"""
    shares = [frames[s]["hit"] for s in G.SEEDS if G.flat_scene(s)[3].instances]
    seen = float(np.mean(np.array(shares) >= 0.1))
    print(f"scenes with instances: {len(shares)}, hit share >= 0.1 on {seen:.3f} of them, mean hit share {np.mean(shares):.3f}")
    assert seen >= 0.7


def test_every_feature_occurs_in_three_scenes(built):
    counts = {name: sum(bool(f(*G.flat_scene(s)[3:])) for s in G.SEEDS) for name, f in G.FEATURES.items()}
    print("\n".join(f"  {n:3d}  {name}" for name, n in sorted(counts.items(), key=lambda kv: kv[1])))
    assert not {name: n for name, n in counts.items() if n < 3}


def test_frame_sizes_and_depths(built):
    sizes = {(G.flat_scene(s)[1].width, G.flat_scene(s)[1].height) for s in G.SEEDS}
    assert sizes == set(G.SIZES) == {(48, 32), (17, 41), (33, 33), (64, 3), (1, 1)}
    assert {G.flat_scene(s)[2].max_depth for s in G.SEEDS} == {1, 2, 6, 16}


def test_oracle_frames_are_finite(frames):
    assert [s for s in G.SEEDS if not frames[s]["finite"]] == []


def test_same_seed_gives_the_same_bytes_in_another_process(built):
    """generated_world is deterministic from the seed alone: the FlatScene, camera and config bytes of a few scenes, hashed here and in a
    fresh interpreter"""
    code = ("import sys, hashlib, ctypes; sys.path[:0] = [%r, %r]; import generated_scenes as G\n"
            "for s in (0, 7, 23, 41, 59):\n"
            "    f, cam, cfg = G.flat_scene(s)[:3]; h = hashlib.sha256()\n"
            "    [h.update(getattr(f, k).tobytes()) for k in f.FIELDS]; h.update(bytes(cam)); h.update(bytes(cfg)); print(h.hexdigest())\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    runs = [subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout for _ in range(2)]
    assert runs[0] == runs[1] and len(runs[0].split()) == 5
    import hashlib
    mine = []
    for s in (0, 7, 23, 41, 59):
        f, cam, cfg = G.flat_scene(s)[:3]
        h = hashlib.sha256()
        for k in f.FIELDS:
            h.update(getattr(f, k).tobytes())
        h.update(bytes(cam)), h.update(bytes(cfg))
        mine.append(h.hexdigest())
    assert mine == runs[0].split()


@pytest.mark.parametrize("mode", COMPAT_MODES)
def test_oracle_against_itself_is_exact(built, mode):
    """harness self-test: the plain oracle in the device's place (on four threads, the reference on one) is `exact` on every segment, in
    the CPU engine's mode and in the compat modes the GPU sweep runs"""
    for seed in G.SEEDS:
        dev, ref = _renderer(seed, mode=mode), _renderer(seed, mode=mode)
        r = lockstep.lockstep(OracleDevice(dev, threads=4), ref, G.PASSES)
        dev.close(), ref.close()
        assert r["exact"] == r["segments"] and bad(r) == 0 and r["depth_mismatch"] == 0, (seed, lockstep.describe(r))


def test_packaging_sweep_comparison_on_the_oracle(built):
    """The comparison of tests/test_packaging_sweep_gpu.py (tests/packaging_sweep.py) with the oracle in the device's place, on the first 10
    scenes: the plain oracle through the call patterns (8,), (1, 2, 5) and (3, 5) equals its own pass-by-pass render — accumulator, depth,
    path state, ray and pass counts after 1, 3 and 8 passes —, and the "lo" libm stand-in as the variant is reported different on at
    least one scene (the comparison can fail)."""
    import packaging_sweep as S
    flagged = []
    for seed in G.SEEDS[:10]:
        base = _renderer(seed)
        want = S.pass_by_pass(OracleDevice(base))
        base.close()
        assert sorted(want) == list(S.KEPT) and want[8]["passes"] == 8 and want[3]["rays"] == 3 * want[1]["rays"] > 0
        same, lo = _renderer(seed), _renderer(seed, lib=oracle.variant("lo"))
        assert S.compare_patterns(OracleDevice(same, threads=4), want) == [], seed
        if S.compare_patterns(OracleDevice(lo), want):
            flagged.append(seed)
        same.close(), lo.close()
    print(f"packaging sweep comparison: the 'lo' stand-in differs from the plain oracle on scenes {flagged}")
    assert flagged


def test_packaging_sweep_comparison_names_what_differs(built):
    """one changed value in one snapshot — a pixel's accumulator, a path depth, the ray count — is reported with its pass count and name"""
    import packaging_sweep as S
    ref = _renderer(0)
    want = S.pass_by_pass(OracleDevice(ref))
    ref.close()
    assert S.differences(want, want) == []
    for name, change in (("accum", lambda v: np.nextafter(v, np.float32(np.inf))), ("state.depth", lambda v: v + 1), ("state.origin", lambda v: -v),
                         ("depth", lambda v: np.nextafter(v, np.float32(0)))):
        got = {n: dict(snap) for n, snap in want.items()}
        got[3][name] = want[3][name].copy()
        got[3][name].reshape(-1)[5] = change(got[3][name].reshape(-1)[5])
        assert [(p, f) for p, f, _ in S.differences(got, want)] == [(3, name)], name
    got = {n: dict(snap) for n, snap in want.items()}
    got[8]["rays"] += 1
    assert [(p, f) for p, f, _ in S.differences(got, want)] == [(8, "rays")]
    nan = {n: dict(snap) for n, snap in want.items()}
    nan[1]["accum"] = want[1]["accum"].copy()
    nan[1]["accum"][0, 0, 0] = np.nan
    assert S.differences(nan, nan) == [] and [(p, f) for p, f, _ in S.differences(nan, want)] == [(1, "accum")]


def test_adopt_continues_a_frame(built):
    """an oracle that adopts another's frame after 3 passes renders the same 4th pass, bit for bit"""
    a, b = _renderer(0), _renderer(0)
    a.render(3, threads=1)
    b.adopt(a.accum, a.state, a.passes)
    a.render(1, threads=1), b.render(1, threads=1)
    assert np.array_equal(a.accum, b.accum) and b.passes == 4
    for k, v in a.state.items():
        assert np.array_equal(v, b.state[k]), k
    a.close(), b.close()


@pytest.mark.parametrize("mode", COMPAT_MODES)
def test_calibration_of_the_libm_standins(built, mode):
    """Lockstep counts of the six libm stand-ins (every inexact libm result moved 1 or 2 ulps down / up / one of the two per argument)
    against the plain oracle.  The one-ulp stand-ins are what the device's caps are made of: no scene may show discrete + far on more than
    1e-3 of its segments, the sweep on no more than 1e-4, in every mode the GPU sweep runs — and the first-hit depth, which no libm call
    precedes, is bit-equal (with HIPRZ_COMPAT_SCATTERING: wherever the medium did not scatter the first segment; a scattered depth is
    -logf(u + 1e-4) / sigma and moves with the nudge)."""
    names = lockstep.STANDINS + lockstep.STANDINS_2
    totals, segments = {n: [0, 0] for n in names}, 0
    print(f"\nmode {mode}\nseed  size   depth segments | " + " | ".join(f"{n:>4s} d/f" for n in names) + " | scene cap")
    for seed in G.SEEDS:
        counts = lockstep.standin_counts(seed, mode, names=names)
        cam, cfg = G.flat_scene(seed)[1:3]
        n = counts["lo"]["segments"]
        segments += n
        for name in names:
            totals[name][0] += counts[name]["discrete"]
            totals[name][1] += counts[name]["far"]
            if not mode & COMPAT_SCATTERING:
                assert counts[name]["depth_mismatch"] == 0, (seed, name)
        if any(bad(counts[name]) for name in names):
            print(f"{seed:4d}  {cam.width:2d}x{cam.height:<2d}  {cfg.max_depth:5d} {n:8d} | " +
                  " | ".join(f"{counts[n_]['discrete']:4d}/{counts[n_]['far']:<3d}" for n_ in names) + f" | {lockstep.scene_cap(seed, mode)}")
        for name in lockstep.STANDINS:
            assert bad(counts[name]) <= 1e-3 * n, (seed, name, bad(counts[name]), n)
    print(f"sweep {segments} segments | " + " | ".join(f"{totals[n_][0]:4d}/{totals[n_][1]:<3d}" for n_ in names) +
          f" | sweep cap {lockstep.sweep_cap(G.SEEDS, mode)}   (scenes not listed: 0 everywhere, cap 2)")
    for name in lockstep.STANDINS:
        assert sum(totals[name]) <= 1e-4 * segments, (name, totals[name], segments)


def _free_running_bar_flags(seed, lib, ref_accum):
    """today's bar of the hand-built scenes: 8 free-running passes, rgb within rel 1e-3 on at least 0.99 of the pixels"""
    dev = _renderer(seed, lib=lib)
    dev.render(G.PASSES, threads=1)
    acc = dev.accum
    dev.close()
    with np.errstate(invalid="ignore"):
        close = (np.abs(acc[..., :3] - ref_accum[..., :3]) <= 1e-3 * np.maximum(np.abs(ref_accum[..., :3]), 1.0)).all(-1).mean()
    return close < 0.99


@pytest.mark.parametrize("mutant,mode", [(m, 0) for m in MUTANTS] + [("spot_angle", 31), ("slot_wrap", 31), ("abs_scale", 63)])
def test_the_rule_flags_every_mutant(frames, mutant, mode):
    """A mutant oracle in the device's place breaks the rule the GPU is held to (discrete + far above the scene's cap) on at least one
    scene.  Printed for the record: on how many scenes, and on how many the free-running bar would have noticed."""
    lib = oracle.variant("mut_" + mutant)
    flagged, old_bar, total = [], [], 0
    for seed in G.SEEDS:
        dev, ref = _renderer(seed, lib=lib, mode=mode), _renderer(seed, mode=mode)
        r = lockstep.lockstep(OracleDevice(dev), ref, G.PASSES, records=1)
        dev.close(), ref.close()
        total += bad(r)
        if bad(r) > lockstep.scene_cap(seed, mode) or r["depth_mismatch"]:
            flagged.append(seed)
        if mode == 0 and _free_running_bar_flags(seed, lib, frames[seed]["accum"]):
            old_bar.append(seed)
    print(f"mutant {mutant} mode {mode}: lockstep rule flags {len(flagged)} scenes {flagged[:12]}, {total} discrete + far segments over the sweep "
          f"(sweep cap {lockstep.sweep_cap(G.SEEDS, mode)}); " +
          (f"the free-running bar flags {len(old_bar)} scenes {old_bar[:12]}" if mode == 0 else "free-running bar not run in this mode"))
    assert flagged
    assert total > lockstep.sweep_cap(G.SEEDS, mode)
