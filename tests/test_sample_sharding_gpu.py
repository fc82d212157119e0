"""Sample sharding ("sample-sharding with per-frame ncclReduce of full accumulators"; include/hiprz.h:
hiprz_set_shard_mode).  Every part renders the whole share on its own seed stream; what leaves the context / the job is the sum.

  * a context over N parts in HIPRZ_SHARD_SAMPLES mode == the sum of N one-part frames on the seeds seed .. seed + N - 1, bit for bit
    (the sum is taken in part order), and == the sum of the ORACLE's frames on those seeds: finished-path counts exact, radiance within
    the stated tolerance, the tone-mapped pixels within one step of the oracle's tone map of its own sum
  * the mode composes with hiprz_set_shard, switching it restarts accumulation, tile mode afterwards is the one-device frame again
  * one process per GPU: ShardedFrame(mode="samples").reduce() — rehearsed with two ranks on GPU 0 over gloo through bench.py

The reference has nothing to compare with (one device, cuda_engine_core.cu:17); per seed the comparison is the usual one against the oracle.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from rayzath_amd import scenes
from rayzath_amd.engine import SHARD_SAMPLES, SHARD_TILES, Context, LightSampling, RenderConfig, Tracing
from rayzath_amd.scene import camera_struct, flatten

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 777


def _config(seed, lights=(1, 1), depth=5):
    return RenderConfig(LightSampling(*lights), Tracing(depth, 4), seed=seed).struct()


def _render(ctx, flat, cam, cfg):
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
    ctx.render(1), ctx.render(4), ctx.render(4)


def _oracle_tonemap(accum, cam):
    lib = oracle.load()
    out = np.zeros(accum.shape[:2] + (4,), np.uint8)
    px = np.ascontiguousarray(accum, dtype=np.float32)
    for y in range(accum.shape[0]):
        for x in range(accum.shape[1]):
            lib.rzo_tonemap_pixel(px[y, x].ctypes.data, cam.aperture, cam.exposure_time, out[y, x].ctypes.data)
    return out


@pytest.mark.parametrize("scene", ["cornell", "living room"])
@pytest.mark.parametrize("n", [2, 8])
def test_sample_sharded_context_is_the_sum_of_the_per_seed_frames(built, scene, n):
    world = scenes.cornell_box(96, 64) if scene == "cornell" else scenes.living_room(96, 64, 16)
    flat, cam = flatten(world), camera_struct(world.camera)
    many = Context([0] * n)
    many.set_shard_mode(SHARD_SAMPLES)
    assert many.shard_mode() == SHARD_SAMPLES and many.device_count() == n
    _render(many, flat, cam, _config(SEED))
    accum = many.read_accum()
    many.tonemap()
    image, depth = many.read_rgba8(), many.read_depth()
    assert many.ray_count() == n * 9 * 96 * 64            # every part traces the whole frame: n * passes * W * H (cpu_engine_renderer.cpp:173 per part)
    # --- against one-part contexts on the same seeds: the same sum, bit for bit (part order) ---
    gpu_sum = ref_sum = None
    for k in range(n):
        one = Context(0)
        _render(one, flat, cam, _config(SEED + k))
        a = one.read_accum()
        gpu_sum = a if gpu_sum is None else gpu_sum + a
        if k == 0:
            assert np.array_equal(depth, one.read_depth())   # the first pass shoots pixel-centre rays: every part's depth buffer
            state0 = one.read_state()
        one.close()
        ref = oracle.OracleRenderer(flat, cam, _config(SEED + k))
        ref.render(9)
        ref_sum = ref.accum if ref_sum is None else ref_sum + ref.accum
        if k == 0:
            assert np.array_equal(depth, ref.depth)
    assert np.array_equal(accum, gpu_sum)
    part0 = many.read_state()                                # part 0 answers for the path state
    assert all(np.array_equal(part0[key], state0[key]) for key in part0)
    # --- against the oracle's frames on the same seeds ---
    # finished paths: small integers, exact in any order.  Cornell: equal everywhere; with lights a path in ten thousand ends elsewhere behind
    # glibc-vs-ocml sinf / powf (per seed: alpha 99.99 % equal), and n seeds add their chances
    alpha_equal = (accum[..., 3] == ref_sum[..., 3]).mean()
    assert alpha_equal >= (1.0 if scene == "cornell" else 0.997), alpha_equal
    err = np.abs(accum[..., :3] - ref_sum[..., :3])
    ok = (err <= 1e-3 * np.maximum(np.abs(ref_sum[..., :3]), 1.0)).all(-1).mean()
    # Cornell: bit-exact per seed.  With lights a seed's frame is within 1e-3 on >= 99.3 % of the pixels (glibc-vs-ocml libm, the
    # bar of tests/test_parity_gpu.py), and a pixel of the sum is off when any of its n seeds is: 0.993 ** n (measured on MI355X at n = 8: 0.971)
    assert ok >= (1.0 if scene == "cornell" else 0.993 ** n), ok
    want = _oracle_tonemap(ref_sum, cam)
    assert (np.abs(image.astype(int) - want.astype(int)) <= 1).mean() >= (1.0 if scene == "cornell" else 0.993 ** n)   # (measured at n = 8: 0.988)
    assert image[..., 3].min() == 255
    many.close()


def test_sample_mode_composes_with_shards_and_switching_restarts(built):
    world = scenes.cornell_box(200, 120)
    flat, cam = flatten(world), camera_struct(world.camera)
    whole = Context([0, 0, 0])
    whole.set_shard_mode(SHARD_SAMPLES)
    _render(whole, flat, cam, _config(SEED))
    full = whole.read_accum()
    # the share split once more by the caller (a job of 2 processes x 3 parts): disjoint tiles, zero elsewhere
    halves, rays = [], 0
    for r in range(2):
        c = Context([0, 0, 0])
        c.set_shard_mode(SHARD_SAMPLES)
        c.set_shard(r, 2)
        _render(c, flat, cam, _config(SEED))
        halves.append(c.read_accum())
        rays += c.ray_count()
        c.close()
    assert np.array_equal(halves[0] + halves[1], full) and rays == whole.ray_count() == 3 * 9 * 200 * 120
    # a picked pixel is answered by part 0, which owns the whole share
    single = Context(0)
    _render(single, flat, cam, _config(SEED))
    for xy in [(10, 10), (100, 60), (150, 100)]:
        assert whole.pick(*xy) == single.pick(*xy)
    # back to tiles: accumulation restarts, and the frame is the one-device frame bit for bit
    whole.set_shard_mode(SHARD_TILES)
    whole.render(1), whole.render(4), whole.render(4)
    assert np.array_equal(whole.read_accum(), single.read_accum())
    assert whole.ray_count() == single.ray_count() == 9 * 200 * 120
    # and samples again: the same sum as before
    whole.set_shard_mode(SHARD_SAMPLES)
    whole.render(1), whole.render(4), whole.render(4)
    assert np.array_equal(whole.read_accum(), full)
    whole.close(), single.close()


@pytest.mark.parametrize("overlap", [1, 0])
def test_sharded_frame_reduce_in_process(built, overlap):
    """tests/sample_reduce_check.py: ShardedFrame(mode="samples").reduce() against the context's own readbacks for every export layout,
    and its stream choreography with both ranks of a 2-GPU job in one process (the reduce of frame k beside the rendering of frame k + 1)."""
    script = os.path.join(ROOT, "tests", "sample_reduce_check.py")
    r = subprocess.run([sys.executable, script, str(overlap)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "frames equal" in r.stdout


@pytest.mark.parametrize("mode", ["samples", "tiles"])
def test_bench_two_ranks_on_one_gpu(built, mode):
    """bench.py --gpus 2 as the driver types it (self-launched), both ranks on GPU 0 over gloo: the assembled frame is checked inside
    (--verify-gather: samples against the sum of the two one-GPU frames on the ranks' seeds, tiles against the unsharded frame) for the
    one-stream packaging, the hosts' default packaging (two streams per rank) and the other shard mode."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--repeats", "1", "--min-seconds", "0", "--config", "A",
           "--rehearse-on-one-gpu", "--no-cpu-baseline", "--verify-gather", "--shard-mode", mode, "--full"]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stdout[-1000:] + proc.stderr[-3000:]
    res = json.loads([l for l in proc.stdout.splitlines() if l.startswith("{")][-1])
    assert res["n_gpus"] == 2 and res["value"] > 0 and res["shard_mode"] == mode
    assert res["scaling"] == ("weak" if mode == "samples" else "strong")
    assert res["rays_per_step"] == 8 * 256 * 256 * (2 if mode == "samples" else 1)
    assert res["other_shard_mode"]["shard_mode"] == ("tiles" if mode == "samples" else "samples")
    assert res["hosts_default_packaging"]["streams"] == 2 and res["hosts_default_packaging"]["shard_mode"] == mode


@pytest.mark.parametrize("mode,rays", [("samples", "1.007M"), ("tiles", "503.8K")])
def test_headless_runner_over_two_parts(built, tmp_path, mode, rays):
    """hiprz_headless --devices 0,0: Hip::Engine over two parts (here both on GPU 0).  By default the runner sample-shards — each part
    renders whole frames on its own seed stream, Engine::ShardMode::Samples — so the report counts twice the rays of the 41 passes;
    --shard-mode tiles divides the frame instead and counts them once.  Either way the saved frame is a picture."""
    import re
    from rayzath_amd import scene_io
    world = scenes.cornell_box(128, 96)
    scene_io.save_scene_json(world, str(tmp_path / "cornell.json"))
    (tmp_path / "tasks.json").write_text('{"tasks": [{"scene path": "cornell.json", "engine": ["HIPGPU"], "rpp": 40, "timeout": 20.0, "max depth": 4}]}')
    exe = os.path.join(ROOT, "rayzath_amd", "csrc", "hiprz_headless")
    out_dir = tmp_path / "report"
    r = subprocess.run([exe, "--headless", str(tmp_path / "tasks.json"), str(out_dir), "-r", "--quiet", "--devices", "0,0", "--shard-mode", mode],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"Scene: cornell\.json\n\tengine: HIPGPU \| max depth: 4\n\tduration: \d+\.\d{3}s \| traced (\S+) rays \((\S+) rps\)\n", (out_dir / "report.txt").read_text())
    assert m and m.group(1) == rays, (out_dir / "report.txt").read_text()
    images = [f for f in os.listdir(out_dir) if f.endswith("_HIPGPU.png")]
    assert len(images) == 1
    frame = scene_io.read_image(str(out_dir / images[0]))
    assert frame.shape == (96, 128, 4) and (frame[..., 3] == 255).all() and frame[..., :3].max() > 100 and frame[..., :3].std() > 10
