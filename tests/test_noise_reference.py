"""The numpy restatement of include/hiprz_noise.h (tests/noise_reference.py) on inputs whose answer is known without it.  No GPU."""
import numpy as np
import pytest

import denoise_reference as ref
import noise_reference as nref

_CAM = dict(aperture=0.02, exposure_time=1.0 / 60.0)


def _frame(H, W, seed, K=8):
    rng = np.random.default_rng(seed)
    accum = np.zeros((H, W, 4), np.float32)
    accum[..., 3] = rng.integers(1, 9, (H, W))
    accum[..., :3] = rng.gamma(2.0, 0.5, (H, W, 3)) * accum[..., 3:4]
    variance = np.zeros((H, W, 4), np.float32)
    variance[..., :3] = rng.gamma(2.0, 0.02, (H, W, 3))
    variance[..., 3] = K
    return accum, variance


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_converged_frame_has_no_noise(dtype):
    accum, variance = _frame(20, 45, 1)
    variance[..., :3] = 0
    s, tiles = nref.measure(accum, variance, **_CAM, dtype=dtype)
    assert tiles.dtype == dtype and np.all(tiles[..., :2] == 0) and np.all(tiles[..., 3] == 0)
    assert s["estimated"] == s["pixels"] == 45 * 20 and s["above"] == 0
    assert s["rms"] == 0 and s["tile_rms_max"] == 0 and s["max"] == 0 and s["worst_tile"] == 0


def test_four_times_the_variance_doubles_every_error():
    accum, variance = _frame(20, 45, 2)
    four = variance.copy()
    four[..., :3] *= 4
    for T in (np.float32, np.float64):
        e1, est1 = nref.pixel_error(accum, variance, **_CAM, dtype=T)
        e2, est2 = nref.pixel_error(accum, four, **_CAM, dtype=T)
        assert est1.all() and est2.all() and (e1 > 0).all()
        if T is np.float32:
            assert np.array_equal(e2, 2 * e1)  # powers of two pass through sqrt, the products and the sums exactly
        else:
            assert np.abs(e2 / e1 - 2).max() < 1e-12
    a, _ = nref.measure(accum, variance, **_CAM)
    b, _ = nref.measure(accum, four, **_CAM)
    assert abs(b["rms"] / a["rms"] - 2) < 1e-12 and abs(b["tile_rms_max"] / a["tile_rms_max"] - 2) < 1e-12 and a["worst_tile"] == b["worst_tile"]


def test_a_one_pixel_frame_in_closed_form():
    r, A, v = 0.37, 5.0, 0.0123
    accum = np.array([[[r * A, r * A, r * A, A]]], np.float32)
    variance = np.array([[[v, v, v, 9]]], np.float32)
    k = ref.tone_k(**_CAM)
    r64, v64 = float(accum[0, 0, 0]) / A, float(variance[0, 0, 0])
    want = (np.float32(0.2126).astype(np.float64) + np.float32(0.7152) + np.float32(0.0722)) * np.sqrt(v64) * k / (k * r64 + 1) ** 2
    s, tiles = nref.measure(accum, variance, **_CAM, threshold=want * 0.99)
    assert tiles.shape == (1, 1, 4)
    assert abs(tiles[0, 0, 1] / want - 1) < 1e-12 and abs(tiles[0, 0, 0] / want ** 2 - 1) < 1e-12 and tuple(tiles[0, 0, 2:]) == (1, 1)
    assert abs(s["rms"] / want - 1) < 1e-12 and abs(s["tile_rms_max"] / want - 1) < 1e-12 and s["pixels"] == s["estimated"] == s["above"] == 1
    assert abs(s["max"] / want - 1) < 1e-6  # (the summary's max is a float)
    s, tiles = nref.measure(accum, variance, **_CAM, threshold=want * 1.01)
    assert s["above"] == 0 and s["estimated"] == 1
    # the slope of the tone curve: a finite difference of t(r) = kr / (kr + 1) through the same standard deviation
    t = lambda x: k * x / (k * x + 1)  # noqa: E731
    h = 1e-6 * np.sqrt(v64)
    assert abs((t(r64 + h) - t(r64 - h)) / (2 * h) * np.sqrt(v64) / (want / 1.0) - 1) < 1e-4
    f32, t32 = nref.measure(accum, variance, **_CAM, dtype=np.float32)
    assert t32.dtype == np.float32 and abs(t32[0, 0, 1] / want - 1) < 1e-6


def test_partial_tiles_count_only_pixels_inside_the_frame():
    W, H = 45, 20
    accum, variance = _frame(H, W, 3)
    s, tiles = nref.measure(accum, variance, **_CAM)
    assert tiles.shape == (3, 2, 4) and (s["tiles_x"], s["tiles_y"]) == (2, 3)
    want = np.array([[32 * 8, 13 * 8], [32 * 8, 13 * 8], [32 * 4, 13 * 4]])
    assert np.array_equal(tiles[..., 2], want) and s["estimated"] == W * H == want.sum()
    # the records are those of the tile's pixels alone
    e, _ = nref.pixel_error(accum, variance, **_CAM)
    block = e[16:20, 32:45]
    assert abs(tiles[2, 1, 0] / (block ** 2).sum() - 1) < 1e-12 and tiles[2, 1, 1] == block.max()
    rms_t = np.sqrt(tiles[..., 0] / tiles[..., 2])
    assert s["worst_tile"] == int(np.argmax(rms_t.reshape(-1))) and s["tile_rms_max"] == rms_t.max()
    assert abs(s["rms"] / np.sqrt((e ** 2).mean()) - 1) < 1e-12


def test_pixels_without_an_estimate_are_left_out():
    W, H = 45, 20
    accum, variance = _frame(H, W, 4)
    rng = np.random.default_rng(5)
    young = rng.uniform(size=(H, W)) < 0.2
    variance[young, 3] = rng.integers(0, 8, young.sum())          # K < min_batches, their V is not to be read
    variance[young, :3] = 1.0e6
    empty = (rng.uniform(size=(H, W)) < 0.1) & ~young             # no finished path: as the renderer leaves them, A = 0, K = 0, V = 0
    accum[empty] = 0
    variance[empty] = 0
    broken = np.zeros((H, W), bool)
    broken[3, 7] = broken[19, 44] = True                          # an infinite and a negative variance: e is not finite
    broken &= ~young & ~empty
    variance[3, 7, 1], variance[19, 44, 0] = np.inf, -1.0
    keep = ~young & ~empty & ~broken
    for T in (np.float32, np.float64):
        e, est = nref.pixel_error(accum, variance, **_CAM, min_batches=8, dtype=T)
        assert np.array_equal(est, keep)
        s, tiles = nref.measure(accum, variance, **_CAM, min_batches=8, dtype=T)
        assert s["estimated"] == keep.sum() < s["pixels"] and np.array_equal(tiles[..., 2], nref.lanes(keep.astype(int)).sum(-1))
        assert np.isfinite(tiles).all() and s["max"] == np.float32(e[keep].max()) and s["max"] < 1.0e3
    # min_batches moves the line; an A = 0 pixel that does have batches is read by the tone map's rule, a = 1
    s2, _ = nref.measure(accum, variance, **_CAM, min_batches=2)
    assert s2["estimated"] > s["estimated"]
    one = np.array([[[0.3, 0.3, 0.3, 0.0]]], np.float32), np.array([[[0.01, 0.01, 0.01, 8]]], np.float32)
    same = np.array([[[0.3, 0.3, 0.3, 1.0]]], np.float32)
    assert nref.measure(*one, **_CAM)[0] == nref.measure(same, one[1], **_CAM)[0]
    # nothing estimated at all: zeros, not a division by zero
    variance[..., 3] = 1
    s0, t0 = nref.measure(accum, variance, **_CAM)
    assert np.all(t0 == 0) and s0["estimated"] == 0 and s0["rms"] == 0 and s0["tile_rms_max"] == 0 and s0["worst_tile"] == 0


def test_the_fixed_summation_order_is_its_own():
    """lane 0 holds 2^24 and every other lane of wave 0 holds 1: summed lane by lane the ones vanish one at a time (2^24 + 1 rounds back to
    2^24); down the wave by halves they first pair up into 2, 4, ... 32, of which only the very first 1 is lost: 2^24 + 62."""
    v = np.zeros(256, np.float32)
    v[0], v[1:64] = 2.0 ** 24, 1.0
    got = nref.ordered_sum(v)
    assert got.dtype == np.float32 and got == np.float32(2.0 ** 24 + 62)
    sequential = np.float32(0)
    for x in v:
        sequential = np.float32(sequential + x)
    assert sequential == np.float32(2.0 ** 24)
    assert got.tobytes() != np.sum(v, dtype=np.float32).tobytes(), "np.sum happens to use the header's order on this input"
    assert nref.ordered_sum(v.astype(np.float64)) == 2.0 ** 24 + 63
    # across the waves: (w0 + w1) + (w2 + w3), not ((w0 + w1) + w2) + w3
    w = np.zeros(256, np.float32)
    w[0], w[64], w[128], w[192] = 2.0 ** 24, 0.0, 1.0, 1.0
    assert nref.ordered_sum(w) == np.float32(2.0 ** 24 + 2)
    # the restatement against the definition written out lane by lane
    rng = np.random.default_rng(6)
    x = (rng.gamma(2.0, 1.0, 256) * 10.0 ** rng.integers(-6, 6, 256)).astype(np.float32)
    lanes = x.copy()
    for wave in range(4):
        for s in (32, 16, 8, 4, 2, 1):
            for l in range(s):
                lanes[64 * wave + l] = np.float32(lanes[64 * wave + l] + lanes[64 * wave + l + s])
    want = np.float32(np.float32(lanes[0] + lanes[64]) + np.float32(lanes[128] + lanes[192]))
    assert nref.ordered_sum(x).tobytes() == want.tobytes()


def test_the_worst_tile_is_the_first_one_on_ties():
    tiles = np.zeros((3, 2, 4), np.float32)
    tiles[0, 1] = (4.0, 1.5, 4, 0)     # rms 1
    tiles[1, 0] = (9.0, 2.5, 9, 2)     # rms 1: a tie, the first stays
    tiles[2, 1] = (0.5, 0.5, 2, 0)
    s = nref.summary(tiles, 45, 20)
    assert s["worst_tile"] == 1 and s["tile_rms_max"] == 1.0 and s["max"] == 2.5 and s["estimated"] == 15 and s["above"] == 2
    assert s["rms"] == np.sqrt(13.5 / 15)
    tiles[0, 1] = 0                    # a tile without an estimate cannot be the worst, whatever its sum
    tiles[0, 0] = (100.0, 0.0, 0, 0)
    assert nref.summary(tiles, 45, 20)["worst_tile"] == 2
