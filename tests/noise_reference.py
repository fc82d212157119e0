"""numpy restatement of include/hiprz_noise.h ("THE NOISE LEVEL", "THE SUMMARY"): per-pixel error in display units, the 32x8 tile records
with the header's fixed summation order, and the host summary.  dtype float32 restates the device's arithmetic operation by operation;
float64 is the yardstick both are held against."""
import numpy as np

import denoise_reference as ref

TILE_W, TILE_H = 32, 8
LUM = (0.2126, 0.7152, 0.0722)


def tile_grid(width, height):
    return (width + TILE_W - 1) // TILE_W, (height + TILE_H - 1) // TILE_H


def pixel_error(accum, variance, aperture, exposure_time, min_batches=8, dtype=np.float64):
    """accum (H, W, 4) (R, A), variance (H, W, 4) (V, K) -> (e (H, W) in dtype, estimated (H, W) bool); e is only meaningful where estimated"""
    T = dtype
    k = ref.tone_k(aperture, exposure_time, T)
    accum, variance = np.asarray(accum, np.float32).astype(T), np.asarray(variance, np.float32).astype(T)
    with np.errstate(all="ignore"):
        a = np.where(accum[..., 3] == 0, T(1), accum[..., 3])
        r = accum[..., :3] / a[..., None]
        d = k * r + T(1)
        s = np.sqrt(variance[..., :3]) * (k / (d * d))
        e = (T(np.float32(LUM[0])) * s[..., 0] + T(np.float32(LUM[1])) * s[..., 1]) + T(np.float32(LUM[2])) * s[..., 2]
    assert e.dtype == T
    estimated = (variance[..., 3] >= T(min_batches)) & np.isfinite(e)
    return e, estimated


def lanes(image, fill=0):
    """(H, W) -> (tiles_y, tiles_x, 256): lane l = (y % 8) * 32 + (x % 32) of tile (y // 8, x // 32); lanes outside the frame hold `fill`"""
    H, W = image.shape
    tx, ty = tile_grid(W, H)
    padded = np.full((ty * TILE_H, tx * TILE_W), fill, dtype=image.dtype)
    padded[:H, :W] = image
    return padded.reshape(ty, TILE_H, tx, TILE_W).transpose(0, 2, 1, 3).reshape(ty, tx, TILE_H * TILE_W)


def ordered_sum(v):
    """(..., 256) -> (...): the header's order — down each wave of 64 lanes by halves (v[l] += v[l + s], s = 32 .. 1), then (w0 + w1) + (w2 + w3)"""
    w = np.array(v).reshape(v.shape[:-1] + (4, 64))
    s = 32
    while s >= 1:
        w[..., :s] = w[..., :s] + w[..., s:2 * s]
        s //= 2
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def tile_records(accum, variance, aperture, exposure_time, threshold=1.0 / 255.0, min_batches=8, dtype=np.float64):
    """(tiles_y, tiles_x, 4) in dtype: (sum e^2, max e, n_estimated, n_above) over each tile's estimated pixels"""
    T = dtype
    e, est = pixel_error(accum, variance, aperture, exposure_time, min_batches, T)
    e = np.where(est, e, T(0))
    sums = ordered_sum(lanes(e * e))
    peak = lanes(e).max(axis=-1)
    n_est = lanes(est.astype(T)).sum(axis=-1)
    n_above = lanes((est & (e > T(np.float32(threshold)))).astype(T)).sum(axis=-1)
    out = np.stack([sums, peak, n_est, n_above], axis=-1)
    assert out.dtype == T
    return out


def summary(tiles, width, height):
    """THE SUMMARY of (tiles_y, tiles_x, 4) tile records, in float64 over the tiles in index order: a dict with the fields of hiprz_noise_summary"""
    ty, tx = tiles.shape[:2]
    assert (tx, ty) == tile_grid(width, height)
    flat = np.asarray(tiles, np.float64).reshape(-1, 4)
    total, estimated, above, peak = 0.0, 0, 0, np.float32(0)
    best, worst, found = 0.0, 0, False
    for t, (s, m, n, na) in enumerate(flat):
        total += s
        estimated += int(n)
        above += int(na)
        peak = max(peak, np.float32(m))
        if int(n) == 0:
            continue
        with np.errstate(all="ignore"):
            rms_t = float(np.sqrt(s / float(int(n))))
        if not found or rms_t > best:
            best, worst, found = rms_t, t, True
    with np.errstate(all="ignore"):
        rms = float(np.sqrt(total / estimated)) if estimated else 0.0
    return dict(rms=rms, tile_rms_max=best, max=float(peak), worst_tile=worst, estimated=estimated, above=above, pixels=width * height,
                tiles_x=tx, tiles_y=ty)


def measure(accum, variance, aperture, exposure_time, threshold=1.0 / 255.0, min_batches=8, dtype=np.float64):
    """(summary dict, tile records) of a frame: what Context.noise returns, restated"""
    H, W = accum.shape[:2]
    tiles = tile_records(accum, variance, aperture, exposure_time, threshold, min_batches, dtype)
    return summary(tiles, W, H), tiles
