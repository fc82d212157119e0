"""numpy restatement of the edge-avoiding a-trous filter as include/hiprz.h specifies it ("THE FILTER"), in the header's order of
operations, evaluated in the floating-point type `dtype`: float32 restates what the device computes, float64 is the reference both are
compared with.  The unit tests at the end are collected through tests/test_denoise_reference.py."""
import math
from types import SimpleNamespace

import numpy as np

from rayzath_amd import _abi

SPLINE = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)  # B3 spline, by |offset|


def params(iterations=5, sigma_normal=128.0, sigma_depth=0.1, sigma_color=0.7, demodulate=True):
    return SimpleNamespace(iterations=iterations, sigma_normal=sigma_normal, sigma_depth=sigma_depth, sigma_color=sigma_color,
                           flags=_abi.DENOISE_DEMODULATE if demodulate else 0)


def tone_k(aperture, exposure_time, dtype=np.float64):
    """k of the renderer's tone curve t(c) = kc / (kc + 1): pi * aperture^2 * exposure_time * 1e5, from the camera's fp32 values"""
    T = dtype
    return ((T(np.float32(aperture)) * T(np.float32(aperture)) * T(np.float32(math.pi))) * T(np.float32(exposure_time))) * T(1.0e5)


def make_guides(height, width, normal=(0.0, 0.0, -1.0), depth=1.0, albedo=(1.0, 1.0, 1.0), instance=0):
    g = np.zeros((height, width), dtype=_abi.guide_dtype)
    g["normal"], g["depth"], g["albedo"], g["instance"] = normal, depth, albedo, instance
    return g


def atrous(accum, guides, p, aperture, exposure_time, dtype=np.float64):
    """accum (H, W, 4) float32 accumulator image (alpha = finished paths), guides (H, W) of _abi.guide_dtype -> (H, W, 4) in `dtype`"""
    T = dtype
    H, W = accum.shape[:2]
    acc = accum.astype(T)
    count = np.where(acc[..., 3:4] == 0, T(1), acc[..., 3:4])
    c = acc[..., :3] / count
    demodulate = bool(p.flags & _abi.DENOISE_DEMODULATE)
    albedo = np.maximum(guides["albedo"].astype(T), T(np.float32(0.01)))
    if demodulate:
        c = c / albedo
    normal, z, inst = guides["normal"].astype(T), guides["depth"].astype(T), guides["instance"]
    k = tone_k(aperture, exposure_time, T)
    depth_scale = T(np.float32(p.sigma_depth)) * z + T(np.float32(1.0e-6))
    sigma_normal = T(np.float32(p.sigma_normal))
    for i in range(p.iterations):
        s = 1 << i
        kc = k * c
        t = kc / (kc + T(1))
        scale = T(np.float32(p.sigma_color)) / T(s)
        scale2 = scale * scale
        sum_c, sum_w = np.zeros((H, W, 3), T), np.zeros((H, W), T)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                spline = T(SPLINE[abs(dx)] * SPLINE[abs(dy)])
                if dx == 0 and dy == 0:
                    sum_c += spline * c
                    sum_w += spline
                    continue
                y0, y1, x0, x1 = max(0, -dy * s), H - max(0, dy * s), max(0, -dx * s), W - max(0, dx * s)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                nP, nQ = normal[P], normal[Q]
                dot = nP[..., 0] * nQ[..., 0] + nP[..., 1] * nQ[..., 1] + nP[..., 2] * nQ[..., 2]
                with np.errstate(all="ignore"):
                    w = spline * np.power(np.maximum(T(0), dot), sigma_normal)
                    w = w * np.exp(-(np.abs(z[P] - z[Q]) / depth_scale[P]))
                    w = np.where(inst[P] == _abi.GUIDE_MISS, spline, w)  # between two misses w_n = w_z = 1
                    if scale2 > 0:
                        d = t[P] - t[Q]
                        w = w * np.exp(-((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) / scale2))
                w = np.where(inst[P] == inst[Q], w, T(0)).astype(T)
                sum_c[P] += w[..., None] * c[Q]
                sum_w[P] += w
        c = sum_c / sum_w[..., None]
    out = np.ones((H, W, 4), T)
    out[..., :3] = c * albedo if demodulate else c
    return out


def tonemap_unquantised(image, aperture, exposure_time):
    """the renderer's tone curve on an RGBA image whose alpha is the sample count: (H, W, 3) in [0, 1), float64, before quantisation"""
    img = np.asarray(image, np.float64)
    count = np.where(img[..., 3:4] == 0, 1.0, img[..., 3:4])
    kc = tone_k(aperture, exposure_time) * (img[..., :3] / count)
    return kc / (kc + 1.0)


# --- unit tests of the restatement itself (no GPU) -------------------------------------------------------------------------------
_CAM = dict(aperture=0.02, exposure_time=1.0 / 60.0)


def test_a_constant_image_comes_back_unchanged():
    H, W = 40, 56
    accum = np.zeros((H, W, 4), np.float32)
    accum[..., :3], accum[..., 3] = (1.5, 0.75, 3.0), 4.0
    guides = make_guides(H, W, albedo=(0.5, 0.25, 1.0))
    for dtype, tol in ((np.float64, 1e-14), (np.float32, 1e-5)):
        out = atrous(accum, guides, params(), dtype=dtype, **_CAM)
        assert out.dtype == dtype
        assert np.abs(out[..., :3] - np.array([0.375, 0.1875, 0.75])).max() < tol and np.all(out[..., 3] == 1)


def test_nothing_crosses_an_instance_boundary():
    H, W = 48, 64
    rng = np.random.default_rng(3)
    accum = np.ones((H, W, 4), np.float32)
    accum[:, : W // 2, :3], accum[:, W // 2:, :3] = 10.0, rng.uniform(0.0, 1.0, (H, W // 2, 3))
    guides = make_guides(H, W)
    guides["instance"][:, W // 2:] = 7
    out = atrous(accum, guides, params(sigma_color=0.0), **_CAM)
    assert np.abs(out[:, : W // 2, :3] - 10.0).max() < 1e-12, "the noisy half leaked into the constant half"
    assert out[:, W // 2:, :3].max() <= 1.0 + 1e-12, "the bright half leaked into the noisy half"
    assert out[:, W // 2:, :3].std() < 0.5 * accum[:, W // 2:, :3].std(), "the noisy half was not smoothed"


def test_with_all_stops_open_an_iteration_is_the_plain_b3_convolution():
    H, W = 33, 47
    rng = np.random.default_rng(5)
    accum = np.ones((H, W, 4), np.float32)
    accum[..., :3] = rng.uniform(0.0, 2.0, (H, W, 3))
    guides = make_guides(H, W)
    for i, step in enumerate((1, 2, 4)):
        p = params(iterations=i + 1, sigma_normal=0.0, sigma_depth=1.0e30, sigma_color=0.0, demodulate=False)
        got = atrous(accum, guides, p, **_CAM)[..., :3]
        prev = accum[..., :3].astype(np.float64) if i == 0 else want
        num, den = np.zeros((H, W, 3)), np.zeros((H, W, 1))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ys, xs = np.arange(H) + dy * step, np.arange(W) + dx * step
                ok = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
                k = SPLINE[abs(dx)] * SPLINE[abs(dy)]
                num += k * ok[..., None] * prev[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)]
                den += k * ok[..., None]
        want = num / den
        assert np.abs(got - want).max() < 1e-12, f"iteration {i}"
