"""numpy restatement of include/hiprz.h "VARIANCE" (batch moments of the accumulator and the estimate they give) and of "THE
VARIANCE-GUIDED FILTER", in the header's order of operations, evaluated in the floating-point type `dtype`: float32 restates what the
device computes, float64 is the reference both are compared with.  Helper of tests/test_variance_gpu.py; its own unit tests are in
tests/test_variance_abi.py."""
import numpy as np

import denoise_reference as ref
from rayzath_amd import _abi

LUM = (0.2126, 0.7152, 0.0722)


class Moments:
    """snap, m0 = (S2_r, S2_g, S2_b, SA), m1 = (S1_r, S1_g, S1_b, K) of a frame; close(accum) is what rz_moments_kernel does after a render
    call that left `accum` (hiprz_read_accum, float32) behind."""

    def __init__(self, shape, dtype=np.float64):
        self.T = dtype
        self.snap, self.m0, self.m1 = (np.zeros(tuple(shape) + (4,), dtype) for _ in range(3))

    def close(self, accum):
        T = self.T
        a = np.asarray(accum, np.float32).astype(T)
        d = (a - self.snap).astype(T)
        closes = d[..., 3] >= 1
        w = d[..., 3:4]
        m0 = self.m0 + np.concatenate([d[..., :3] * d[..., :3], w * w], axis=-1)
        m1 = self.m1 + np.concatenate([d[..., :3] * w, np.ones_like(w)], axis=-1)
        self.m0 = np.where(closes[..., None], m0, self.m0).astype(T)
        self.m1 = np.where(closes[..., None], m1, self.m1).astype(T)
        self.snap = np.where(closes[..., None], a, self.snap).astype(T)
        return self

    def restart_from_history(self, accum):
        """the call carried reprojected history over: the moments start from zero and only snap = accum"""
        self.__init__(self.snap.shape[:-1], self.T)
        self.snap = np.asarray(accum, np.float32).astype(self.T)
        return self


def estimate(accum, m0, m1, dtype=np.float64):
    """(V_r, V_g, V_b, K) of hiprz_read_variance from the accumulator image and the moments"""
    T = dtype
    a, m0, m1 = np.asarray(accum).astype(T), np.asarray(m0).astype(T), np.asarray(m1).astype(T)
    K, A = m1[..., 3:4], a[..., 3:4]
    out = np.zeros(a.shape, T)
    out[..., 3] = K[..., 0]
    with np.errstate(all="ignore"):
        r = a[..., :3] / A
        E = np.maximum(T(0), (m0[..., :3] - (T(2) * r) * m1[..., :3]) + (r * r) * m0[..., 3:4])
        V = (E * (K / (K - T(1)))) / (A * A)
    out[..., :3] = np.where(K >= 2, V, T(0))
    return out


def sum_parts(parts, dtype=np.float64):
    """HIPRZ_SHARD_SAMPLES: images of the parts added in part order"""
    total = np.asarray(parts[0]).astype(dtype)
    for p in parts[1:]:
        total = (total + np.asarray(p).astype(dtype)).astype(dtype)
    return total


def lum(c, T):
    return (T(np.float32(LUM[0])) * c[..., 0] + T(np.float32(LUM[1])) * c[..., 1]) + T(np.float32(LUM[2])) * c[..., 2]


def params(iterations=5, sigma_normal=128.0, sigma_depth=0.1, sigma_color=4.0, demodulate=True):
    p = ref.params(iterations, sigma_normal, sigma_depth, sigma_color, demodulate)
    p.flags |= _abi.DENOISE_VARIANCE
    return p


def atrous_variance(accum, guides, variance, p, dtype=np.float64):
    """accum (H, W, 4) float32 accumulator image, guides (H, W) of _abi.guide_dtype, variance (H, W, 4) float32 (V_r, V_g, V_b, K)
    -> (H, W, 4) in `dtype`"""
    T = dtype
    H, W = accum.shape[:2]
    acc = accum.astype(T)
    count = np.where(acc[..., 3:4] == 0, T(1), acc[..., 3:4])
    c = acc[..., :3] / count
    demodulate = bool(p.flags & _abi.DENOISE_DEMODULATE)
    albedo = np.maximum(guides["albedo"].astype(T), T(np.float32(0.01)))
    var = np.asarray(variance, np.float32).astype(T)
    sd = np.sqrt(var[..., :3])
    if demodulate:
        c = c / albedo
        sd = sd / albedo
    sd_l = lum(sd, T)
    v = np.where(var[..., 3] >= 2, sd_l * sd_l, T(-1)).astype(T)
    normal, z, inst = guides["normal"].astype(T), guides["depth"].astype(T), guides["instance"]
    depth_scale = T(np.float32(p.sigma_depth)) * z + T(np.float32(1.0e-6))
    sigma_normal, sigma_l = T(np.float32(p.sigma_normal)), T(np.float32(p.sigma_color))
    for i in range(p.iterations):
        s = 1 << i
        l = lum(c, T)
        known = v >= 0

        def taps():
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    y0, y1, x0, x1 = max(0, -dy * s), H - max(0, dy * s), max(0, -dx * s), W - max(0, dx * s)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    yield (dx, dy, T(ref.SPLINE[abs(dx)] * ref.SPLINE[abs(dy)]), (slice(y0, y1), slice(x0, x1)),
                           (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s)))

        gv, gk = np.zeros((H, W), T), np.zeros((H, W), T)
        for dx, dy, spline, P, Q in taps():
            use = (inst[P] == inst[Q]) & known[Q]
            gv[P] += np.where(use, spline * v[Q], T(0))
            gk[P] += np.where(use, spline, T(0))
        with np.errstate(all="ignore"):
            lum_scale = (sigma_l * np.sqrt(gv / gk) + T(np.float32(1.0e-10))).astype(T)
        sum_c, sum_w, sum_v = np.zeros((H, W, 3), T), np.zeros((H, W), T), np.zeros((H, W), T)
        for dx, dy, spline, P, Q in taps():
            if dx == 0 and dy == 0:
                sum_c += spline * c
                sum_w += spline
                sum_v += (spline * spline) * np.maximum(v, T(0))
                continue
            nP, nQ = normal[P], normal[Q]
            dot = nP[..., 0] * nQ[..., 0] + nP[..., 1] * nQ[..., 1] + nP[..., 2] * nQ[..., 2]
            with np.errstate(all="ignore"):
                w = spline * np.power(np.maximum(T(0), dot), sigma_normal)
                w = w * np.exp(-(np.abs(z[P] - z[Q]) / depth_scale[P]))
                w = np.where(inst[P] == _abi.GUIDE_MISS, spline, w)  # between two misses w_n = w_z = 1
                w_l = np.exp(-(np.abs(l[P] - l[Q]) / lum_scale[P]))
                w = np.where(known[P], w * w_l, w)
            w = np.where(inst[P] == inst[Q], w, T(0)).astype(T)
            sum_c[P] += w[..., None] * c[Q]
            sum_w[P] += w
            sum_v[P] += (w * w) * np.maximum(v[Q], T(0))
        c = sum_c / sum_w[..., None]
        v = np.where(known, sum_v / (sum_w * sum_w), T(-1)).astype(T)
    out = np.ones((H, W, 4), T)
    out[..., :3] = c * albedo if demodulate else c
    return out
