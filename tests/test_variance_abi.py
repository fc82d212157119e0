"""The variance estimate and the variance-guided filter at the C-ABI level, without a GPU: the entry points are exported and bound, the
flag has the header's value and does not touch the parameter record, every call refuses a null context — and the numpy restatement
(tests/variance_reference.py) behaves as the header's formulas say on inputs whose answer is known in closed form."""
import ctypes as C
import os
import re

import numpy as np

import denoise_reference as ref
import variance_reference as vref
from rayzath_amd import _abi, _lib
from rayzath_amd.engine import Context, Engine, denoise_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hiprz_set_variance", "hiprz_read_variance", "hiprz_variance_device", "hiprz_denoise_image_variance")


def test_the_entry_points_are_exported_and_bound(built):
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _abi.ENTRY_POINTS, name
    for name in ("set_variance", "read_variance", "variance_device", "denoise_image_variance"):
        assert callable(getattr(Context, name)), name
    assert callable(Engine.set_denoise)


def test_the_flag_has_the_headers_value_and_the_record_is_unchanged(built):
    header = open(os.path.join(ROOT, "include", "hiprz.h")).read()
    assert int(re.search(r"#define\s+HIPRZ_DENOISE_VARIANCE\s+(\d+)u", header).group(1)) == _abi.DENOISE_VARIANCE == 2
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\(", header), f"{name} is not declared in include/hiprz.h"
    out = (C.c_uint32 * 4)()
    _lib.load().hiprz_denoise_layout(out)
    assert out[1] == C.sizeof(_abi.DenoiseParams) == 20
    p = denoise_params()
    assert p.flags == _abi.DENOISE_DEMODULATE, "the defaults carry the variance flag"
    q = denoise_params(variance=True, sigma_color=4.0)
    assert q.flags == _abi.DENOISE_DEMODULATE | _abi.DENOISE_VARIANCE and q.sigma_color == 4.0 and q.iterations == p.iterations
    assert denoise_params(variance=True, demodulate=False).flags == _abi.DENOISE_VARIANCE
    assert denoise_params(variance=False).flags == p.flags


def test_calls_on_a_null_context_fail_cleanly(built):
    lib = _lib.load()
    p = denoise_params(variance=True)
    buf = (C.c_uint8 * 64)()
    ptr = C.c_void_p()
    assert lib.hiprz_set_variance(None, 1) == _abi.ERR_INVALID
    assert lib.hiprz_read_variance(None, buf, 64) == _abi.ERR_INVALID
    assert lib.hiprz_variance_device(None, C.byref(ptr)) == _abi.ERR_INVALID and not ptr
    assert lib.hiprz_denoise_image_variance(None, buf, None, buf, C.byref(p), buf, None) == _abi.ERR_INVALID
    assert lib.hiprz_set_denoise(None, C.byref(p)) == _abi.ERR_INVALID


# --- the restatement itself ------------------------------------------------------------------------------------------------------
def test_moments_of_known_batches_give_the_textbook_variance_of_the_mean():
    """one finished path per batch (A_k = 1): V is the sample variance of the batch radiances divided by K"""
    rng = np.random.default_rng(1)
    K, H, W = 7, 3, 5
    x = rng.gamma(2.0, 1.0, (K, H, W, 3)).astype(np.float32)
    accum = np.zeros((H, W, 4), np.float32)
    m = vref.Moments((H, W))
    for k in range(K):
        accum = accum + np.concatenate([x[k], np.ones((H, W, 1), np.float32)], axis=-1)
        m.close(accum)
    got = vref.estimate(accum, m.m0, m.m1)
    assert np.all(got[..., 3] == K)
    want = x.astype(np.float64).var(axis=0, ddof=1) / K  # (the moments see differences of the float32 accumulator: 1e-7 relative of x)
    assert np.abs(got[..., :3] - want).max() < 1e-5 * want.max()


def test_a_batch_without_a_finished_path_merges_into_the_next_one():
    accum = np.zeros((1, 2, 4), np.float32)
    m = vref.Moments((1, 2))
    steps = [((1.0, 0.0), (0.5, 1.0)), ((2.0, 1.0), (0.5, 1.0)), ((0.5, 0.0), (1.5, 1.0)), ((0.5, 2.0), (0.5, 1.0))]
    for (r0, a0), (r1, a1) in steps:
        accum = accum + np.array([[[r0, r0, r0, a0], [r1, r1, r1, a1]]], np.float32)
        m.close(accum)
    assert m.m1[0, 0, 3] == 2 and m.m1[0, 1, 3] == 4  # pixel 0 closed (3.0, 1) and (1.0, 2): its first and third calls merged forward
    assert m.m0[0, 0, 0] == 3.0 ** 2 + 1.0 ** 2 and m.m0[0, 0, 3] == 1 + 4 and m.m1[0, 0, 0] == 3.0 * 1 + 1.0 * 2
    v = vref.estimate(accum, m.m0, m.m1)
    r = 4.0 / 3.0
    assert abs(v[0, 0, 0] - ((3.0 - r) ** 2 + (1.0 - 2 * r) ** 2) * 2 / 9) < 1e-12
    one = vref.Moments((1, 2)).close(accum)
    assert np.all(vref.estimate(accum, one.m0, one.m1)[..., :3] == 0) and np.all(one.m1[..., 3] == 1)


def test_with_no_estimate_anywhere_the_flagged_filter_is_the_plain_filter_without_its_colour_term():
    H, W = 30, 41
    rng = np.random.default_rng(9)
    accum = np.ones((H, W, 4), np.float32)
    accum[..., :3] = rng.uniform(0.0, 2.0, (H, W, 3))
    guides = ref.make_guides(H, W, albedo=(0.5, 0.8, 0.3))
    guides["instance"][:, W // 2:] = 3
    variance = np.zeros((H, W, 4), np.float32)
    variance[..., 3] = 1  # K = 1: no estimate
    got = vref.atrous_variance(accum, guides, variance, vref.params(iterations=3))
    want = ref.atrous(accum, guides, ref.params(iterations=3, sigma_color=0.0), 0.02, 1.0 / 60.0)
    assert np.abs(got - want).max() < 1e-13


def test_the_luminance_stop_keeps_an_edge_that_exceeds_the_noise_and_smooths_what_does_not():
    H, W = 32, 48
    rng = np.random.default_rng(4)
    sigma = 0.05
    accum = np.ones((H, W, 4), np.float32)
    level = np.where(np.arange(W) < W // 2, 1.0, 3.0)[None, :, None]
    accum[..., :3] = level + rng.normal(0.0, sigma, (H, W, 1))
    guides = ref.make_guides(H, W)
    variance = np.full((H, W, 4), sigma * sigma, np.float32)
    variance[..., 3] = 8
    out = vref.atrous_variance(accum, guides, variance, vref.params(sigma_color=4.0, demodulate=False))
    for half, value in ((slice(0, W // 2), 1.0), (slice(W // 2, W), 3.0)):
        assert np.abs(out[:, half, :3] - value).max() < 4 * sigma, "the edge leaked"
        assert out[:, half, 0].std() < 0.4 * sigma, "the noise was not smoothed"
    assert np.all(out[..., 3] == 1)
