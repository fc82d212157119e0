"""The numpy float32 restatement of bounce baking (tests/gather_reference.py) without a GPU: held to the same rules evaluated in float64 over
generated hits, and shown to differ from each of its four mutants on these inputs — the proof that the comparisons of
tests/test_gather_gpu.py, which hold the device to this restatement bit for bit, can tell a wrong reading of the header from the right one.

THE INPUTS: 37 charts with UVs drawn from [0, 1]^2 (three of them reaching outside the atlas: the clamp), a 53 x 29 source whose values
differ per texel and of which one texel in eleven has no value, n = 96 points of K = 16, 64 and 128 samples: front-face hits on a random
chart with barycentrics drawn uniformly from the triangle, and one sample in five a miss, an unmapped hit, a back-face hit or an invalid ray.

THE FLOAT64 COMPARISON: a float32 u differs from the float64 one by at most 4 roundings of values below 2 in magnitude, 4 * 2^-24 * 2 < 5e-7,
so u * W by less than 53 * 5e-7 + 2^-24 * 53 < 3e-5 texel: samples whose float64 u * W or v * H lies within 1e-4 of an integer are left out
of the texel comparison (and their number is bounded), every other texel must agree.  The mean of K float32 values summed in any order
differs from the exact mean by at most K * 2^-24 * mean(|values|) (Higham, Accuracy and Stability, (4.4), and one more rounding for the
product with 1 / K)."""
import numpy as np
import pytest

import gather_reference as GR
from rayzath_amd import bake, gather
from rayzath_amd.query import HIT_EXTERNAL, HIT_FOUND, HIT_INVALID

F = np.float32
W, H, C, N = 53, 29, 37, 96
SKY = (0.25, 0.5, 2.0)


def _charts(rng):
    charts = np.zeros(C, gather.chart_dtype)
    for name in ("u1", "v1", "u2", "v2", "u3", "v3"):
        charts[name] = rng.uniform(0.0, 1.0, C)
    charts["u1"][:3], charts["v2"][:3] = (-0.4, 1.3, 0.5), (1.2, -0.1, 1.6)
    return charts


def _source(rng):
    source = np.zeros((H, W), gather.record_dtype)
    source["rgb"] = rng.uniform(0.0, 4.0, (H, W, 3))
    source["word"] = rng.integers(0, 100, (H, W))
    source["word"][rng.random((H, W)) < 1.0 / 11.0] = gather.INVALID
    return source


def _samples(rng, K):
    r1, r2 = rng.random((N, K)), rng.random((N, K))
    bx, by = (1.0 - np.sqrt(r1)) * r2, np.sqrt(r1) * (1.0 - r2)          # uniform over the triangle, bx + by <= 1
    idv = rng.integers(0, C, (N, K)).astype(np.uint32)
    kind = rng.integers(0, 20, (N, K))
    for code, k in ((gather.MISS, 0), (gather.UNMAPPED, 1), (gather.BACK, 2), (gather.INVALID_RAY, 3)):
        idv[kind == k] = code
    hit = idv != gather.MISS
    hit &= idv != gather.INVALID_RAY
    return GR.make_samples(idv, np.where(hit, bx, 0).astype(F), np.where(hit, by, 0).astype(F), rng.uniform(0.1, 9.0, (N, K)).astype(F))


def _points(rng):
    points = bake.points(rng.uniform(-1, 1, (N, 3)), rng.normal(size=(N, 3)), 1e-3, 1e3)
    points["normal"][7] = 0.0                    # two invalid points
    points["far"][N - 1] = np.nan
    return points


@pytest.mark.parametrize("K", (16, 64, 128))
def test_the_restatement_against_float64(K):
    rng = np.random.default_rng(2027 + K)
    charts, source, samples, points = _charts(rng), _source(rng), _samples(rng, K), _points(rng)
    u32, v32, mapped = GR.uv(samples, charts, F)
    u64, v64, mapped64 = GR.uv(samples, charts, np.float64)
    assert np.array_equal(mapped, mapped64) and mapped.mean() > 0.7
    assert np.abs(u32 - u64)[mapped].max() < 5e-7 and np.abs(v32 - v64)[mapped].max() < 5e-7
    x32, y32, _ = GR.texel_of(u32, v32, W, H)
    x64, y64, _ = GR.texel_of(u64, v64, W, H)
    near = lambda a: np.abs(a - np.rint(a)) < 1e-4
    edge = mapped & (near(u64 * W) | near(v64 * H))
    assert edge.mean() < 0.01, "the inputs: hardly a sample lies on a texel boundary"
    keep = mapped & ~edge
    assert np.array_equal(x32[keep], x64[keep]) and np.array_equal(y32[keep], y64[keep])
    assert (x32 == 0).any() and (x32 == W - 1).any() and x32.min() >= 0 and x32.max() <= W - 1 and y32.max() <= H - 1, "the clamp is exercised"
    # the contributions and the mean
    values, read, missed = GR.contributions(samples, charts, source, W, H, SKY)
    flat = source.reshape(-1)
    want = np.zeros((N, K, 3))
    at = keep & (flat["word"][y64 * W + x64] != gather.INVALID)
    want[at] = flat["rgb"][(y64 * W + x64)[at]]
    is_miss = (samples["id"] == gather.MISS) | (samples["id"] == gather.INVALID_RAY)
    want[is_miss] = SKY
    assert np.array_equal(values[keep | ~mapped].astype(np.float64), want[keep | ~mapped]), "a contribution is a copy: the texel's RGB, the sky or +0"
    assert np.array_equal(missed, is_miss) and np.array_equal(read[keep], at[keep]) and not read[~mapped].any()
    assert not values[(samples["id"] == gather.BACK) | (samples["id"] == gather.UNMAPPED)].any()
    texels = GR.texels(points, samples, charts, source, W, H, SKY)
    ok = np.ones(N, bool)
    ok[[7, N - 1]] = False
    assert (texels["counts"][~ok] == gather.INVALID).all() and (texels["mean"][~ok].view(np.uint32) == 0).all()
    assert np.array_equal(texels["counts"][ok] & 0xFFFF, read.sum(-1)[ok]) and np.array_equal(texels["counts"][ok] >> 16, missed.sum(-1)[ok])
    exact = values.astype(np.float64).mean(1)
    bound = K * 2.0 ** -24 * np.abs(values).astype(np.float64).mean(1) + 1e-30
    assert (np.abs(texels["mean"] - exact)[ok] <= bound[ok]).all(), "the fixed-order float32 mean lies within the summation bound of the exact mean"


def test_ids_from_hits():
    base = np.array([0, gather.NONE, 12, 40], np.uint32)
    flags = np.array([HIT_FOUND | HIT_EXTERNAL, HIT_FOUND, 0, HIT_INVALID, HIT_FOUND | HIT_EXTERNAL, HIT_FOUND | HIT_EXTERNAL, HIT_FOUND | HIT_EXTERNAL, HIT_FOUND], np.uint32)
    instance = np.array([0, 0, -1, -1, 1, 2, 3, 1], np.int32)
    source_index = np.array([5, 5, 0, 0, 2, 7, 3, 2], np.uint32)
    got = GR.ids(flags, instance, source_index, base, 42)
    assert got.tolist() == [5, gather.BACK, gather.MISS, gather.INVALID_RAY, gather.UNMAPPED, 19, gather.UNMAPPED, gather.BACK]
    assert GR.ids(flags, instance, source_index, base, 44).tolist()[6] == 43
    back = GR.ids(flags, instance, source_index, base, 42, mutant="back")
    assert back.tolist() == [5, 5, gather.MISS, gather.INVALID_RAY, gather.UNMAPPED, 19, gather.UNMAPPED, gather.UNMAPPED]
    assert GR.ids(flags[:4], instance[:4], source_index[:4], np.zeros(0, np.uint32), 0).tolist() == [gather.UNMAPPED, gather.BACK, gather.MISS, gather.INVALID_RAY]


def test_every_mutant_differs_on_these_inputs():
    rng = np.random.default_rng(5)
    K = 64
    charts, source, samples, points = _charts(rng), _source(rng), _samples(rng, K), _points(rng)
    right = GR.texels(points, samples, charts, source, W, H, SKY)
    for mutant in ("swap", "rint", "order"):
        wrong = GR.texels(points, samples, charts, source, W, H, SKY, mutant)
        differs = (wrong["mean"].view(np.uint32) != right["mean"].view(np.uint32)).any(-1)
        assert differs.sum() > N // 2, f"{mutant}: only {int(differs.sum())} of {N} texels differ"
        assert (wrong["counts"][[7, N - 1]] == gather.INVALID).all()
    assert np.array_equal(GR.texels(points, samples, charts, source, W, H, SKY, "order")["counts"], right["counts"]), "the order of the sum changes no count"
    # `back` is a mutant of the ids: over hits of which some are back-face hits it differs, and a sample that keeps its id contributes
    flags = np.where(rng.random((N, K)) < 0.3, HIT_FOUND, HIT_FOUND | HIT_EXTERNAL).astype(np.uint32)
    instance, source_index = np.zeros((N, K), np.int32), rng.integers(0, C, (N, K)).astype(np.uint32)
    base = np.zeros(1, np.uint32)
    good, bad = GR.ids(flags, instance, source_index, base, C), GR.ids(flags, instance, source_index, base, C, "back")
    assert (good != bad).mean() > 0.2 and ((good == gather.BACK) == ((flags & HIT_EXTERNAL) == 0)).all()
    as_good = GR.make_samples(good, samples["bx"], samples["by"], samples["t"])
    as_bad = GR.make_samples(bad, samples["bx"], samples["by"], samples["t"])
    a, b = GR.texels(points, as_good, charts, source, W, H, SKY), GR.texels(points, as_bad, charts, source, W, H, SKY)
    assert (a["mean"][0] != b["mean"][0]).any() and ((b["counts"] & 0xFFFF)[:7] > (a["counts"] & 0xFFFF)[:7]).all()


def test_compose():
    rng = np.random.default_rng(9)
    shape = (5, 7)
    direct, indirect, albedo, emission = (np.zeros(shape, gather.record_dtype) for _ in range(4))
    for a in (direct, indirect, albedo, emission):
        a["rgb"], a["word"] = rng.uniform(0, 3, shape + (3,)), rng.integers(0, 2**32, shape)
    direct["word"][0, 0] = gather.INVALID
    out = GR.compose(direct, indirect, albedo, emission)
    want = albedo["rgb"].astype(np.float64) * (direct["rgb"].astype(np.float64) + indirect["rgb"]) + emission["rgb"]
    assert np.abs(out["rgb"] - want).max() <= 3 * 2.0 ** -24 * np.abs(want).max() and np.array_equal(out["word"], direct["word"])
    assert out["rgb"].tobytes() == ((albedo["rgb"] * (direct["rgb"] + indirect["rgb"])) + emission["rgb"]).astype(F).tobytes()
    none = GR.compose(direct, None, albedo, None)
    assert none["rgb"].tobytes() == (albedo["rgb"] * direct["rgb"]).tobytes() and np.array_equal(none["word"], direct["word"])
    zero = np.zeros(shape, gather.record_dtype)
    assert not GR.compose(direct, indirect, zero, None)["rgb"].view(np.uint32).any(), "a zero albedo and no emission: +0"


def test_the_boundary_cap_of_the_gpu_tests_world_holds_in_float64():
    """tests/test_gather_gpu.py leaves out of its barycentrics case the rays whose float64 UV lies within 1e-3 texel of a texel boundary, at
    most 1 % of them.  That the atlas size and the rectangles of tests/gather_world.py allow this is shown here without a device: the
    hemisphere rays (tests/bake_reference.py, K = 64, three sets) of a 32 x 24 grid of floor points and of a 16 x 12 grid of points on
    the wall's front, walked in float64 over the world's 64 triangles.  Measured: 7.7 % of the floor's 49 152 rays and 50 % of the
    wall's 12 288 land on a chart (the floor sees mostly sky); of those 0.34 % and 0.60 % lie on a boundary (the cube's faces in cells of their own); 2.5 % of the floor's rays hit
    a back face (the wall's)."""
    import bake_reference as BR
    import gather_world as GW
    from rayzath_amd.scene import flatten
    w = GW.world()
    flat = flatten(w)
    triangles = GW.world_triangles(w, flat)
    assert [len(t) for t in triangles] == [2, 12, 48, 2]
    base, charts = gather.chart_tables(GW.parts(w), len(flat.instances))
    assert base.tolist() == [0, 2, gather.NONE, 14] and len(charts) == 16
    gx, gz = np.meshgrid(np.linspace(-3.0, 3.0, 32), np.linspace(-3.0, 3.0, 24))
    floor = bake.points(np.stack([gx.ravel(), np.zeros(gx.size), gz.ravel()], -1), (0.0, 1.0, 0.0), 1e-3, 1e3)
    gx, gy = np.meshgrid(np.linspace(-1.9, -0.1, 16), np.linspace(0.15, 1.35, 12))
    wall = bake.points(np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 1.0 - 1e-3)], -1), (0.0, 0.0, -1.0), 1e-3, 1e3)
    for name, points in (("floor", floor), ("wall", wall)):
        rays = BR.rays(points, BR.cosine_table(64, 3), 7).reshape(-1)
        inst, tri, bx, by, front = GW.closest_hits(triangles, rays["origin"].astype(np.float64), rays["direction"].astype(np.float64), 1e-3)
        mapped = (inst >= 0) & front & (base[np.maximum(inst, 0)] != gather.NONE)
        c = charts[(base[np.maximum(inst, 0)] + tri)[mapped]]
        b1 = (1.0 - bx[mapped]) - by[mapped]
        u = c["u1"] * b1 + c["u2"] * bx[mapped] + c["u3"] * by[mapped]
        v = c["v1"] * b1 + c["v2"] * bx[mapped] + c["v3"] * by[mapped]
        edge = GW.on_a_boundary(u, v, 1e-3)
        print(f"{name}: {mapped.mean():.2%} of {len(rays)} rays land on a chart, {edge.mean():.3%} of those within 1e-3 texel of a boundary; back-face hits {((inst >= 0) & ~front).mean():.2%}")
        assert mapped.sum() > 2000 and edge.mean() <= 0.01
        assert u.min() >= 0.03 - 1e-6 and u.max() <= 0.97 + 1e-6, "a hit's UV lies in its instance's rectangle"
