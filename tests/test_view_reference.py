"""The numpy float32 restatement of the baked view (tests/view_reference.py) without a GPU: held to the same rule evaluated in float64 over
generated hits, shown to differ from each of its five mutants on these inputs — the proof that the comparisons of tests/test_view_gpu.py,
which hold the device to this restatement bit for bit, can tell a wrong reading of the header from the right one — and the boundary cap of
the GPU tests shown to hold, in float64 alone, for every camera and source they use.

THE INPUTS: tests/test_gather_reference.py's kind — 37 charts with UVs from [0, 1]^2 (three reaching outside the atlas), a 53 x 29 source
whose values differ per texel and of which one texel in nine has no value, 96 x 16 samples: front-face hits on a random chart with
barycentrics uniform over the triangle, one sample in five a miss, an unmapped hit, a back-face hit or an invalid ray.

THE FLOAT64 COMPARISON.  A float32 u differs from the float64 one by less than 5e-7 (four roundings of values below 2), so u * W by less
than W * 6e-7 < 3.2e-5 texel.  NEAREST: samples whose float64 u * W or v * H lies within 1e-4 of an integer are left out, every other texel
must agree and the RGB is then a copy.  BILINEAR: samples whose float64 gx or gy lies within 1e-4 of an integer are left out (the taps are
then the same four); the result is a weighted mean R = sum(w v) / sum(w) of at most four values, |dw/dfx| <= 1 per tap, so a shift of fx
and fy by dg moves R by at most 4 vmax (dgx + dgy) / sw, and the float32 evaluation — four products and three sums per numerator, three
sums in the denominator, one division, each within 2^-24 relative — adds at most 12 * 2^-24 * vmax."""
import numpy as np
import pytest

import field_reference as FR
import gather_reference as GR
import view_reference as VR
from rayzath_amd import bake, field, gather, probe, view
from rayzath_amd.scene import camera_struct, flatten

F = np.float32
W, H, C, N, K = 53, 29, 37, 96, 16
SKY = (0.25, 0.5, 2.0)


def _charts(rng):
    charts = np.zeros(C, gather.chart_dtype)
    for name in ("u1", "v1", "u2", "v2", "u3", "v3"):
        charts[name] = rng.uniform(0.0, 1.0, C)
    charts["u1"][:3], charts["v2"][:3] = (-0.4, 1.3, 0.5), (1.2, -0.1, 1.6)
    return charts


def _samples(rng):
    r1, r2 = rng.random((N, K)), rng.random((N, K))
    bx, by = (1.0 - np.sqrt(r1)) * r2, np.sqrt(r1) * (1.0 - r2)          # uniform over the triangle, bx + by <= 1
    idv = rng.integers(0, C, (N, K)).astype(np.uint32)
    kind = rng.integers(0, 20, (N, K))
    for code, k in ((gather.MISS, 0), (gather.UNMAPPED, 1), (gather.BACK, 2), (gather.INVALID_RAY, 3)):
        idv[kind == k] = code
    hit = (idv != gather.MISS) & (idv != gather.INVALID_RAY)
    return GR.make_samples(idv, np.where(hit, bx, 0).astype(F), np.where(hit, by, 0).astype(F), rng.uniform(0.1, 3.0, (N, K)).astype(F))


def _field(rng, shape=(3, 2, 3)):
    lo, hi = (-1.0, 0.0, 0.5), (1.0, 1.0, 2.5)
    n = int(np.prod(shape))
    probes = probe.grid(lo, hi, shape)
    sh = np.zeros(n, probe.sh_dtype)
    sh["sh"][:, 0, :3] = rng.uniform(1.0, 2.0, (n, 3))
    sh["sh"][:, 1:, :3] = rng.uniform(-0.3, 0.3, (n, 8, 3))
    vis = np.zeros(n, field.vis_dtype)
    mean = rng.uniform(0.2, 1.5, (n, 64)).astype(F)
    vis["moments"][..., 0], vis["moments"][..., 1] = mean, mean * mean + rng.uniform(0.0, 0.2, (n, 64)).astype(F)
    vis["words"][:] = (60, 1, 3, 64)
    return field.grid_of(lo, hi, shape), probes, sh, vis, field.params(bias=0.02, max_back=4)


def _surface(rng):
    origin = rng.uniform((-1.0, 0.0, 0.5), (1.0, 1.0, 2.5), (N, K, 3)).astype(F)
    direction = rng.normal(size=(N, K, 3))
    direction = (direction / np.sqrt((direction ** 2).sum(-1, keepdims=True))).astype(F)
    normal = rng.normal(size=(N, K, 3))
    normal = (normal / np.sqrt((normal ** 2).sum(-1, keepdims=True))).astype(F)
    color = (rng.integers(0, 256, (N, K, 3)).astype(F) / F(255.0)).astype(F)
    emission = np.where(rng.random((N, K)) < 0.5, rng.uniform(0.5, 3.0, (N, K)), 0.0).astype(F)
    return origin, direction, normal, color, emission


def test_nearest_against_float64():
    rng = np.random.default_rng(41)
    charts, source, samples = _charts(rng), VR.source_of(W, H), _samples(rng)
    u64, v64, mapped = GR.uv(samples, charts, np.float64)
    edge = mapped & VR.on_a_boundary(u64, v64, W, H)
    assert edge.mean() < 0.01, "the inputs: hardly a sample lies on a texel boundary"
    keep = mapped & ~edge
    rgb32, count32 = VR.atlas_taps(samples, charts, source, W, H, view.NEAREST, F)
    rgb64, count64 = VR.atlas_taps(samples, charts, source, W, H, view.NEAREST, np.float64)
    assert np.array_equal(count32[keep], count64[keep]) and np.array_equal(rgb32[keep].astype(np.float64), rgb64[keep]), "away from a boundary the nearest texel is float64's, its RGB a copy"
    assert (count32[keep] == 1).mean() > 0.8 and (count32[keep] == 0).any(), "most texels have a value, some have none"
    assert not count32[~mapped].any() and not rgb32[~mapped].any()
    # it is the gather's texel: a view pixel equals what a gather ray hitting the same place reads
    values, read, _ = GR.contributions(samples, charts, source, W, H, (0.0, 0.0, 0.0))
    assert np.array_equal(read, count32 == 1) and values[read].tobytes() == rgb32[read].tobytes()


def test_bilinear_against_float64():
    rng = np.random.default_rng(42)
    charts, source, samples = _charts(rng), VR.source_of(W, H), _samples(rng)
    u64, v64, mapped = GR.uv(samples, charts, np.float64)
    edge = mapped & VR.on_a_boundary(u64 - 0.5 / W, v64 - 0.5 / H, W, H)          # gx = u * W - 0.5 near an integer
    assert edge.mean() < 0.01
    keep = mapped & ~edge
    rgb32, count32 = VR.atlas_taps(samples, charts, source, W, H, view.BILINEAR, F)
    rgb64, count64 = VR.atlas_taps(samples, charts, source, W, H, view.BILINEAR, np.float64)
    assert np.array_equal(count32[keep], count64[keep]), "away from a boundary the taps used are float64's"
    for c in range(5):
        assert (count32[keep] == c).any(), f"no sample with {c} taps: holes and edges are not exercised"
    # sw in float64, from the counts' own rule: recomputed here over the taps that lie inside and have a value
    src = source.reshape(-1)
    gx, gy = u64 * W - 0.5, v64 * H - 0.5
    x0, y0 = np.floor(gx), np.floor(gy)
    fx, fy = gx - x0, gy - y0
    sw = np.zeros(samples.shape)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        x, y = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        has = inside & (src["word"][np.clip(y, 0, H - 1) * W + np.clip(x, 0, W - 1)] != gather.INVALID)
        sw += np.where(has, (fx if dx else 1 - fx) * (fy if dy else 1 - fy), 0.0)
    vmax = float(source["rgb"].max())
    used = keep & (count64 > 0)
    bound = 4 * vmax * (W * 6e-7 + H * 6e-7) / np.maximum(sw, 1e-300) + 12 * 2.0 ** -24 * vmax
    err = np.abs(rgb32.astype(np.float64) - rgb64).max(-1)
    assert (err[used] <= bound[used]).all(), f"{(err[used] / bound[used]).max():.3f} of the bound"
    assert np.median(bound[used]) < 1e-3, "the bound means something on most samples"
    # a source of 1.0 everywhere: acc and sw take the same sums, the quotient is exactly 1
    ones = VR.source_of(W, H)
    ones["rgb"] = 1.0
    rgb, count = VR.atlas_taps(samples, charts, ones, W, H, view.BILINEAR, F)
    assert (rgb[count > 0] == 1.0).all() and not rgb[count == 0].any()


def test_the_record_and_its_kinds():
    rng = np.random.default_rng(43)
    charts, source, samples = _charts(rng), VR.source_of(W, H), _samples(rng)
    fld, surface = _field(rng), _surface(rng)
    for filter in (view.NEAREST, view.BILINEAR):
        plain = VR.pixels(samples, charts, source, W, H, SKY, filter)
        full = VR.pixels(samples, charts, source, W, H, SKY, filter, *surface, field=fld)
        kinds, full_kinds = view.kind(plain), view.kind(full)
        missed = (samples["id"] == gather.MISS) | (samples["id"] == gather.INVALID_RAY)
        assert (kinds[missed] == view.SKY).all() and (plain["rgb"][missed] == np.asarray(SKY, F)).all() and not view.count(plain)[missed].any()
        back = samples["id"] == gather.BACK
        assert (kinds[back] == view.BACK).all() and not plain["rgb"][back].view(np.uint32).any()
        unmapped = samples["id"] == gather.UNMAPPED
        assert (kinds[unmapped] == view.NONE).all() and not plain["rgb"][unmapped].view(np.uint32).any(), "without a field an unmapped hit reads NONE"
        assert (full_kinds[unmapped] == view.FIELD).all() and (view.count(full)[unmapped] >= 1).all() and (view.count(full)[unmapped] <= 8).all()
        assert plain[~unmapped].tobytes() == full[~unmapped].tobytes(), "a field changes no other pixel"
        atlas = kinds == view.ATLAS
        assert atlas.mean() > 0.6 and (view.count(plain)[atlas] >= 1).all() and (view.count(plain)[atlas] <= (1 if filter == view.NEAREST else 4)).all()
        none = (kinds == view.NONE) & ~unmapped
        assert none.any() and not plain["rgb"][none].view(np.uint32).any() and not view.count(plain)[none].any()
        # the field's value is lookup's, times the colour, plus colour x emission where there is any
        origin, direction, normal, color, emission = surface
        points = bake.points(VR.hit_points(origin, direction, samples["t"])[unmapped], normal[unmapped])
        E = FR.lookup(*fld[:4], fld[4], points)["rgb"]
        want = color[unmapped] * E
        want = np.where((emission[unmapped] > 0)[:, None], want + color[unmapped] * emission[unmapped][:, None], want).astype(F)
        assert full["rgb"][unmapped].tobytes() == want.tobytes()
        image = VR.image_of(full)
        assert image[..., :3].tobytes() == full["rgb"].tobytes() and (image[..., 3] == 1.0).all()


def test_every_mutant_differs_on_these_inputs():
    rng = np.random.default_rng(44)
    charts, source, samples = _charts(rng), VR.source_of(W, H), _samples(rng)
    fld, surface = _field(rng), _surface(rng)
    right = VR.pixels(samples, charts, source, W, H, SKY, view.BILINEAR, *surface, field=fld)
    atlas = view.kind(right) == view.ATLAS
    unmapped = samples["id"] == gather.UNMAPPED
    for mutant in VR.MUTANTS:
        wrong = VR.pixels(samples, charts, source, W, H, SKY, view.BILINEAR, *surface, field=fld, mutant=mutant)
        differs = wrong.view(np.uint32).reshape(N, K, 4) != right.view(np.uint32).reshape(N, K, 4)
        where = atlas if mutant in VR.ATLAS_MUTANTS else (unmapped & (surface[4] > 0) if mutant == "noemission" else unmapped)      # (only an emitter has the term)
        share = differs.any(-1)[where].mean()
        print(f"{mutant}: {share:.1%} of the {'atlas' if mutant in VR.ATLAS_MUTANTS else 'field'} pixels differ")
        assert share > (0.05 if mutant == "zero" else 0.4), f"{mutant}: only {share:.1%} differ"
        if mutant in VR.FIELD_MUTANTS:
            assert not differs.any(-1)[~unmapped].any(), f"{mutant} is a mutant of the field branch alone"
    # the nearest filter has no -0.5 and no weights: its only mutant here is the swap
    near = VR.pixels(samples, charts, source, W, H, SKY, view.NEAREST)
    assert VR.pixels(samples, charts, source, W, H, SKY, view.NEAREST, mutant="nohalf").tobytes() == near.tobytes()


def test_the_boundary_cap_of_the_gpu_tests_holds_in_float64():
    """tests/test_view_gpu.py leaves out of its texel comparison the pixels whose float64 UV lies within 1e-4 texel of a texel boundary, at
    most 1 % of the mapped pixels of a camera.  That the cameras of view_reference.cameras() and both sources allow this is shown here
    without a device: tests/query_reference.py's pixel rays walked in float64 over the world's 64 triangles, for the world as it is and
    with the cube moved."""
    import gather_world as GW
    for moved in (False, True):
        w = GW.world(moved=moved)
        flat = flatten(w)
        base, charts = gather.chart_tables(GW.parts(w), len(flat.instances))
        for cam in VR.cameras():
            cs = camera_struct(cam)
            mapped, u, v, inst, front = VR.float64_uv(w, flat, cs, base, charts)
            for SW, SH in VR.SOURCES:
                edge = mapped & (VR.on_a_boundary(u, v, SW, SH) | VR.on_a_boundary(u - 0.5 / SW, v - 0.5 / SH, SW, SH))
                share = edge.sum() / max(int(mapped.sum()), 1)
                print(f"moved {moved} camera {cs.width} x {cs.height} source {SW} x {SH}: {int(mapped.sum())} mapped pixels, {int(edge.sum())} on a boundary ({share:.3%})")
                assert share <= VR.CAP
            if cs.width > 1:
                assert mapped.mean() > 0.3 and ((inst == GW.SPHERE) & front).sum() >= 3 and (inst < 0).any(), "the camera sees the atlas, the sphere and the sky"
