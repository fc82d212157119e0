"""Probe baking without a GPU (include/hiprz_probe.h): the nine weights of the evaluation held to a quadrature of the clamped cosine, the
float32 restatement of both terms (tests/probe_reference.py) held to the same rules in float64, its mutants told apart, the sphere table
and the trilinear Field.

THE QUADRATURE: a radiance that is a combination of the nine basis functions is a polynomial of degree 2 in the direction.  Its uniform
mean against a basis function (degree 4) is exact under Gauss-Legendre in z (32 nodes) times a uniform rule in phi (64 angles); the
cosine-weighted integral over the hemisphere of n is taken in the frame of n, cos(theta) by Gauss-Legendre on [0, 1], where the integrand is
a polynomial as well.  Both sides are exact up to float64 rounding, so they must agree to 1e-7 (the issue's figure) with room to spare.

THE FLOAT64 COMPARISON: the mean of K float32 terms summed in any order differs from the exact mean by at most K * 2^-24 * mean(|terms|)
(Higham, Accuracy and Stability, (4.4)); a term L.c * B_b itself carries at most three roundings (the products of the basis, the - 1 or
the difference, the product with L), so evaluated in float64 from the same float32 inputs it moves by at most 3 * 2^-24 of the magnitudes
involved — below the bound from K = 16 on, where K * mean(|L B_b|) is several times mean(|L|).  For the light term the sum runs over L * K
terms."""
import ctypes as C

import numpy as np
import pytest

import bake_reference as BR
import gather_reference as GR
import light_reference as LR
import probe_reference as PR
from rayzath_amd import gather, probe
from rayzath_amd.bake import point_dtype

F = np.float32
W, H = 23, 17
SKY = (0.3, 0.5, 0.9)


def _sphere_rule(nz=32, nphi=64):
    z, wz = np.polynomial.legendre.leggauss(nz)
    phi = (np.arange(nphi) + 0.5) * (2.0 * np.pi / nphi)
    r = np.sqrt(1.0 - z * z)
    d = np.stack([r[:, None] * np.cos(phi), r[:, None] * np.sin(phi), np.broadcast_to(z[:, None], (nz, nphi))], -1).reshape(-1, 3)
    w = np.repeat(wz * 0.5, nphi) / nphi                 # sums to 1: the uniform mean over the sphere
    return d, w


def _frame64(n):
    t, bt = BR.frame(np.asarray(n, np.float64))
    return t, bt


def _cosine_integral(coeff, n):
    """(1 / pi) * integral over the hemisphere of n of L(w) (n . w) dw for L = sum_b coeff[b] B_b, by quadrature in the frame of n"""
    c, wc = np.polynomial.legendre.leggauss(32)
    c, wc = 0.5 * (c + 1.0), 0.5 * wc                    # cos(theta) on [0, 1]
    phi = (np.arange(64) + 0.5) * (2.0 * np.pi / 64)
    s = np.sqrt(1.0 - c * c)
    t, bt = _frame64(n)
    local = np.stack([s[:, None] * np.cos(phi), s[:, None] * np.sin(phi), np.broadcast_to(c[:, None], (32, 64))], -1)
    d = local[..., 0:1] * t + local[..., 1:2] * bt + local[..., 2:3] * np.asarray(n, np.float64)
    L = PR.basis(d) @ coeff                              # (32, 64, 3)
    weight = (wc * c)[:, None] * (2.0 * np.pi / 64)      # dw = d(cos) dphi, times cos
    return (L * weight[..., None]).sum((0, 1)) / np.pi


def test_the_nine_weights_reproduce_the_clamped_cosine_of_a_band_limited_radiance():
    rng = np.random.default_rng(11)
    d, w = _sphere_rule()
    B = PR.basis(d)
    # the basis functions are orthogonal under the uniform mean, with the squares the weights undo: 1 / (w_b * band factor)
    gram = (B * w[:, None]).T @ B
    assert np.abs(gram - np.diag(np.diag(gram))).max() < 1e-12
    assert np.allclose(np.diag(gram), [1, 1 / 3, 1 / 3, 1 / 3, 1 / 15, 1 / 15, 4 / 5, 1 / 15, 4 / 15], rtol=0, atol=1e-12)
    for _ in range(4):
        coeff = rng.normal(size=(9, 3))
        L = B @ coeff
        sh = (B[:, :, None] * L[:, None, :] * w[:, None, None]).sum(0)           # the stored numbers: plain means of L * B_b
        for n in BR.normalized(rng.normal(size=(5, 3)).astype(F)).astype(np.float64):
            n = n / np.linalg.norm(n)
            want, got = _cosine_integral(coeff, n), PR.irradiance(sh, n)
            assert np.abs(got - want).max() < 1e-7, (got, want)
    assert PR.WEIGHTS == tuple(float(v) for v in probe.WEIGHTS), "the module's float32 weights are the header's, exactly"
    # the band factors pi, 2 pi / 3, pi / 4 times the squared SH constants, times 4 pi (a stored number is a mean, not an integral) over pi
    k2 = [1 / (4 * np.pi), 3 / (4 * np.pi), 3 / (4 * np.pi), 3 / (4 * np.pi), 15 / (4 * np.pi), 15 / (4 * np.pi), 5 / (16 * np.pi), 15 / (4 * np.pi), 15 / (16 * np.pi)]
    band = [np.pi] + [2 * np.pi / 3] * 3 + [np.pi / 4] * 5
    assert np.allclose([a * b * 4 for a, b in zip(band, k2)], PR.WEIGHTS, rtol=1e-14, atol=0)


@pytest.mark.parametrize("cosine", [1.0, 0.5, 0.0, -1.0])
def test_a_delta_light_reads_the_band_two_clamped_cosine(cosine):
    """a light of weight w from direction w0 stores P * B_b(w0), P = w * 0.25; a surface point with normal n holds w * max(0, n . w0).  The
    evaluation reads w * (1 + 2 c + (5 / 8) (3 c^2 - 1)) / 4: 1.0625 of the true value at c = 1, the known overshoot, and 0.0625 w behind"""
    rng = np.random.default_rng(5)
    for _ in range(6):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        t, bt = _frame64(n)
        s, phi = np.sqrt(max(0.0, 1.0 - cosine * cosine)), rng.uniform(0, 2 * np.pi)
        w0 = s * np.cos(phi) * t + s * np.sin(phi) * bt + cosine * n
        weight = np.array([3.0, 0.5, 1.25])
        sh = (weight * 0.25)[None, :] * PR.basis(w0)[:, None]
        want = weight * (1.0 + 2.0 * cosine + 0.625 * (3.0 * cosine * cosine - 1.0)) / 4.0
        assert np.abs(PR.irradiance(sh, n) - want).max() < 1e-12
    if cosine == 1.0:
        assert want[0] / weight[0] == 1.0625


def _inputs(K, seed=0, n=40, n_charts=20):
    """probes (two of them invalid), their rays under a three-set sphere table, samples of every kind, charts and a source with holes"""
    rng = np.random.default_rng(100 + K + seed)
    probes = np.zeros(n, point_dtype)
    probes["position"], probes["normal"] = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    probes["near"], probes["far"] = 1e-3, 1e3
    probes["normal"][5] = 0.0
    probes["far"][n - 2] = -1.0
    table = PR.sphere_table(K, 3)
    rays = BR.rays(probes, table, 9)
    kind = rng.random((n, K))
    ids = rng.integers(0, n_charts, (n, K)).astype(np.uint32)
    for code, lo in ((gather.MISS, 0.80), (gather.UNMAPPED, 0.87), (gather.BACK, 0.92), (gather.INVALID_RAY, 0.97)):
        ids[kind >= lo] = code
    bx = rng.random((n, K)).astype(F)
    by = (rng.random((n, K)).astype(F) * (F(1.0) - bx)).astype(F)
    samples = GR.make_samples(ids, bx, by, rng.random((n, K)).astype(F))
    charts = np.zeros(n_charts, gather.chart_dtype)
    for name in ("u1", "v1", "u2", "v2", "u3", "v3"):
        charts[name] = rng.random(n_charts)
    source = np.zeros((H, W), gather.record_dtype)
    source["rgb"] = rng.random((H, W, 3)) * 4.0
    source["word"][rng.random((H, W)) < 0.1] = gather.INVALID
    return probes, table, rays, samples, charts, source


@pytest.mark.parametrize("K", [16, 64, 128])
def test_the_gathered_term_lies_within_the_summation_bound_of_float64(K):
    probes, table, rays, samples, charts, source = _inputs(K)
    rec = PR.gather_records(probes, samples, rays, charts, source, W, H, SKY)
    ok = PR.valid(probes)
    assert ok.sum() == len(probes) - 2
    words = rec["sh"][..., 3].view(np.uint32)
    assert (words[~ok, 0] == probe.INVALID).all() and not rec["sh"][~ok][..., :3].view(np.uint32).any() and not words[:, 1:].any()
    values, read, missed = GR.contributions(samples, charts, source, W, H, SKY)
    assert np.array_equal(words[ok, 0] & 0xFFFF, read.sum(-1)[ok]) and np.array_equal(words[ok, 0] >> 16, missed.sum(-1)[ok])
    assert read[ok].any() and missed[ok].any() and (~read & ~missed)[ok].any()
    exact, magnitude = PR.gather_exact(samples, rays, charts, source, W, H, SKY)
    bound = K * 2.0 ** -24 * magnitude + 1e-30
    err = np.abs(rec["sh"][..., :3].astype(np.float64) - exact)
    assert (err[ok] <= bound[ok]).all(), (err[ok] / bound[ok]).max()
    # B0 = 1: the first coefficient is the gather's own mean, bit for bit
    assert rec["sh"][:, 0, :3].tobytes() == GR.texels(probes, samples, charts, source, W, H, SKY)["mean"].tobytes()


def _lights():
    spot = dict(position=np.array([1.5, 4.0, -1.0], F), direction=BR.normalized(np.array([-0.3, -1.0, 0.25], F)), size=F(0.35), cos_angle=F(np.cos(0.8)), angle=F(0.8),
                color=np.array([255, 240, 220, 255], np.uint8), emission=F(60.0))
    dim = dict(spot, position=np.array([-2.0, 3.0, 2.0], F), emission=F(0.0))
    direct = dict(direction=BR.normalized(np.array([-0.25, -1.0, 0.45], F)), cos_angular_size=F(np.cos(0.15)), color=np.array([255, 255, 240, 255], np.uint8), emission=F(4.0))
    return [spot, dim], [direct]


@pytest.mark.parametrize("K", [16, 64, 128])
def test_the_light_term_lies_within_the_summation_bound_of_float64(K):
    rng = np.random.default_rng(K)
    probes = _inputs(16)[0]
    spots, directs = _lights()
    table = LR.disk_table(K, 3)
    w3, far, w, kept = PR.light_samples(probes, spots, directs, table, 4)
    ok = PR.valid(probes)
    assert not kept[~ok].any() and not kept[:, 1].any() and kept[ok][:, 2].all() and kept[ok][:, 0].any(), "the dim light is skipped, the direct light never"
    occluded = (rng.random(w.shape) < 0.3).astype(np.uint32)
    ce = LR.colour_emission(spots, directs)
    base = np.zeros(len(probes), probe.sh_dtype)
    base["sh"][..., :3] = rng.random((len(probes), 9, 3))
    base["sh"][:, 0, 3] = np.arange(len(probes), dtype=np.uint32).view(F)
    base["sh"][3, 0, 3] = np.array([probe.INVALID], np.uint32).view(F)[0]
    rec = PR.light_records(probes, w3, w, occluded, ce, base)
    alone = PR.light_records(probes, w3, w, occluded, ce)
    words = rec["sh"][..., 3].view(np.uint32)
    good = ok.copy()
    good[3] = False
    assert (words[~good, 0] == probe.INVALID).all() and not rec["sh"][~good][..., :3].view(np.uint32).any()
    assert np.array_equal(words[good, 0], np.arange(len(probes))[good]) and np.array_equal(words[good, 1], ((occluded != 0) & (w > 0)).sum((1, 2))[good])
    assert rec["sh"][good][..., :3].tobytes() == (base["sh"][good][..., :3] + alone["sh"][good][..., :3]).tobytes(), "the sum per component"
    exact = PR.light_term(w3, w, occluded, ce, np.float64)
    adds = (w > 0) & (occluded == 0)
    terms = np.where(adds[..., None], ce.astype(np.float64)[None, :, None, :] * w.astype(np.float64)[..., None] * 0.25, 0.0)[:, :, :, None, :] * PR.basis(w3.astype(np.float64))[..., None]
    bound = 3 * K * 2.0 ** -24 * np.abs(terms).sum((1, 2)) / K + 1e-30
    err = np.abs(alone["sh"][..., :3].astype(np.float64) - exact)
    assert (err[ok] <= bound[ok]).all(), (err[ok] / bound[ok]).max()
    # against the light bake's own restatement: with the cosine put back, B0's coefficient is light_reference's texel times 0.25
    with np.errstate(all="ignore"):                      # (the invalid probes' axes)
        c = np.maximum(LR._dot(BR.normalized(probes["normal"])[:, None, None, :], w3), F(0.0))
    with_cosine = PR.light_samples(probes, spots, directs, table, 4, F, "cosine")
    lw3, lfar, lw, lkept = LR.samples(probes, spots, directs, table, 4)
    assert with_cosine[2].tobytes() == lw.tobytes() and with_cosine[0].tobytes() == lw3.tobytes(), "the sampling is the light bake's up to the cosine"
    assert (c[kept] >= 0).all()


def test_the_mutants_differ_from_the_restatement():
    probes, table, rays, samples, charts, source = _inputs(128)
    right = PR.gather_records(probes, samples, rays, charts, source, W, H, SKY)
    for mutant in ("swap", "b6", "order"):
        wrong = PR.gather_records(probes, samples, rays, charts, source, W, H, SKY, mutant)
        differs = (wrong["sh"][..., :3] != right["sh"][..., :3]).any((1, 2))
        assert differs[PR.valid(probes)].mean() > 0.9, mutant
    spots, directs = _lights()
    disk = LR.disk_table(128, 2)
    w3, far, w, kept = PR.light_samples(probes, spots, directs, disk, 1)
    occluded = np.zeros(w.shape, np.uint32)
    ce = LR.colour_emission(spots, directs)
    right = PR.light_records(probes, w3, w, occluded, ce)
    ok = PR.valid(probes)
    for mutant in ("swap", "b6", "quarter", "order"):
        wrong = PR.light_records(probes, w3, w, occluded, ce, None, mutant)
        assert (wrong["sh"][..., :3] != right["sh"][..., :3]).any((1, 2))[ok].mean() > 0.9, mutant
    quarter = PR.light_records(probes, w3, w, occluded, ce, None, "quarter")
    assert np.allclose(quarter["sh"][ok][:, 0, :3], 4.0 * right["sh"][ok][:, 0, :3], rtol=1e-5)
    cw3, cfar, cw, ckept = PR.light_samples(probes, spots, directs, disk, 1, F, "cosine")
    assert (cw[ok] < w[ok]).any() and (ckept[ok].sum() < kept[ok].sum()), "with the cosine left in, samples below the probe's axis are skipped"
    wrong = PR.light_records(probes, cw3, cw, occluded, ce)
    assert (wrong["sh"][..., :3] != right["sh"][..., :3]).any((1, 2))[ok].all()


def _passes_the_table_rule(table):
    t = np.asarray(table, F)
    sq = (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]
    return np.isfinite(t).all() and ((sq >= F(0.999)) & (sq <= F(1.001))).all()


def test_the_sphere_table(built):
    worst = {}
    for K in (16, 64, 256, 1024):
        for S in (1, 3):
            table = PR.sphere_table(K, S)
            assert table.shape == (S, K, 4) and _passes_the_table_rule(table) and not table[..., 3].any()
            assert probe.sphere_directions(K, S).tobytes() == table.tobytes(), "the library's table is the formula's"
            assert (table[..., 2] < 0).sum() == S * K // 2, "the whole sphere: half the directions look down"
        one = PR.sphere_table(K, 1)[0, :, :3].astype(np.float64)
        worst[K] = np.abs(PR.basis(one)[:, 1:].mean(0)).max()
        print(f"K = {K}: the largest |mean of B1 .. B8| over one set is {worst[K]:.2e}")
        # z is stratified (a midpoint rule, error of order 1 / K^2), phi a golden-ratio sequence (discrepancy of order log K / K): 1 / (4 K) has room
        assert worst[K] <= 0.25 / K
    assert worst[16] > worst[64] > worst[256] > worst[1024]
    with pytest.raises(ValueError):
        probe.sphere_directions(8, 1)
    with pytest.raises(ValueError):
        probe.sphere_directions(16, 65)


def test_the_vectorised_evaluation_is_the_headers(built):
    rng = np.random.default_rng(2)
    sh = np.zeros(50, probe.sh_dtype)
    sh["sh"][..., :3] = rng.normal(size=(50, 9, 3))
    sh["sh"][7, 0, 3] = np.array([probe.INVALID], np.uint32).view(F)[0]
    normals = BR.normalized(rng.normal(size=(50, 3)).astype(F))
    got = probe.irradiance(sh, normals)
    assert got.dtype == F and got.shape == (50, 3) and not got[7].view(np.uint32).any()
    lib = probe.load()
    want = np.zeros((50, 3), F)
    for i in range(50):
        lib.hiprz_probe_irradiance(sh[i:i + 1].ctypes.data, normals[i].ctypes.data, want[i].ctypes.data)
    assert got.tobytes() == want.tobytes(), "probe.irradiance and hiprz_probe_irradiance agree in every byte"
    exact = PR.irradiance(sh["sh"][..., :3], normals)
    exact[7] = 0.0
    assert np.abs(got - exact).max() < 9 * 2.0 ** -22 * np.abs(sh["sh"][..., :3]).max() * 3.75
    assert probe.irradiance(sh, normals[0]).shape == (50, 3)


def test_a_field_reproduces_its_corners_and_blends_to_the_mean_at_the_centre():
    rng = np.random.default_rng(8)
    lo, hi = (-1.0, 0.0, 2.0), (3.0, 2.0, 4.0)
    probes = probe.grid(lo, hi, (2, 2, 2))
    assert probes.dtype == point_dtype and probes.shape == (2, 2, 2)
    assert probes["position"][0, 0, 0].tolist() == list(lo) and probes["position"][1, 1, 1].tolist() == list(hi) and probes["position"][1, 0, 1].tolist() == [3.0, 0.0, 4.0]
    assert (probes["normal"] == np.array([0, 1, 0], F)).all() and (probes["near"] == F(1e-3)).all() and PR.valid(probes).all()
    sh = np.zeros((2, 2, 2), probe.sh_dtype)
    sh["sh"][..., :3] = rng.random((2, 2, 2, 9, 3))
    field = probe.Field(lo, hi, (2, 2, 2), sh)
    corners = probes["position"].reshape(-1, 3)
    assert field.blend(corners)["sh"][..., :3].tobytes() == sh["sh"].reshape(8, 9, 4)[..., :3].tobytes(), "a corner reads its own probe"
    centre = field.blend(np.array([[1.0, 1.0, 3.0]]))
    assert np.abs(centre["sh"][0, :, :3] - sh["sh"].reshape(8, 9, 4)[..., :3].mean(0)).max() < 1e-6
    n = np.array([[0.0, 0.6, 0.8]], F)
    assert field.irradiance(np.array([[1.0, 1.0, 3.0]]), n).tobytes() == probe.irradiance(centre, n).tobytes()
    # outside: clamped to the grid
    assert field.blend(np.array([[9.0, 9.0, 9.0]]))["sh"][0, :, :3].tobytes() == sh["sh"][1, 1, 1, :, :3].tobytes()
    # an invalid probe is left out and the weights renormalised: the centre is then the mean of the other seven
    sh["sh"][0, 1, 0, 0, 3] = np.array([probe.INVALID], np.uint32).view(F)[0]
    field = probe.Field(lo, hi, (2, 2, 2), sh)
    keep = np.ones(8, bool)
    keep[np.ravel_multi_index((0, 1, 0), (2, 2, 2))] = False
    centre = field.blend(np.array([[1.0, 1.0, 3.0]]))
    assert np.abs(centre["sh"][0, :, :3] - sh["sh"].reshape(8, 9, 4)[keep][..., :3].mean(0)).max() < 1e-6
    at_invalid = field.blend(probes["position"][0, 1, 0][None])
    assert at_invalid["sh"][0, 0, 3:].view(np.uint32)[0] == probe.INVALID and not probe.irradiance(at_invalid, n).any()
    line = probe.grid((0, 0, 0), (1, 0, 0), (3, 1, 1))
    assert line["position"][:, 0, 0, 0].tolist() == [0.0, 0.5, 1.0]
