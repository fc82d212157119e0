"""What the bake pipeline's rules add up to, held to the path tracer: the world, the traced side and the float64 side of
tests/test_bake_meaning.py (CPU) and tests/test_bake_meaning_gpu.py.  The claim under "THE MEANING" in include/hiprz_light.h and
include/hiprz_gather.h is that a baked view shows, at a pixel, surface colour x the light the tracer collects at that pixel's surface point.

THE WORLD (world()) is tests/gather_world.py's geometry made matte: every material of ior 1.0 (Fresnel 0, so brdf_color is the colour and
every bounce is the cosine-sampled diffuse one), roughness 1, metalness 0, opaque, the sphere black — it is outside the atlas, the gather
counts an unmapped hit as +0, and a black sphere makes the tracer agree while it still casts shadows.  The lights are small (a spot of size
0.05 and a direct light of angular size 0.02) so that the tracer's unnormalised weight Lw = 1 / (1 + solid angle x pdf) is 1 to 1e-3 (bias()).
The world material has a colour and an emission: the sky, colour / 255 x emission on both sides.  Camera 64 x 48, atlas 128 x 96.

THE TRACED SIDE (first_path) keeps of every pixel the first finished path alone: pass 0 casts the pixel-centre ray (generate_simple_ray),
the ray the view casts, and a path that finishes is followed by one through the lens and an antialiasing offset, which this discards.

THE FLOAT64 SIDE (direct64, bounce64) is the light at each pixel's own first-hit point: tests/light_reference.py's samples in float64 with
the oracle's occlusion (tests/query_reference.py: oracle_ray's route, rzo_first_hit through a 1 x 1 camera), and one cosine-sampled bounce
of the same by a sampler of its own (numpy's generator, not the bake's table).  pipeline() chains the committed restatements from the charts
to the pixel.  The difference of the two per group is the discretisation the bar of the tests allows for; it involves no device."""
import ctypes as C
import os

import numpy as np

import atlas_reference as AR
import bake_reference as BR
import gather_reference as GR
import gather_world as GW
import light_reference as LR
import oracle
import query_reference as QR
import view_reference as VR
from rayzath_amd import _abi, bake, gather, view
from rayzath_amd.engine import RenderConfig, Tracing
from rayzath_amd.query import HIT_EXTERNAL, HIT_FOUND, hit_dtype
from rayzath_amd.scene import Camera, DirectLight, Material, SpotLight, camera_struct, flatten

F = np.float32
CAMERA, ATLAS = (64, 48), (128, 96)
COLOR = (200, 200, 200, 255)
ALBEDO = tuple(float(F(c) / F(255.0)) for c in COLOR[:3])
SPOT = dict(GW.SPOT, size=0.05, emission=3000.0)
DIRECT = dict(GW.DIRECT, angular_size=0.02, emission=200.0)
SKY_COLOR, SKY_EMISSION = (140, 180, 255, 0), 0.4
SKY = tuple(float(F(c) / F(255.0) * F(SKY_EMISSION)) for c in SKY_COLOR[:3])
LIGHT_SAMPLES, DIRECTIONS, SEED, RINGS, NEAR, FAR = (16, 4), (64, 4), 5, 2, 1.0e-3, 1.0e3
LUMA = np.array([0.2126, 0.7152, 0.0722])
THREADS = min(16, os.cpu_count() or 1)
SIDES = {0: "top", 1: "bottom", 2: "front", 3: "back", 4: "right", 5: "left"}          # generate_cube's faces, f = triangle // 2


def luminance(rgb):
    return np.asarray(rgb, np.float64) @ LUMA


def world(resolution=CAMERA, sky=True):
    """the matte world; sky=False: the world material emits nothing"""
    w = GW.world(lights=False)
    matte = w.add(Material(COLOR, metalness=0.0, roughness=1.0, ior=1.0, name="matte"))
    black = w.add(Material((0, 0, 0, 255), metalness=0.0, roughness=1.0, ior=1.0, name="black"))
    for i, inst in enumerate(w.instances):
        inst.materials = [black if i == GW.SPHERE else matte]
    w.add(SpotLight(**SPOT))
    w.add(DirectLight(**DIRECT))
    w.material = Material(SKY_COLOR, 0.0, 0.0, SKY_EMISSION if sky else 0.0, 1.0, 0.0, name="world_material")
    w.camera = Camera(position=(0.5, 3.5, -6.0), resolution=resolution, fov=1.0, near_far=(1e-2, 1e3))
    w.camera.look_at((0.0, 0.5, 0.0))
    return w


def first_path(flat, cam, depth, seeds, threads=THREADS):
    """(mean (H, W, 3), standard error (H, W, 3)) over `seeds` of every pixel's FIRST finished path under max_depth = depth: per seed the
    oracle is rendered one pass at a time, up to `depth` passes; a pixel keeps the accumulator's rgb of the first pass after which its
    alpha is 1 — the path of the pixel-centre ray — and whatever later passes add (paths through the lens) is discarded"""
    shape = (cam.height, cam.width)
    total, squares = np.zeros(shape + (3,)), np.zeros(shape + (3,))
    for seed in seeds:
        r = oracle.OracleRenderer(flat, cam, RenderConfig(tracing=Tracing(max_depth=depth), seed=seed).struct())
        try:
            value, done = np.zeros(shape + (3,)), np.zeros(shape, bool)
            for _ in range(depth):
                r.render(1, threads=threads)
                a = r.accum
                now = ~done & (a[..., 3] == 1.0)
                value[now], done = a[..., :3][now], done | now
            assert done.all(), "a path of at most `depth` segments is finished after `depth` passes"
        finally:
            r.close()
        total += value
        squares += value * value
    n = len(seeds)
    mean = total / n
    var = np.maximum(squares / n - mean * mean, 0.0) * (n / max(n - 1, 1))
    return mean, np.sqrt(var / n)


class Caster:
    """query_reference.oracle_ray for many rays: the same entry point (rzo_first_hit through a 1 x 1 camera at the ray's origin whose
    z_axis is the ray's direction), with the camera and the record made once"""

    def __init__(self, flat, cam):
        self.flat, self.lib = flat, oracle.load()
        self.one = _abi.Camera.from_buffer_copy(cam)
        self.one.width = self.one.height = 1
        self.rec = np.zeros(1, oracle.first_hit_dtype)
        self.rays = 0

    def hits(self, origin, direction, near, far):
        """oracle.first_hit_dtype records of rays (n, 3), (n, 3), (n,), (n,)"""
        origin, direction = np.asarray(origin, F).reshape(-1, 3), np.asarray(direction, F).reshape(-1, 3)
        near, far = np.broadcast_to(np.asarray(near, F), len(origin)), np.broadcast_to(np.asarray(far, F), len(origin))
        out = np.zeros(len(origin), oracle.first_hit_dtype)
        one, rec, call = self.one, self.rec, self.lib.rzo_first_hit
        scene, camera, where = C.byref(self.flat.struct), C.byref(one), rec.ctypes.data
        o, d, nf = origin.tolist(), direction.tolist(), np.stack([near, far], -1).tolist()
        for k in range(len(o)):
            one.position[:], one.z_axis[:], one.near_far[:] = o[k], d[k], nf[k]
            call(scene, camera, 0, 0, 0, where)
            out[k] = rec[0]
        self.rays += len(o)
        return out

    def occluded(self, origin, direction, near, far):
        return self.hits(origin, direction, near, far)["instance"] != _abi.GUIDE_MISS


def surface(flat, cam, caster):
    """what every pixel's centre ray hits first, from the oracle: dict(hits (H, W) hit_dtype, origin, direction (H, W, 3) float64 unit,
    point (H, W, 3) float64 on the surface, normal (H, W, 3) the record's (it faces the camera))"""
    rays = QR.pixel_rays_d0(cam)
    d = rays["direction"].astype(np.float64)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = rays["origin"].astype(np.float64)
    rec = caster.hits(rays["origin"].reshape(-1, 3), rays["direction"].reshape(-1, 3), rays["near"].reshape(-1), rays["far"].reshape(-1)).reshape(rays.shape)
    assert rec.tobytes() == oracle.first_hits(flat, cam).tobytes(), "the 1 x 1 camera's record is rzo_first_hit_frame's"
    hits = QR.as_hits(rec)
    return dict(hits=hits, origin=o, direction=d, point=o + hits["t"].astype(np.float64)[..., None] * d, normal=hits["normal"].astype(np.float64))


def faces(hits, base):
    """the pixel groups {name: (H, W) bool}: floor, wall and every cube face (instance CUBE, triangle // 2) the camera sees, front-face
    hits on a mapped instance only — the pixels a view marks ATLAS"""
    front = ((hits["flags"] & HIT_FOUND) != 0) & ((hits["flags"] & HIT_EXTERNAL) != 0)
    mapped = front & (np.asarray(base)[np.maximum(hits["instance"], 0)] != gather.NONE)
    out = {"floor": mapped & (hits["instance"] == GW.FLOOR), "wall": mapped & (hits["instance"] == GW.WALL)}
    cube = mapped & (hits["instance"] == GW.CUBE)
    for f in np.unique(hits["triangle"][cube] // 2):
        out[f"cube {SIDES[int(f)]}"] = cube & (hits["triangle"] // 2 == f)
    return out


def lifted(point, normal, t):
    """the point the tracer lights and continues from: p + n * (1e-4 * t) (TracingResult's point), as bake points with near 0"""
    return bake.points(point + normal * (1.0e-4 * t)[..., None], normal, 0.0, 3.0e38)


def direct64(points, flat, caster, samples=LIGHT_SAMPLES, seed=SEED):
    """(n, 3) float64: include/hiprz_light.h's light at 1-d bake points, light_reference.samples evaluated in float64 under the library's
    disk table, every kept sample's shadow ray walked by the oracle"""
    points = np.ascontiguousarray(points).reshape(-1)
    spots, directs = list(flat.spot_lights), list(flat.direct_lights)
    w3, far, w, kept = LR.samples(points, spots, directs, LR.disk_table(*samples), seed, np.float64)
    n, L, K = w.shape
    origin = np.broadcast_to(points["position"][:, None, None, :], w3.shape)
    near = np.broadcast_to(points["near"][:, None, None], w.shape)
    blocked = np.zeros(w.shape, bool)
    blocked[kept] = caster.occluded(origin[kept], w3[kept], near[kept], far[kept])
    ce = LR.colour_emission(spots, directs, np.float64)
    return np.einsum("nlk,lc->nc", np.where(kept & ~blocked, w, 0.0), ce) / K


def bounce64(points, flat, caster, base, rays_per_point=32, light_samples=2, seed=11, sky=SKY, albedo=ALBEDO):
    """(mean (n, 3) float64, its standard error (n, 3)): one bounce at 1-d bake points, the mean over `rays_per_point` cosine-sampled directions (numpy's generator and
    Malley's method, nothing of the bake's table) of what arrives: the sky on a miss, albedo x direct64 (`light_samples` per light) at a
    front-face hit on a mapped instance, 0 on a back face or the unmapped sphere — include/hiprz_gather.h "A RAY'S CONTRIBUTION" with
    the source that compose makes of the direct light alone"""
    points = np.ascontiguousarray(points).reshape(-1)
    rng = np.random.default_rng(seed)
    n, K = len(points), rays_per_point
    normal = points["normal"].astype(np.float64)
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    helper = np.where(np.abs(normal[:, 0:1]) < 0.9, np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    t = np.cross(helper, normal)
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    bt = np.cross(normal, t)
    r, phi = np.sqrt((np.arange(K) + rng.random((n, K))) / K), 2.0 * np.pi * rng.random((n, K))          # stratified in r^2
    d = (t[:, None] * (r * np.cos(phi))[..., None] + bt[:, None] * (r * np.sin(phi))[..., None]) + normal[:, None] * np.sqrt(np.maximum(0.0, 1.0 - r * r))[..., None]
    origin = np.broadcast_to(points["position"][:, None, :], d.shape).reshape(-1, 3)
    rec = caster.hits(origin, d.reshape(-1, 3), 0.0, 3.0e38)
    hits = QR.as_hits(rec)
    found = (hits["flags"] & HIT_FOUND) != 0
    lit = found & ((hits["flags"] & HIT_EXTERNAL) != 0) & (np.asarray(base)[np.maximum(hits["instance"], 0)] != gather.NONE)
    dn = d.reshape(-1, 3)[lit]
    dn = dn / np.linalg.norm(dn, axis=-1, keepdims=True)
    p = origin[lit].astype(np.float64) + hits["t"][lit].astype(np.float64)[:, None] * dn
    there = lifted(p, hits["normal"][lit].astype(np.float64), hits["t"][lit].astype(np.float64))
    value = np.zeros((n * K, 3))
    value[lit] = np.asarray(albedo, np.float64) * direct64(there, flat, caster, (light_samples, 64), seed)
    value[~found] = np.asarray(sky, np.float64)
    value = value.reshape(n, K, 3)
    return value.mean(1), value.std(1, ddof=1) / np.sqrt(K)


class Pipeline:
    """the committed restatements chained from the charts to the pixel — atlas_reference.build, light_reference's rays and texels over the
    oracle's verdicts, gather_reference.compose, atlas_reference.dilate, bake_reference's rays and gather_reference.texels over the
    oracle's hits, view_reference.atlas_taps over samples made from the oracle's first hits.  What depends on the charts alone (the atlas,
    the direct light and what the gather's rays hit) is computed once per instance; pixels() takes what a case varies."""

    def __init__(self, w, flat, caster, parts, W, H, samples=LIGHT_SAMPLES, directions=DIRECTIONS, seed=SEED, rings=RINGS):
        self.w, self.flat, self.caster, self.W, self.H, self.seed, self.rings, self.directions = w, flat, caster, W, H, seed, rings, directions
        self.base, self.charts = gather.chart_tables(parts, len(flat.instances))
        self.triangles = GW.world_triangles(w, flat)
        _, self.samples, pts = AR.build([(AR.placement_of(flat.instances[i]), tris) for i, tris in parts], W, H, NEAR, FAR)
        self.points = pts.reshape(-1)
        self.has = BR.valid(self.points)
        spots, directs = list(flat.spot_lights), list(flat.direct_lights)
        rays, weights = LR.rays(self.points, spots, directs, LR.disk_table(*samples), seed)
        walked = weights > 0
        words = np.zeros(weights.shape, np.uint32)
        words[walked] = caster.occluded(rays["origin"][walked], rays["direction"][walked], rays["near"][walked], rays["far"][walked])
        self.direct = LR.texels(self.points, weights, words, LR.colour_emission(spots, directs)).reshape(H, W)
        self.gathered, self.sources = None, {}

    def _gather_samples(self):
        """gather.sample_dtype (n, K) of the bake's own rays: the oracle's hit, its chart id by gather_reference.ids and the float64
        barycentrics of the ray on the triangle the oracle names"""
        if self.gathered is None:
            rays = BR.rays(self.points, BR.cosine_table(*self.directions), self.seed)
            out = np.zeros(rays.shape, gather.sample_dtype)
            out["id"] = gather.INVALID_RAY
            ok = np.broadcast_to(self.has[:, None], rays.shape)
            out[ok] = samples_of(QR.as_hits(self.caster.hits(rays["origin"][ok], rays["direction"][ok], rays["near"][ok], rays["far"][ok])),
                                 rays["origin"][ok], rays["direction"][ok], self.triangles, self.base, len(self.charts))
            self.gathered = out
        return self.gathered

    def source(self, bounces, albedo=ALBEDO, sky=SKY):
        """the W x H source a view reads: albedo x (direct + indirect of `bounces` bounces), dilated"""
        key = (bounces, tuple(albedo), tuple(sky))
        if key not in self.sources:
            a = gather.records(albedo, (self.H, self.W))
            indirect = None
            for _ in range(bounces):
                src, _ = AR.dilate(GR.compose(self.direct, indirect, a, None), self.samples, self.rings)
                indirect = GR.texels(self.points, self._gather_samples(), self.charts, src, self.W, self.H, sky).reshape(self.H, self.W)
            self.sources[key] = AR.dilate(GR.compose(self.direct, indirect, a, None), self.samples, self.rings)[0]
        return self.sources[key]

    def pixels(self, view_samples, bounces, filter, albedo=ALBEDO, sky=SKY):
        """(rgb (H_c, W_c, 3) float32, count) of the camera's pixels"""
        return VR.atlas_taps(view_samples, self.charts, self.source(bounces, albedo, sky), self.W, self.H, filter)


def samples_of(hits, origin, direction, triangles, base, n_charts):
    """gather.sample_dtype of hit_dtype rows: id by gather_reference.ids, bx and by the float64 barycentrics (tests/gather_world.py) of the
    ray on the world-space triangle the hit names, rounded to float32"""
    hits = np.asarray(hits)
    ids = GR.ids(hits["flags"], hits["instance"], hits["triangle"], base, n_charts)
    found = (hits["flags"] & HIT_FOUND) != 0
    bx, by = np.zeros(hits.shape), np.zeros(hits.shape)
    if found.any():
        tri = np.zeros(hits.shape + (3, 3))
        for i in np.unique(hits["instance"][found]):
            at = found & (hits["instance"] == i)
            tri[at] = triangles[i][hits["triangle"][at]]
        d = np.asarray(direction, np.float64)
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        _, b1, b2, _ = GW.barycentrics(tri[found], np.asarray(origin, np.float64)[found], d[found])
        bx[found], by[found] = b1, b2
    return GR.make_samples(ids, bx.astype(F), by.astype(F), hits["t"])


def bias(flat, points):
    """2 x the larger solid angle of the lights as flatten stores them: the direct light's 2 pi (1 - cos_angular_size) and the spot's
    A / (d + 1)^2 at the nearest of `points`.  The tracer weights its light sample with Lw = 1 / (1 + solid angle x pdf) >= 1 / (1 + solid
    angle) (the pdf of a diffuse surface is a cosine, <= 1) and adds a BRDF-sampled term of second order in the solid angle."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    omega = [2.0 * np.pi * (1.0 - float(l["cos_angular_size"])) for l in flat.direct_lights]
    for l in flat.spot_lights:
        d = np.linalg.norm(l["position"].astype(np.float64) - p, axis=-1).min()
        omega.append(np.pi * float(l["size"]) ** 2 / (d + 1.0) ** 2)
    return 2.0 * max(omega)


def group_ratio(baked, mean, err, mask):
    """(baked / traced of the group's mean luminance, the standard error of the traced mean relative to it): the pixels' errors are
    independent of one another (every pixel has its own generator), a pixel's three channels are not (bounded by their weighted sum)"""
    traced = luminance(mean)[mask].mean()
    se = np.sqrt(((np.asarray(err, np.float64) @ LUMA)[mask] ** 2).sum()) / mask.sum()
    return float(luminance(baked)[mask].mean() / traced), float(se / traced)


SEEDS = range(100, 356)
_ONCE = {}


def study():
    """everything both test modules share, computed once per process and never written to: the world, the oracle's first hits and the
    groups, the float64 rules at the pixels' points, the first-path frames of depth 1 and 2 over SEEDS, the pipeline of the default
    charts and, per (bounces, filter) and group, the discretisation: |pipeline / rule - 1| of the group's mean luminance"""
    if "study" not in _ONCE:
        w = world()
        flat, cam = flatten(w), camera_struct(w.camera)
        caster = Caster(flat, cam)
        parts = GW.parts(w)
        base, charts = gather.chart_tables(parts, len(flat.instances))
        s = surface(flat, cam, caster)
        groups = faces(s["hits"], base)
        atlas_pixels = np.logical_or.reduce(list(groups.values()))
        points = lifted(s["point"][atlas_pixels], s["normal"][atlas_pixels], s["hits"]["t"][atlas_pixels].astype(np.float64))
        direct, bounce, bounce_err = (np.zeros(atlas_pixels.shape + (3,)) for _ in range(3))
        direct[atlas_pixels] = direct64(points, flat, caster)
        bounce[atlas_pixels], bounce_err[atlas_pixels] = bounce64(points, flat, caster, base, 128)
        albedo = np.asarray(ALBEDO, np.float64)
        rules = {0: albedo * direct, 1: albedo * (direct + bounce)}
        frames = {depth: first_path(flat, cam, depth, SEEDS) for depth in (1, 2)}
        pipe = Pipeline(w, flat, caster, parts, *ATLAS)
        view_samples = samples_of(s["hits"], s["origin"], s["direction"], pipe.triangles, base, len(charts))
        baked, discretisation = {}, {}
        for bounces in (0, 1):
            for filter in (view.NEAREST, view.BILINEAR):
                rgb, count = pipe.pixels(view_samples, bounces, filter)
                assert (count[atlas_pixels] > 0).all(), "a mapped pixel reads no texel"
                baked[bounces, filter] = rgb
                discretisation[bounces, filter] = {g: abs(luminance(rgb)[m].mean() / luminance(rules[bounces])[m].mean() - 1.0) for g, m in groups.items()}
        _ONCE["study"] = dict(world=w, flat=flat, cam=cam, caster=caster, parts=parts, base=base, charts=charts, surface=s, groups=groups, atlas_pixels=atlas_pixels,
                              rules=rules, rule_err={0: np.zeros_like(bounce_err), 1: albedo * bounce_err}, frames=frames, pipeline=pipe, view_samples=view_samples,
                              baked=baked, discretisation=discretisation, bias=bias(flat, s["point"][atlas_pixels]))
    return _ONCE["study"]


def pipeline(parts, W, H, bounces, filter, albedo=ALBEDO, sky=SKY):
    """(rgb (H_c, W_c, 3), count) of the study's camera under the restatements chained over `parts`; the instance of the default charts at
    ATLAS is the study's own"""
    st = study()
    key = ("pipeline", W, H, np.concatenate([t.view(np.uint8).reshape(-1) for _, t in parts]).tobytes())
    if key not in _ONCE:
        same = (W, H) == ATLAS and key[3] == np.concatenate([t.view(np.uint8).reshape(-1) for _, t in st["parts"]]).tobytes()
        _ONCE[key] = st["pipeline"] if same else Pipeline(st["world"], st["flat"], st["caster"], parts, W, H)
    p = _ONCE[key]
    samples = samples_of(st["surface"]["hits"], st["surface"]["origin"], st["surface"]["direction"], p.triangles, p.base, len(p.charts))
    return p.pixels(samples, bounces, filter, albedo, sky)


def bar(st, bounces, filter, group, depth):
    """(the bar, its three terms) of a group: bias + discretisation + 4 x the standard error of the traced group mean"""
    mean, err = st["frames"][depth]
    se = group_ratio(mean, mean, err, st["groups"][group])[1]
    terms = (st["bias"], st["discretisation"][bounces, filter][group], 4.0 * se)
    return sum(terms), terms
