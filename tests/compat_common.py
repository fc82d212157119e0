"""Shared by the CUDA-compat tests: the analytic micro-scenes and the float64 fetch restatement that test_cuda_compat_gpu.py checks the
GPU with and test_oracle_compat.py checks the oracle with (the same scene objects on both sides), the float32 fetch restatement of the
oracle's KAT, and the scenes of the oracle comparison (test_cuda_compat_oracle_gpu.py)."""
import math

import numpy as np

from rayzath_amd import _abi
from rayzath_amd.scene import Camera, Instance, Material, Mesh, SpotLight, TextureBuffer, World, generate_plane

F = np.float32
TEX_FILTER_LINEAR = 1                                             # hiprz.h HIPRZ_TEX_FILTER_* / HIPRZ_TEX_ADDRESS_*
TEX_ADDRESS_CLAMP, TEX_ADDRESS_MIRROR, TEX_ADDRESS_BORDER = 1 << 8, 2 << 8, 3 << 8
TEXEL_LIMIT = F(2.0 ** 30)   # texel coordinates are exact below |u * w| = 2^30 and clamped there (hiprz_compat.hpp, rz_oracle.c D4)


def quad(size, z=0.0):
    """Square [-size, size]^2 in the plane z, facing -z (towards a camera on the negative z axis), uv = ((x + size) / 2 size, (y + size) / 2 size)."""
    v = [(-size, -size, z), (size, -size, z), (size, size, z), (-size, size, z)]
    t = [(0, 0), (1, 0), (1, 1), (0, 1)]
    return Mesh(v, [(0, 2, 1), (0, 3, 2)], texcrds=t, tri_texcrds=[(0, 2, 1), (0, 3, 2)], name="quad")


def narrow_camera(width=64, height=64, fov=0.2, z=-3.0):
    return Camera(position=(0, 0, z), rotation=(0, 0, 0), resolution=(width, height), fov=fov, near_far=(1e-2, 1e3), focal_distance=3.0,
                  aperture=1e-6, exposure_time=1.0 / 60.0)


def slab_scene(thickness=0.5):
    world = World()
    glow = world.add(Material((255, 255, 255, 255), 0.0, 1.0, emission=1.0, name="panel"))
    tinted = world.add(Material((200, 150, 100, 128), 0.0, 0.0, 0.0, 1.0, 0.0, name="absorbing glass"))   # ior 1: rays go straight through
    world.add(Instance(world.add(quad(3.0)), [glow], position=(0, 0, 2.0), name="panel"))
    world.add(Instance(world.add(_cube()), [tinted], rotation=(0.0, 0.0, 0.37), scale=(4.0, 4.0, thickness), name="slab"))  # turned about z: no pixel centre on a face diagonal
    world.camera = narrow_camera()
    return world


def _cube():
    from rayzath_amd.scene import generate_cube
    return generate_cube()


def fog_scene(sigma=0.5, distance=4.0):
    world = World()
    world.material = Material((255, 255, 255, 0), 0.0, 0.0, 0.0, 1.0, sigma, name="fog")
    wall = world.add(Material((255, 255, 255, 255), 0.0, 1.0, emission=1.0, name="wall"))
    world.add(Instance(world.add(quad(3.0)), [wall], position=(0, 0, distance - 3.0), name="wall"))
    world.camera = narrow_camera(128, 128)
    return world


def shadow_scene(with_sheet):
    world = World()
    floor = world.add(Material((255, 255, 255, 255), 0.0, 1.0, name="floor"))
    world.add(Instance(world.add(generate_plane(4, 8.0, 8.0)), [floor], position=(0, -1, 0), name="floor"))
    if with_sheet:
        sheet = world.add(Material((255, 64, 64, 128), 0.0, 0.3, name="red sheet"))
        world.add(Instance(world.add(generate_plane(4, 1.5, 1.5)), [sheet], position=(0, 1.0, 0), name="sheet"))
    world.add(SpotLight(position=(0, 3.0, 0), direction=(0, -1, 0), color=(255, 255, 255, 255), size=0.05, emission=200.0, beam_angle=1.2))
    world.camera = Camera(position=(0, -0.2, -2.5), rotation=(-0.35, 0, 0), resolution=(96, 64), fov=1.0, near_far=(1e-2, 1e3),
                          focal_distance=3.0, aperture=1e-6, exposure_time=1.0 / 60.0)
    return world


def map_panel(emission_map, texture=None, color=(255, 255, 255, 255), emission=1.0):
    world = World()
    m = world.add(Material(color, 0.0, 1.0, emission=emission, texture=texture, emission_map=emission_map, name="panel"))
    world.add(Instance(world.add(quad(1.0)), [m], name="panel"))
    world.camera = narrow_camera(96, 96, fov=0.5)
    return world


def panel_hits(cam):
    """Where generateSimpleRay of narrow_camera(.., z=-3) meets the plane z = 0, per pixel."""
    px, py = np.meshgrid(np.arange(cam.width), np.arange(cam.height))
    tan = np.tan(cam.fov / 2)
    hit_x = ((px + 0.5) / cam.width - 0.5) * tan * 3.0
    hit_y = ((py + 0.5) / cam.height - 0.5) * (-tan / (cam.width / cam.height)) * 3.0
    return hit_x, hit_y


def sample_numpy(bitmap, u, v, scale, filter_mode, address_mode):
    """TextureBuffer::fetch of the CUDA engine on an R32F map without rotation / translation (cuda_buffer.cuh:427-438), float64."""
    h, w = bitmap.shape
    x, y = u * scale[0], 1.0 - v * scale[1]

    def texel(i, n):
        if address_mode == "clamp":
            return np.clip(i, 0, n - 1), np.ones_like(i, dtype=bool)
        if address_mode == "border":
            return np.clip(i, 0, n - 1), (i >= 0) & (i < n)
        if address_mode == "mirror":
            k = np.mod(i, 2 * n)
            return np.where(k < n, k, 2 * n - 1 - k), np.ones_like(i, dtype=bool)
        return np.mod(i, n), np.ones_like(i, dtype=bool)

    if filter_mode == "point":
        xi, okx = texel(np.floor(x * w).astype(int), w)
        yi, oky = texel(np.floor(y * h).astype(int), h)
        return np.where(okx & oky, bitmap[yi, xi], 0.0)
    fx, fy = x * w - 0.5, y * h - 0.5
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    ax, ay = fx - x0, fy - y0
    out = np.zeros_like(x)
    for k in range(4):
        xi, okx = texel(x0 + (k & 1), w)
        yi, oky = texel(y0 + (k >> 1), h)
        wgt = np.where(k & 1, ax, 1 - ax) * np.where(k >> 1, ay, 1 - ay)
        out += np.where(okx & oky, bitmap[yi, xi], 0.0) * wgt
    return out


def texels_as_float(flat, index):
    """Texture `index` of a flattened scene as (H, W, 4) float32, as a texture object reads it: uint8 kinds normalised (/255), R32F as
    is, missing channels 0."""
    rec = flat.textures[index]
    w, h, off, kind = int(rec["width"]), int(rec["height"]), int(rec["offset"]), int(rec["kind"])
    pool = np.asarray(flat.texels).view(np.uint8)
    out = np.zeros((h, w, 4), F)
    if kind == _abi.TEX_RGBA8:
        out[:] = pool[off:off + 4 * w * h].reshape(h, w, 4).astype(F) / F(255)
    elif kind == _abi.TEX_R8:
        out[..., 0] = pool[off:off + w * h].reshape(h, w).astype(F) / F(255)
    else:
        out[..., 0] = pool[off:off + 4 * w * h].view(F).reshape(h, w)
    return out


def fetch_numpy(flat, index, u, v):
    """TextureBuffer::fetch (cuda_buffer.cuh:427-438) restated with numpy in float32, every rounding as the C restatement has it: texcrd +=
    translation, rotated, scaled, tex2D(x, 1 - y) with normalised coordinates under the texture's filter and address modes."""
    rec = flat.textures[index]
    img = texels_as_float(flat, index)
    h, w = img.shape[:2]
    with np.errstate(invalid="ignore", over="ignore"):     # coordinates near the float limit become inf / NaN here as in C
        u, v = np.asarray(u, F) + rec["translation"][0], np.asarray(v, F) + rec["translation"][1]
        xx = u * rec["cos_rotation"] - v * rec["sin_rotation"]
        yy = u * rec["sin_rotation"] + v * rec["cos_rotation"]
        u, v = xx * rec["scale"][0], F(1) - yy * rec["scale"][1]
    address, linear = int(rec["sampling"]) & 0xFF00, (int(rec["sampling"]) & 0xFF) == TEX_FILTER_LINEAR

    def clampf(x):
        x = np.where(np.isnan(x), -TEXEL_LIMIT, x)
        return np.minimum(np.maximum(x, -TEXEL_LIMIT), TEXEL_LIMIT).astype(F)

    def texel(i, n):
        if address == TEX_ADDRESS_CLAMP:
            return np.clip(i, 0, n - 1), np.ones_like(i, dtype=bool)
        if address == TEX_ADDRESS_BORDER:
            return np.clip(i, 0, n - 1), (i >= 0) & (i < n)
        if address == TEX_ADDRESS_MIRROR:
            k = np.mod(i, 2 * n)
            return np.where(k < n, k, 2 * n - 1 - k), np.ones_like(i, dtype=bool)
        return np.mod(i, n), np.ones_like(i, dtype=bool)

    with np.errstate(invalid="ignore", over="ignore"):
        if not linear:
            xi, okx = texel(np.floor(clampf(u * F(w))).astype(np.int64), w)
            yi, oky = texel(np.floor(clampf(v * F(h))).astype(np.int64), h)
            return np.where((okx & oky)[..., None], img[yi, xi], F(0))
        fx, fy = clampf(u * F(w) - F(0.5)), clampf(v * F(h) - F(0.5))
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0).astype(F), (fy - y0).astype(F)
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    out = np.zeros(fx.shape + (4,), F)
    for k in range(4):
        xi, okx = texel(x0 + (k & 1), w)
        yi, oky = texel(y0 + (k >> 1), h)
        wgt = (ax if k & 1 else F(1) - ax) * (ay if k >> 1 else F(1) - ay)
        out = out + np.where((okx & oky)[..., None], img[yi, xi] * wgt[..., None], F(0))
    return out


def _maps(rng):
    """RGBA8 / R8 / R32F maps under every filter x address mode, on transforms that leave [0, 1]."""
    modes = [(f, a) for f in ("point", "linear") for a in ("wrap", "clamp", "mirror", "border")]
    transforms = [dict(scale=(2.5, -1.75), rotation=0.7, translation=(0.3, -1.2)), dict(scale=(-1.6, 3.1), rotation=-2.2, translation=(-2.5, 0.9)),
                  dict(scale=(0.7, 0.45), rotation=0.0, translation=(1.7, 2.3)), dict(scale=(4.0, 4.0), rotation=3.0, translation=(-0.4, -0.6))]

    def buf(bitmap, i):
        f, a = modes[i % len(modes)]
        return TextureBuffer(bitmap, filter_mode=f, address_mode=a, **transforms[i % len(transforms)])

    rgba = [rng.integers(40, 256, size=(h, w, 4), dtype=np.uint8) for h, w in ((5, 7), (8, 8), (3, 1), (6, 9))]
    for t in rgba:
        t[..., 3] = rng.integers(60, 256, size=t.shape[:2])        # partly transparent: the alpha turns into transmission / mask alpha
    r8 = [rng.integers(0, 256, size=(h, w), dtype=np.uint8) for h, w in ((4, 5), (7, 3))]
    r32 = [rng.uniform(0.2, 3.0, size=(h, w)).astype(np.float32) for h, w in ((3, 4), (5, 5))]
    return [buf(b, i) for i, b in enumerate(rgba)], [buf(b, i + 4) for i, b in enumerate(r8)], [buf(b, i + 6) for i, b in enumerate(r32)]


def compat_showcase(width=160, height=96, seed=3):
    """Every CUDA-compat behaviour in one small scene: coloured, partly transparent textured sheets between a spot light, a direct light and
    the receivers; tinted absorbing glass (material alpha < 255); a scattering world medium and one scattering object; RGBA8, R8 and R32F
    maps under every filter x address mode on transforms that leave [0, 1]."""
    from rayzath_amd.scene import DirectLight, generate_cube, generate_sphere
    rng = np.random.default_rng(seed)
    rgba, r8, r32 = _maps(rng)
    world = World()
    world.material = Material((235, 240, 255, 0), 0.0, 0.0, 0.15, 1.0, 0.06, texture=rgba[3], name="hazy sky")  # scattering air, textured sky
    floor = world.add(Material((230, 230, 220, 255), 0.0, 0.7, texture=rgba[1], roughness_map=r8[0], name="floor"))
    wall = world.add(Material((200, 210, 230, 255), 0.2, 0.4, metalness_map=r8[1], name="wall"))
    sheet_a = world.add(Material((255, 120, 90, 90), 0.0, 0.3, 0.0, 1.0, texture=rgba[0], name="red sheet"))
    sheet_b = world.add(Material((80, 200, 255, 150), 0.0, 0.5, 0.0, 1.0, texture=rgba[2], name="blue sheet"))
    glass = world.add(Material((180, 255, 200, 110), 0.0, 0.0, 0.0, 1.35, 0.0, name="tinted glass"))
    smoke = world.add(Material((255, 230, 200, 60), 0.0, 0.3, 0.0, 1.0, 0.9, name="smoke"))
    panel = world.add(Material((255, 250, 240, 255), 0.0, 1.0, 2.0, texture=rgba[0], emission_map=r32[0], name="glow panel"))
    panel2 = world.add(Material((255, 255, 255, 255), 0.0, 1.0, 1.5, emission_map=r32[1], name="glow strip"))
    plane, cube, sphere = world.add(generate_plane(4, 1.0, 1.0)), world.add(generate_cube()), world.add(generate_sphere(16))
    tex_quad = world.add(quad(1.0))
    world.add(Instance(world.add(quad(6.0)), [floor], position=(0, -1, 1), rotation=(-math.pi / 2, 0, 0), name="floor"))
    world.add(Instance(world.add(quad(6.0)), [wall], position=(0, 1, 4), name="back wall"))
    world.add(Instance(tex_quad, [sheet_a], position=(-0.6, 0.8, 1.2), rotation=(-1.2, 0.3, 0), scale=(1.2, 1.2, 1.0), name="sheet a"))
    world.add(Instance(tex_quad, [sheet_b], position=(0.7, 0.5, 1.6), rotation=(-1.4, -0.2, 0.4), scale=(1.0, 1.4, 1.0), name="sheet b"))
    world.add(Instance(cube, [glass], position=(0.9, -0.5, 1.0), rotation=(0.2, 0.6, 0), scale=(0.5, 0.5, 0.5), name="glass"))
    world.add(Instance(sphere, [smoke], position=(-0.9, -0.45, 0.9), scale=(0.55, 0.55, 0.55), name="smoke ball"))
    world.add(Instance(tex_quad, [panel], position=(0.0, 1.2, 3.9), scale=(0.9, 0.5, 1.0), name="panel"))
    world.add(Instance(plane, [panel2], position=(-1.8, 0.2, 3.0), rotation=(1.5, 0.4, 0), scale=(0.8, 1.0, 0.3), name="strip"))
    world.add(SpotLight(position=(-0.4, 2.6, 1.0), direction=(0.1, -1.0, 0.1), color=(255, 240, 220, 255), size=0.15, emission=120.0, beam_angle=1.1))
    world.add(DirectLight(direction=(0.4, -1.0, 0.6), color=(255, 250, 240, 255), emission=20.0, angular_size=0.06))
    world.camera = Camera(position=(0, 0.4, -2.2), rotation=(-0.12, 0, 0), resolution=(width, height), fov=1.2, near_far=(1e-2, 1e3),
                          focal_distance=3.0, aperture=1e-6, exposure_time=1.0 / 60.0)
    return world


def open_sky(width=96, height=64):
    """A textured, emission-mapped sky around a camera that stands outside the scene's bounds: most primary rays miss the world's root box,
    where the CUDA engine still takes the sky's texcrd (calculateTexcrd, cuda_world.cuh:86-88) and the CPU engine keeps (0, 0)."""
    from rayzath_amd.scene import generate_cube
    rng = np.random.default_rng(17)
    sky_tex = rng.integers(30, 256, size=(6, 9, 4), dtype=np.uint8)
    sky_tex[..., 3] = 255
    sky_em = rng.uniform(0.5, 2.5, size=(5, 7)).astype(np.float32)
    world = World()
    world.material = Material((255, 255, 255, 0), 0.0, 0.0, 1.0, 1.0, 0.0, texture=TextureBuffer(sky_tex, filter_mode="linear"),
                              emission_map=TextureBuffer(sky_em, address_mode="mirror"), name="mapped sky")
    box = world.add(Material((200, 180, 160, 255), 0.0, 0.6, name="box"))
    world.add(Instance(world.add(generate_cube()), [box], position=(0.8, 0.0, 0.0), scale=(0.5, 0.5, 0.5), name="box"))
    world.add(SpotLight(position=(0.8, 2.0, -1.0), direction=(0, -1, 0.3), color=(255, 255, 255, 255), size=0.1, emission=50.0, beam_angle=1.2))
    world.camera = Camera(position=(0, 0, -4.0), rotation=(0, 0, 0), resolution=(width, height), fov=1.4, near_far=(1e-2, 1e3),
                          focal_distance=4.0, aperture=1e-6, exposure_time=1.0 / 60.0)
    return world
