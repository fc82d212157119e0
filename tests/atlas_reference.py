"""Bake atlases (include/hiprz_atlas.h) restated in numpy float32, one rounding per operation like the device build (-ffp-contract=off):
the texel-space vertices, the canonical edge value, coverage with the lowest id as owner, the samples, the points under a placement given
as arrays, and the dilation.  For tests/test_atlas_reference.py (CPU), which holds it to answers worked by hand and to float64, and for
tests/test_atlas_gpu.py and tools/atlas_time.py, which hold the device to it in every byte."""
import numpy as np

from rayzath_amd.atlas import NONE, sample_dtype, tri_dtype
from rayzath_amd.bake import point_dtype

F = np.float32
ONE, HALF = F(1.0), F(0.5)
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))     # (dx, dy), the order a gutter texel asks in


def texel_vertices(tris, W, H):
    """a_i = (u_i * float(W) - 0.5, v_i * float(H) - 0.5): three (n, 2) float32 arrays"""
    t = np.ascontiguousarray(tris).reshape(-1).view(tri_dtype)
    with np.errstate(all="ignore"):
        return tuple(np.stack([t[f"u{k}"] * F(W) - HALF, t[f"v{k}"] * F(H) - HALF], -1).astype(F) for k in (1, 2, 3))


def edge(P, Q, px, py):
    """the oriented value at (px, py) of the edge walked from P to Q ((..., 2) float32 each): e of the canonical pair (smaller x first, ties
    by smaller y), negated when the walk runs from B to A"""
    swap = (Q[..., 0] < P[..., 0]) | ((Q[..., 0] == P[..., 0]) & (Q[..., 1] < P[..., 1]))
    A, B = np.where(swap[..., None], Q, P), np.where(swap[..., None], P, Q)
    with np.errstate(all="ignore"):
        e = (B[..., 0] - A[..., 0]) * (py - A[..., 1]) - (B[..., 1] - A[..., 1]) * (px - A[..., 0])
    return np.where(swap, -e, e).astype(F)


def orientation(tris, W, H):
    """(area, s, degenerate) per triangle: area the oriented value of edge 1->2 at a_3, s = +-1 its sign (0 where degenerate)"""
    t = np.ascontiguousarray(tris).reshape(-1).view(tri_dtype)
    a1, a2, a3 = texel_vertices(t, W, H)
    area = edge(a1, a2, a3[:, 0], a3[:, 1])
    finite = np.isfinite(t.view(F).reshape(-1, 24)).all(-1)
    degenerate = ~finite | ~np.isfinite(area) | (area == 0)
    s = np.where(degenerate, F(0), np.where(area > 0, ONE, -ONE)).astype(F)
    return area, s, degenerate


def _box(a1, a2, a3, i, W, H):
    """the texels a triangle may cover: those with min a.x <= float(x) <= max a.x and the same in y, inside the atlas (inclusive ranges)"""
    lo = np.minimum(np.minimum(a1[i], a2[i]), a3[i])
    hi = np.maximum(np.maximum(a1[i], a2[i]), a3[i])
    x0, y0 = (int(np.ceil(max(lo[k], F(0)))) for k in (0, 1))
    x1, y1 = int(np.floor(min(hi[0], F(W - 1)))), int(np.floor(min(hi[1], F(H - 1))))
    return x0, x1, y0, y1


def cover(tris, W, H, triangle_base=0):
    """(owner (H, W) uint32 — the lowest id covering the texel or NONE, claims (H, W) — how many triangles cover it, texels per triangle)"""
    t = np.ascontiguousarray(tris).reshape(-1).view(tri_dtype)
    a1, a2, a3 = texel_vertices(t, W, H)
    area, s, degenerate = orientation(t, W, H)
    owner, claims, per_tri = np.full((H, W), NONE, np.uint32), np.zeros((H, W), np.uint32), np.zeros(len(t), np.int64)
    for i in np.flatnonzero(~degenerate):
        x0, x1, y0, y1 = _box(a1, a2, a3, i, W, H)
        if x1 < x0 or y1 < y0:
            continue
        py, px = np.meshgrid(np.arange(y0, y1 + 1).astype(F), np.arange(x0, x1 + 1).astype(F), indexing="ij")
        w1, w2, w3 = edge(a2[i], a3[i], px, py), edge(a3[i], a1[i], px, py), edge(a1[i], a2[i], px, py)
        inside = (s[i] * w1 >= 0) & (s[i] * w2 >= 0) & (s[i] * w3 >= 0)
        per_tri[i] = inside.sum()
        view = owner[y0:y1 + 1, x0:x1 + 1]
        view[inside] = np.minimum(view[inside], np.uint32(triangle_base + i))
        claims[y0:y1 + 1, x0:x1 + 1] += inside
    return owner, claims, per_tri


def samples(tris, owner, W, H, triangle_base=0):
    """(H, W) sample_dtype of an owner map whose ids lie in [triangle_base, triangle_base + len(tris)) or are NONE"""
    t = np.ascontiguousarray(tris).reshape(-1).view(tri_dtype)
    out = np.zeros((H, W), sample_dtype)
    out["triangle"] = owner
    has = owner != NONE
    if not has.any():
        return out
    i = (owner[has] - np.uint32(triangle_base)).astype(np.int64)
    a1, a2, a3 = (a[i] for a in texel_vertices(t, W, H))
    area, s, _ = (v[i] for v in orientation(t, W, H))
    ys, xs = np.nonzero(has)
    px, py = xs.astype(F), ys.astype(F)
    with np.errstate(all="ignore"):
        sa = s * area
        out["bx"][has] = (s * edge(a3, a1, px, py)) / sa
        out["by"][has] = (s * edge(a1, a2, px, py)) / sa
    return out


def _length(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def normalized(v):
    """the device's normalized(): v * (1 / sqrt((x*x + y*y) + z*z))"""
    return (v * (ONE / _length(v))[..., None]).astype(F)


def forward(xa, ya, za, v):
    """transform_forward: (xa * v.x + ya * v.y) + za * v.z on (..., 3)"""
    return ((xa * v[..., 0:1] + ya * v[..., 1:2]) + za * v[..., 2:3]).astype(F)


def face_normals(t):
    """hiprz_tri_attr::face_normal: normalize(cross(p2 - p3, p2 - p1))"""
    a, b = t["p2"] - t["p3"], t["p2"] - t["p1"]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1).astype(F)
    return normalized(c)


def points(tris, sample_array, placement, near, far, triangle_base=0):
    """(H, W) point_dtype of the samples under `placement` = (position, scale, xa, ya, za), five (3,) float32 arrays: the instance record's"""
    t = np.ascontiguousarray(tris).reshape(-1).view(tri_dtype)
    position, scale, xa, ya, za = (np.asarray(v, F).reshape(3) for v in placement)
    out = np.zeros(sample_array.shape, point_dtype)
    has = sample_array["triangle"] != NONE
    if not has.any():
        return out
    smp = sample_array[has]
    tri = t[(smp["triangle"] - np.uint32(triangle_base)).astype(np.int64)]
    with np.errstate(all="ignore"):
        bx, by = smp["bx"][:, None], smp["by"][:, None]
        b1 = (ONE - bx) - by
        p = (tri["p1"] * b1 + tri["p2"] * bx) + tri["p3"] * by
        world = forward(xa, ya, za, p * scale) + position
        flat = (np.stack([tri["n1"], tri["n2"], tri["n3"]], 1).reshape(-1, 9) == 0).all(-1)
        n = (tri["n1"] * b1 + tri["n2"] * bx) + tri["n3"] * by
        n = np.where(flat[:, None], face_normals(tri), n).astype(F)
        n = normalized(forward(xa, ya, za, normalized(n) / scale))
        bad = ~np.isfinite(n).all(-1) | (n == 0).all(-1)
        n[bad] = 0.0
    rec = np.zeros(len(smp), point_dtype)
    rec["position"], rec["near"], rec["normal"], rec["far"] = world, F(near), n, F(far)
    out[has] = rec
    return out


def placement_of(instance):
    """(position, scale, xa, ya, za) of one _abi.instance_dtype record"""
    return tuple(np.asarray(instance[k], F) for k in ("position", "scale", "x_axis", "y_axis", "z_axis"))


def build(parts, W, H, near=1.0e-3, far=3.0e38):
    """what begin + adds leave: (owner, samples, points) for `parts` = [(placement, tris), ...] with ids numbered through in list order.
    The owner of a texel is the lowest id over all parts; its sample and point are its owner's part's."""
    owner, base, bases = np.full((H, W), NONE, np.uint32), 0, []
    for _, tris in parts:
        owner = np.minimum(owner, cover(tris, W, H, base)[0])
        bases.append(base)
        base += np.asarray(tris).size
    smp, pts = np.zeros((H, W), sample_dtype), np.zeros((H, W), point_dtype)
    smp["triangle"] = NONE
    for (placement, tris), b in zip(parts, bases):
        mine = (owner != NONE) & (owner >= b) & (owner < b + np.asarray(tris).size)
        part_owner = np.where(mine, owner, np.uint32(NONE))
        s = samples(tris, part_owner, W, H, b)
        p = points(tris, s, placement, near, far, b)
        smp[mine], pts[mine] = s[mine], p[mine]
    return owner, smp, pts


def dilate(records, sample_array, rings):
    """(records after `rings` rings, ring map): records (H, W) of 16 bytes; each ring reads the state before it, a texel without a value
    takes the record of its first neighbour (NEIGHBOURS' order) that has one"""
    rec = np.ascontiguousarray(records).copy()
    H, W = rec.shape
    has = sample_array["triangle"] != NONE
    ring = np.where(has, np.uint32(0), np.uint32(NONE)).astype(np.uint32)
    for r in range(1, rings + 1):
        src_has, src = has.copy(), rec.copy()
        todo = ~src_has
        for dx, dy in NEIGHBOURS:
            ys, xs = np.nonzero(todo)
            ny, nx = ys + dy, xs + dx
            ok = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
            take = np.zeros(len(ys), bool)
            take[ok] = src_has[ny[ok], nx[ok]]
            rec[ys[take], xs[take]] = src[ny[take], nx[take]]
            has[ys[take], xs[take]] = True
            ring[ys[take], xs[take]] = r
            todo[ys[take], xs[take]] = False
    return rec, ring
