"""tests/atlas_reference.py (the rules of include/hiprz_atlas.h in numpy float32) held to known answers, without a GPU: a right triangle
in a 4x4 atlas worked by hand, the antisymmetry of the oriented edge value over every shared edge of generate_sphere(16), the independence
of the result from the order of the parts, the dilation of a hand-made 5x5 mask, the points of a unit-scale axis-aligned instance against
float64, and the coverage counts of the procedural meshes — a change of rule shows up as a changed count."""
import numpy as np
import pytest

import atlas_reference as AR
from rayzath_amd import atlas, scene
from rayzath_amd.atlas import NONE

F = np.float32
IDENTITY = (np.zeros(3, F), np.ones(3, F), np.array([1, 0, 0], F), np.array([0, 1, 0], F), np.array([0, 0, 1], F))


def _tri(p, uv, n=None):
    t = np.zeros(1, atlas.tri_dtype)
    for k in range(3):
        t[f"p{k + 1}"], t[f"u{k + 1}"], t[f"v{k + 1}"] = p[k], uv[k][0], uv[k][1]
        if n is not None:
            t[f"n{k + 1}"] = n[k]
    return t


def test_a_right_triangle_in_a_4x4_atlas_worked_by_hand():
    """UVs (0,0) (1,0) (0,1): a = (-0.5,-0.5) (3.5,-0.5) (-0.5,3.5); area = 4 * 4 = 16; the hypotenuse is x + y = 3, inclusive: ten texels.
    bx = 4 (x + 0.5) / 16, by = 4 (y + 0.5) / 16; positions (0,0,0) (4,0,0) (0,0,4) put texel (x, y) at (x + 0.5, 0, y + 0.5); the face
    normal is normalize(cross((4,0,-4), (4,0,0))) = (0,-1,0)."""
    t = _tri([(0, 0, 0), (4, 0, 0), (0, 0, 4)], [(0, 0), (1, 0), (0, 1)])
    a1, a2, a3 = AR.texel_vertices(t, 4, 4)
    assert a1.tolist() == [[-0.5, -0.5]] and a2.tolist() == [[3.5, -0.5]] and a3.tolist() == [[-0.5, 3.5]]
    area, s, degenerate = AR.orientation(t, 4, 4)
    assert area.tolist() == [16.0] and s.tolist() == [1.0] and not degenerate.any()
    owner, claims, per_tri = AR.cover(t, 4, 4, triangle_base=7)
    ys, xs = np.mgrid[0:4, 0:4]
    assert np.array_equal(owner != NONE, xs + ys <= 3) and (owner[owner != NONE] == 7).all() and per_tri.tolist() == [10] and claims.max() == 1
    smp = AR.samples(t, owner, 4, 4, triangle_base=7)
    inside = owner != NONE
    assert np.array_equal(smp["bx"][inside], ((xs + 0.5) / 4)[inside].astype(F)) and np.array_equal(smp["by"][inside], ((ys + 0.5) / 4)[inside].astype(F))
    assert not smp["zero"].any() and not smp["bx"][~inside].any() and not smp["by"][~inside].any()
    pts = AR.points(t, smp, IDENTITY, 1e-3, 9.0, triangle_base=7)
    assert np.array_equal(pts["position"][inside], np.stack([xs + 0.5, 0 * xs, ys + 0.5], -1)[inside].astype(F))
    assert np.array_equal(pts["normal"][inside], np.broadcast_to(F([0, -1, 0]), (10, 3)))
    assert (pts["near"][inside] == F(1e-3)).all() and (pts["far"][inside] == F(9.0)).all()
    assert not pts[~inside].view(np.uint32).any(), "an uncovered texel is 32 zero bytes"
    # the mirrored chart (vertices 2 and 3 exchanged): s = -1, the same texels, the weights exchanged with the vertices
    m = _tri([(0, 0, 0), (0, 0, 4), (4, 0, 0)], [(0, 0), (0, 1), (1, 0)])
    assert AR.orientation(m, 4, 4)[0].tolist() == [-16.0] and AR.orientation(m, 4, 4)[1].tolist() == [-1.0]
    owner_m = AR.cover(m, 4, 4, 7)[0]
    smp_m = AR.samples(m, owner_m, 4, 4, 7)
    assert np.array_equal(owner_m, owner) and np.array_equal(smp_m["bx"], smp["by"]) and np.array_equal(smp_m["by"], smp["bx"])
    assert np.array_equal(AR.points(m, smp_m, IDENTITY, 1e-3, 9.0, 7)["position"], pts["position"])
    assert np.array_equal(AR.points(m, smp_m, IDENTITY, 1e-3, 9.0, 7)["normal"][inside], np.broadcast_to(F([0, 1, 0]), (10, 3))), "the face normal follows the winding"


def test_degenerate_triangles_cover_nothing():
    good = _tri([(0, 0, 0), (4, 0, 0), (0, 0, 4)], [(0, 0), (1, 0), (0, 1)])
    for field, value in (("p2", np.nan), ("n3", np.inf), ("u1", -np.inf), ("v2", np.nan)):
        bad = good.copy()
        if bad[field].ndim == 2:
            bad[field][0, 1] = value
        else:
            bad[field] = value
        assert AR.orientation(bad, 4, 4)[2].all() and (AR.cover(bad, 4, 4)[0] == NONE).all(), field
    line = _tri([(0, 0, 0), (4, 0, 0), (2, 0, 0)], [(0, 0), (1, 1), (0.5, 0.5)])
    assert AR.orientation(line, 4, 4)[0].tolist() == [0.0] and (AR.cover(line, 4, 4)[0] == NONE).all()
    outside = _tri([(0, 0, 0), (4, 0, 0), (0, 0, 4)], [(2, 2), (3, 2), (2, 3)])
    assert not AR.orientation(outside, 4, 4)[2].any() and (AR.cover(outside, 4, 4)[0] == NONE).all(), "nothing wraps"
    partly = _tri([(0, 0, 0), (4, 0, 0), (0, 0, 4)], [(-1, -1), (1.25, -1), (-1, 1.25)])
    assert np.array_equal(AR.cover(partly, 4, 4)[0] != NONE, np.array([[True, False, False, False]] + [[False] * 4] * 3)), "a = (-4.5,-4.5) (4.5,-4.5) (-4.5,4.5): x + y <= 0 leaves texel (0, 0)"


def test_the_edge_value_is_antisymmetric_over_every_shared_edge_of_a_sphere():
    t = atlas.charts(scene.generate_sphere(16))
    shared = 0
    for W, H in ((64, 64), (65, 33), (7, 5)):
        a = np.stack(AR.texel_vertices(t, W, H), 1)                                      # (T, 3, 2)
        py, px = np.meshgrid(np.arange(H).astype(F), np.arange(W).astype(F), indexing="ij")
        walks = {}
        for i in range(len(t)):
            for k in range(3):
                P, Q = a[i, k], a[i, (k + 1) % 3]
                forth, back = AR.edge(P, Q, px, py), AR.edge(Q, P, px, py)
                assert np.array_equal(forth.view(np.uint32), (-back).view(np.uint32)), "the two walks of one edge are exact negatives, signed zeros included"
                walks[(P.tobytes(), Q.tobytes())] = forth
        for (P, Q), forth in walks.items():
            if (Q, P) in walks:                                                           # the neighbour walks it the other way
                shared += 1
                assert ((forth >= 0) | (walks[(Q, P)] >= 0)).all(), "a texel is refused by both sides of a shared edge"
    assert shared >= 3 * 2 * 200, shared


def test_adds_in_any_order_and_in_parts_are_one_add():
    t = atlas.charts(scene.generate_sphere(16))
    cube = atlas.charts(scene.generate_cube())
    both = np.concatenate([cube, t])
    for W, H in ((65, 33), (7, 5)):
        whole = AR.build([(IDENTITY, both)], W, H)
        parts = AR.build([(IDENTITY, cube), (IDENTITY, t)], W, H)
        for a, b in zip(whole, parts):
            assert a.tobytes() == b.tobytes()
        # the owner is a minimum over ids: taking the parts in the other order (with their ids) changes nothing
        sphere_first = np.minimum(AR.cover(t, W, H, len(cube))[0], AR.cover(cube, W, H, 0)[0])
        assert np.array_equal(sphere_first, whole[0]) and (whole[0] < len(cube)).all(), "the cube covers everything and has the lower ids"
        split = AR.build([(IDENTITY, t[:100]), (IDENTITY, t[100:])], W, H)
        one = AR.build([(IDENTITY, t)], W, H)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(split, one))


def test_dilation_of_a_hand_made_5x5_mask():
    """values at (0,0) = B and (2,2) = A.  Ring 1: the eight around (2,2) take A, except (1,1), whose first neighbour with a value in the
    order left, right, up, down, then the diagonals is (0,0): B; (1,0) and (0,1) take B.  Ring 2: (2,0) asks (1,0) first: B; every other
    texel reaches an A."""
    smp = np.zeros((5, 5), atlas.sample_dtype)
    smp["triangle"] = NONE
    smp["triangle"][0, 0], smp["triangle"][2, 2] = 3, 9
    rec = np.zeros((5, 5), np.dtype([("v", "<u4", 4)]))
    rec["v"] = np.arange(25, dtype=np.uint32).reshape(5, 5, 1) + 100                     # every texel starts with bytes of its own
    A, B = rec["v"][2, 2].copy(), rec["v"][0, 0].copy()
    out0, ring0 = AR.dilate(rec, smp, 0)
    assert out0.tobytes() == rec.tobytes() and np.array_equal(ring0 == 0, smp["triangle"] != NONE) and (ring0[ring0 != 0] == NONE).all()
    out1, ring1 = AR.dilate(rec, smp, 1)
    want1 = np.array([[0, 1, NONE, NONE, NONE], [1, 1, 1, 1, NONE], [NONE, 1, 0, 1, NONE], [NONE, 1, 1, 1, NONE], [NONE] * 5], np.uint32)
    assert np.array_equal(ring1, want1)
    is_b = np.zeros((5, 5), bool)
    is_b[0, 0] = is_b[0, 1] = is_b[1, 0] = is_b[1, 1] = True
    assert (out1["v"][is_b] == B).all() and (out1["v"][(want1 != NONE) & ~is_b] == A).all()
    assert np.array_equal(out1["v"][want1 == NONE], rec["v"][want1 == NONE]), "a texel still without a value keeps its bytes"
    out2, ring2 = AR.dilate(rec, smp, 2)
    assert np.array_equal(ring2, np.where(want1 == NONE, np.uint32(2), want1)) and (ring2 == 2).sum() == 13
    is_b[0, 2] = True
    assert (out2["v"][is_b] == B).all() and (out2["v"][~is_b] == A).all()
    out64, ring64 = AR.dilate(rec, smp, 64)
    assert out64.tobytes() == out2.tobytes() and np.array_equal(ring64, ring2), "a full atlas no longer changes"
    assert rec["v"][0, 1, 0] == 101, "the input is not changed"


def test_points_of_a_unit_scale_axis_aligned_instance_against_float64():
    """position: three products, two sums and the sum with the instance's position, on a unit sphere moved to where every coordinate lies
    in [2, 8): at most 3 * 2^-25 + 2 * 2^-25 + 2 * 2^-25 (b1) + half an ulp of the result, which is below 2 ulp of the result.  normal: two
    normalisations of a vector of about unit length, about 3 ulp of 1 each, and the interpolation: 16 * 2^-24 absolute."""
    t = atlas.charts(scene.generate_sphere(16))
    position = np.array([3, -5, 6], F)
    placement = (position, np.ones(3, F), np.array([1, 0, 0], F), np.array([0, 1, 0], F), np.array([0, 0, 1], F))
    owner, smp, pts = AR.build([(placement, t)], 65, 33)
    has = owner != NONE
    assert has.sum() == 1881
    tri = t[owner[has]]
    bx, by = smp["bx"][has].astype(np.float64)[:, None], smp["by"][has].astype(np.float64)[:, None]
    b1 = 1.0 - bx - by
    want = tri["p1"] * b1 + tri["p2"] * bx + tri["p3"] * by + position.astype(np.float64)
    err = np.abs(pts["position"][has].astype(np.float64) - want)
    ulp = np.spacing(np.abs(want).astype(F)).astype(np.float64)
    print(f"position: worst error {float((err / ulp).max()):.3f} ulp")
    assert (err <= 2 * ulp).all()
    n = tri["n1"] * b1 + tri["n2"] * bx + tri["n3"] * by
    n /= np.sqrt((n * n).sum(-1, keepdims=True))
    nerr = np.abs(pts["normal"][has].astype(np.float64) - n).max()
    print(f"normal: worst absolute error {nerr:.3e}")
    assert nerr <= 16 * 2.0**-24
    assert np.abs(np.sqrt((pts["normal"][has].astype(np.float64) ** 2).sum(-1)) - 1).max() < 4 * 2.0**-24


def test_a_scaled_rotated_instance_is_the_inverse_of_to_local():
    """under a rotation and the scale (2, 0.5, 3) the point is the world place of the local point and the normal stays perpendicular to the
    surface: for a sphere, normal_world ~ R (n / scale) normalised — held to float64 at 1e-6"""
    t = atlas.charts(scene.generate_sphere(16))
    c, s = np.cos(0.7), np.sin(0.7)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])                                     # columns: the images of x, y, z
    placement = (np.array([1, 2, 3], F), np.array([2, 0.5, 3], F), R[:, 0].astype(F), R[:, 1].astype(F), R[:, 2].astype(F))
    owner, smp, pts = AR.build([(placement, t)], 64, 64)
    has = owner != NONE
    tri = t[owner[has]]
    bx, by = smp["bx"][has].astype(np.float64)[:, None], smp["by"][has].astype(np.float64)[:, None]
    b1 = 1.0 - bx - by
    local = tri["p1"] * b1 + tri["p2"] * bx + tri["p3"] * by
    axes = np.stack([placement[2], placement[3], placement[4]], 1).astype(np.float64)
    want = (local * placement[1].astype(np.float64)) @ axes.T + placement[0].astype(np.float64)
    assert np.abs(pts["position"][has] - want).max() < 1e-5
    n = tri["n1"] * b1 + tri["n2"] * bx + tri["n3"] * by
    n /= np.sqrt((n * n).sum(-1, keepdims=True))
    wn = (n / placement[1].astype(np.float64)) @ axes.T
    wn /= np.sqrt((wn * wn).sum(-1, keepdims=True))
    assert np.abs(pts["normal"][has] - wn).max() < 1e-6


# charts, atlas -> (covered texels, texels claimed by more than one triangle, triangles covering nothing); measured on the CPU with these rules
COUNTS = [("cube", 64, 64, 4096, 4096, 0), ("cube", 65, 33, 2145, 2145, 0), ("sphere16", 64, 64, 3584, 0, 0), ("sphere16", 65, 33, 1881, 89, 0),
          ("sphere16", 7, 5, 33, 9, 178), ("sphere8", 65, 33, 1617, 81, 0), ("plane4", 64, 64, 2116, 8, 0), ("sphere16", 1, 1, 1, 1, 218)]
MESHES = dict(cube=scene.generate_cube, sphere16=lambda: scene.generate_sphere(16), sphere8=lambda: scene.generate_sphere(8), plane4=lambda: scene.generate_plane(4))


@pytest.mark.parametrize("name,W,H,covered,claimed,empty", COUNTS)
def test_coverage_counts(name, W, H, covered, claimed, empty):
    t = atlas.charts(MESHES[name]())
    assert len(t) == dict(cube=12, sphere16=224, sphere8=48, plane4=2)[name]
    owner, claims, per_tri = AR.cover(t, W, H)
    assert (int((owner != NONE).sum()), int((claims > 1).sum()), int((per_tri == 0).sum())) == (covered, claimed, empty)
    assert np.array_equal(owner != NONE, claims > 0)
    if name == "cube":
        assert (owner < 2).all(), "total overlap: the lowest id wins on every texel"
