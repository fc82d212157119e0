"""Probe placement on the CPU (include/hiprz_place.h): the numpy float32 restatement (tests/place_reference.py) on the scene the feature was
asked for — the two rooms of tests/field_reference.py 0.2 apart under a (5, 2, 2) grid of step 0.8, whose four probes at x = 0 stand in
the gap — with an analytic float64 caster that also answers from outside a room, on synthetic verdicts that force one case each, and the
mutants, every one of which must differ.  No GPU: the library is loaded for its pure host calls only.

THE SCENE is the issue's, unchanged: lo (-1.6, 0.5, -0.5), hi (1.6, 1.5, 0.5), shape (5, 2, 2); min_front 0.2, reach 4, max_offset 0.36
per axis, iterations 4, K = 64, S = 1, max_back K // 4 = 16.  Under the reference alone the four gap probes start INSIDE (54 to 56 of their 64
rays see the back of a room's wall), leave the gap with their first move and end NEAR, 0.19 from the wall, within the bound."""
import numpy as np
import pytest

import bake_reference as BR
import field_reference as FR
import place_reference as PL
from rayzath_amd import bake, place, probe

F = np.float32


def _classify(params):
    p = params.copy()
    p["iterations"] = 0
    return p


def test_the_caster_from_inside_outside_and_along_the_gap():
    cast = PL.room_caster()
    o = [(-1.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 3.0, 0.0), (0.0, 1.0, 0.0)]
    d = [(1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.6, -0.8, 0.0), (0.0, 0.0, 0.0)]
    rays = np.zeros((1, 6), PL.ray_dtype)
    rays["origin"], rays["direction"], rays["near"], rays["far"] = o, d, 1e-3, 1e3
    found, front, t = cast(rays)
    assert found[0].tolist() == [True, True, True, False, True, False], "inside; from the gap both ways; along the gap: a miss; from above; an invalid ray"
    assert front[0].tolist() == [True, False, False, False, False, False], "from outside a room the wall shows its back"
    assert np.allclose(t[0, [0, 1, 2]], [0.9, 0.1, 0.1]) and np.isclose(t[0, 4], 1.25)
    # inside a room the caster is field_reference.room_distances
    grid, probes, table, params = PL.gap_scene()
    flat = probes.reshape(-1)
    inside = np.abs(flat["position"][:, 0]) > 0.2
    rays = BR.rays(flat, table, 0)
    found, front, t = cast(rays)
    assert found[inside].all() and front[inside].all()
    assert np.array_equal(t[inside], FR.room_distances(flat["position"], rays["direction"])[inside].astype(F))


def test_the_gap_probes_leave_the_gap(built):
    grid, probes, table, params = PL.gap_scene()
    flat, cast = probes.reshape(-1), PL.room_caster()
    in_gap = flat["position"][:, 0] == 0.0
    assert in_gap.sum() == 4 and params["max_back"] == 16
    _, before = PL.place(flat, table, 0, _classify(params), cast)
    assert (place.state(before)[in_gap] == place.INSIDE).all(), "the gap probes start INSIDE"
    assert (place.state(before)[~in_gap] == place.CLEAR).all() and not before["offset"].view(np.uint32).any() and (place.moves(before) == 0).all()
    print("back-face rays of the gap probes:", before["n_back"][in_gap].tolist())
    trail = []
    moved, records = PL.place(flat, table, 0, params, cast, trail=trail)
    state = place.state(records)
    assert (state[in_gap] != place.INSIDE).all(), "a gap probe is still INSIDE"
    assert (np.abs(records["offset"]) <= params["max_offset"]).all(), "an offset beyond the bound"
    assert (np.abs(moved["position"][in_gap, 0]) > 0.1).all(), "a gap probe did not reach a room"
    assert (place.moves(records)[in_gap] >= 1).all() and (records["n_back"][in_gap] == 0).all()
    # probes that start CLEAR keep offset +0 exactly, and every byte of the probe
    assert not records["offset"][~in_gap].view(np.uint32).any() and moved[~in_gap].tobytes() == flat[~in_gap].tobytes()
    assert (records["word"][~in_gap] == place.CLEAR).all()
    # the position is H + o, the other 20 bytes are the probe's
    assert np.array_equal(moved["position"][in_gap], flat["position"][in_gap] + records["offset"][in_gap])
    for name in ("near", "normal", "far"):
        assert moved[name].tobytes() == flat[name].tobytes()
    # at most iterations + 1 evaluations, and the rays of each are bake_reference.rays' for a probe that stands where the loop had it
    assert len(trail) <= int(params["iterations"]) + 1
    for rays, live in trail:
        at = flat.copy()
        at["position"] = rays["origin"][:, 0]
        assert rays.tobytes() == BR.rays(at, table, 0).tobytes()
    # the reported state is that of an evaluation at the final position
    _, again = PL.place(moved, table, 0, _classify(params), cast)
    assert np.array_equal(place.state(again), state)
    for name in ("front", "back", "n_back", "n_front"):
        assert again[name].tobytes() == records[name].tobytes()
    print("offsets of the gap probes:", records["offset"][in_gap].tolist(), "states", state[in_gap].tolist(), "moves", place.moves(records)[in_gap].tolist())


def test_iterations_bound_the_moves_and_an_invalid_probe_is_copied(built):
    grid, probes, table, params = PL.gap_scene()
    flat, cast = probes.reshape(-1).copy(), PL.room_caster()
    flat["normal"][7] = 0.0
    for iterations in (0, 1, 4):
        p = params.copy()
        p["iterations"] = iterations
        trail = []
        moved, records = PL.place(flat, table, 0, p, cast, trail=trail)
        assert len(trail) <= iterations + 1 and (place.moves(records) <= iterations).all()
        assert records["word"][7] == place.INVALID and not records[7].tobytes()[:12].strip(b"\0") and not records[7].tobytes()[16:].strip(b"\0")
        assert moved[7].tobytes() == flat[7].tobytes()
        assert place.state(records)[7] == place.INVALID and place.moves(records)[7] == 0


def _table_caster(found, front, t):
    """verdicts that do not depend on where the probe stands: (K,) each, for one probe"""
    return lambda rays: (np.broadcast_to(np.asarray(found, bool), rays.shape).copy(), np.broadcast_to(np.asarray(front, bool), rays.shape).copy(),
                         np.broadcast_to(np.asarray(t, F), rays.shape).copy())


def _one_probe():
    return bake.points([(0.25, -0.5, 1.0)], [(0.3, 1.0, -0.2)], 1e-3, 1e3)


def _differs(probes, table, params, cast, mutant):
    want, got = PL.place(probes, table, 0, params, cast), PL.place(probes, table, 0, params, cast, mutant)
    return want[0].tobytes() != got[0].tobytes() or want[1].tobytes() != got[1].tobytes()


def test_every_mutant_differs(built):
    K = 128
    table = probe.sphere_directions(K, 1)
    probes = _one_probe()
    d = PL.directions(probes, table, 0)[0]
    yes, no = np.ones(K, bool), np.zeros(K, bool)
    params = place.params(0.2, 4.0, 0.36, 4, K // 4)
    caught = {}
    # ties_high: equal distances at k and k + 64 — the nearest front face at 3 and 67, the farthest at every other ray
    t = np.full(K, 1.0, F)
    t[[3, 67]] = 0.05
    e = PL.evaluate(yes[None], yes[None], t[None], params)
    assert e["F"][1][0] == 3 and e["O"][1][0] == 0 and e["state"][0] == place.NEAR
    assert PL.evaluate(yes[None], yes[None], t[None], params, "ties_high")["F"][1][0] == 67
    caught["ties_high"] = _differs(probes, table, params, _table_caster(yes, yes, t), "ties_high")
    # no_open: one near front face, two far ones, the sky everywhere else — O is the first ray of the sky
    found = no.copy()
    found[[5, 90, 91]] = True
    t = np.where(np.arange(K) == 5, F(0.05), F(0.5)).astype(F)
    e = PL.evaluate(found[None], found[None], t[None], params)
    assert e["O"][1][0] == 0 and e["O"][2][0] == F(4.0) and PL.evaluate(found[None], found[None], t[None], params, "no_open")["O"][1][0] == 90
    caught["no_open"] = _differs(probes, table, params, _table_caster(found, found, t), "no_open")
    # length: an INSIDE probe whose nearest back face lies along a diagonal, 0.4 away: the step of 0.5 stays within 0.36 on every axis
    k = int(np.abs(d).max(1).argmin())
    assert np.abs(d[k]).max() * 0.5 < 0.36 < 0.5
    t = np.full(K, 1.0, F)
    t[k] = 0.4
    moved, records = PL.place(probes, table, 0, params, _table_caster(yes, no, t))
    assert place.moves(records)[0] >= 1 and np.sqrt((records["offset"][0].astype(np.float64) ** 2).sum()) > 0.36
    caught["length"] = _differs(probes, table, params, _table_caster(yes, no, t), "length")
    # uncapped: the nearest back face beyond the reach
    short = place.params(0.2, 0.3, 0.36, 4, K // 4)
    caught["uncapped"] = _differs(probes, table, short, _table_caster(yes, no, t), "uncapped")
    # full_step: any INSIDE move
    t = np.full(K, 1.0, F)
    t[k] = 0.05
    caught["full_step"] = _differs(probes, table, params, _table_caster(yes, no, t), "full_step")
    assert set(caught) == set(PL.MUTANTS) and all(caught.values()), caught
    # and the scene itself tells the mutants that its cases reach
    grid, gprobes, gtable, gparams = PL.gap_scene()
    on_scene = {m: _differs(gprobes.reshape(-1), gtable, gparams, PL.room_caster(), m) for m in PL.MUTANTS}
    print("mutants the gap scene tells apart:", on_scene)
    assert on_scene["full_step"]


def test_stuck_by_the_bound_and_by_the_open_direction(built):
    K = 64
    table = probe.sphere_directions(K, 1)
    probes = _one_probe()
    d = PL.directions(probes, table, 0)[0]
    yes, no = np.ones(K, bool), np.zeros(K, bool)
    # a back face 0.5 away along a ray: the step of 0.6 leaves the box on some axis — STUCK, no move, offset +0
    t = np.full(K, 0.5, F)
    moved, records = PL.place(probes, table, 0, place.params(0.2, 4.0, 0.3, 4, 16), _table_caster(yes, no, t))
    assert records["word"][0] == place.INSIDE | place.STUCK and not records["offset"].view(np.uint32).any() and moved.tobytes() == probes.tobytes()
    assert records["n_back"][0] == K and records["back"][0] == F(0.5) and records["front"][0] == F(4.0)
    # NEAR with the most open direction next to the nearest front face: rays 0 and 1 of a sphere table are 13 degrees apart
    t = np.full(K, 0.1, F)
    t[0], t[1] = 3.0, 0.05
    assert (d[0] * d[1]).sum() > 0.5
    moved, records = PL.place(probes, table, 0, place.params(0.2, 4.0, 0.3, 4, 16), _table_caster(yes, yes, t))
    assert records["word"][0] == place.NEAR | place.STUCK and moved.tobytes() == probes.tobytes() and records["front"][0] == F(0.05)
    # ... and away from it: ray 63 looks the other way; the step is min(min_front - r_F, 0.5 r_O) along it, once per move until CLEAR never comes
    t[0], t[63] = 0.1, 0.2
    moved, records = PL.place(probes, table, 0, place.params(0.2, 4.0, 0.3, 1, 16), _table_caster(yes, yes, t))
    step = min(F(0.2) - F(0.05), F(0.5) * F(0.2))
    assert records["word"][0] == place.NEAR | (1 << 16) and records["offset"][0].tobytes() == (d[63] * step).astype(F).tobytes()


def test_params_and_their_defaults(built):
    from rayzath_amd import field
    grid = field.grid_of(PL.GAP_LO, PL.GAP_HI, PL.GAP_SHAPE)
    p = place.params_for(grid, 0.2, 4.0)
    rec = place._params(p, 256)
    assert rec["max_back"] == 64 and rec["iterations"] == 4 and rec["max_offset"].tobytes() == (F(0.45) * grid["step"]).astype(F).tobytes()
    assert place._params(place.params(0.2, 4.0, (0.1, 0.2, 0.3), 2, 7), 256)["max_back"] == 7
    assert place._params(dict(min_front=0.2, reach=4.0, max_offset=0.1), 64)["max_back"] == 16
    for bad in (dict(min_front=0.0), dict(min_front=np.nan), dict(reach=-1.0), dict(reach=np.inf), dict(max_offset=-0.1), dict(max_offset=(0.1, np.nan, 0.1)), dict(iterations=17)):
        with pytest.raises(ValueError):
            place.params(**{**dict(min_front=0.2, reach=4.0, max_offset=0.1), **bad})
    records = np.zeros(3, place.record_dtype)
    records["word"] = (place.INSIDE | place.STUCK | (3 << 16), place.INVALID, place.NEAR)
    assert place.state(records).tolist() == [place.INSIDE, place.INVALID, place.NEAR] and place.moves(records).tolist() == [3, 0, 0]
