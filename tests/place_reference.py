"""Probe placement (include/hiprz_place.h) restated in numpy float32, one rounding per operation like the device build
(-ffp-contract=off): the evaluation of a probe by its K rays, the three selections with their ties, the state, and the loop that moves a
probe.  The rays are hiprz_bake.h's (tests/bake_reference.py) from the probe's current position; what each ray hits comes from a caller's
`cast(rays) -> (found, front, t)` — Context.trace on the GPU (tests/test_place_gpu.py, which holds the device's probes and records to
place() in every byte), an analytic scene or a synthetic table on the CPU (tests/test_place_reference.py).

MUTANTS, each a wrong reading of the header that the tests must tell from the right one:
  ties_high   ties of a selection go to the highest k
  no_open     O is chosen among the FRONT rays alone: the OPEN ones are kept out
  length      the offset is bounded by its length (against the largest max_offset) instead of per axis
  uncapped    r = t, not min(t, reach)
  full_step   the INSIDE step is r_B + min_front: the 0.5 is dropped"""
import numpy as np

import bake_reference as BR
import field_reference as FR
from rayzath_amd.bake import point_dtype
from rayzath_amd.place import CLEAR, INSIDE, INVALID, NEAR, STUCK, params_dtype, record_dtype
from rayzath_amd.query import HIT_EXTERNAL, HIT_FOUND, ray_dtype

F = np.float32
U64 = np.uint64
NONE = U64(0xFFFFFFFFFFFFFFFF)
MUTANTS = ("ties_high", "no_open", "length", "uncapped", "full_step")


def directions(probes, table, seed):
    """the directions (n, K, 3) float32 of the probes' rays: bake_reference.rays()'s, which depend on the normal alone (+0 for an invalid
    probe)"""
    return BR.rays(probes, table, seed)["direction"].astype(F)


def rays_from(probes, position, d):
    """the rays (n, K) of the 1-d `probes` standing at `position` (n, 3): origin = position, the probe's near, direction d, the probe's far"""
    out = np.zeros(d.shape[:2], ray_dtype)
    out["origin"], out["near"], out["far"] = position[:, None, :], probes["near"][:, None], probes["far"][:, None]
    out["direction"] = d
    return out


def trace_caster(trace):
    """cast() over a closest-hit query (Context.trace): hits of query.hit_dtype -> (found, front, t)"""
    def cast(rays):
        hits = trace(rays)
        found = (hits["flags"] & HIT_FOUND) != 0
        return found, found & ((hits["flags"] & HIT_EXTERNAL) != 0), hits["t"].astype(F)
    return cast


def _least(r_bits, mask, K, complement, mutant):
    """the least key per row among the rays of `mask`: ((~)bits of r << 32) | k.  (exists, k): ties go to the lowest k"""
    k = np.arange(K, dtype=U64)[None, :]
    low = (U64(K - 1) - k) if mutant == "ties_high" else k
    high = (~r_bits if complement else r_bits).astype(np.uint32).astype(U64)
    keys = np.where(mask, (high << U64(32)) | low, NONE)
    best = keys.min(1)
    at = (best & U64(0xFFFFFFFF)).astype(np.int64)
    if mutant == "ties_high":
        at = (K - 1) - at
    exists = best != NONE
    return exists, np.where(exists, at, 0)


def evaluate(found, front, t, params, mutant=None):
    """ "ONE EVALUATION AT P" for (n, K) verdicts: a dict of state, n_back, n_front, front, back (the record's), and per selection B, F,
    O whether it exists, its k and its r"""
    reach = F(params["reach"])
    found, front = np.asarray(found, bool), np.asarray(front, bool) & np.asarray(found, bool)
    n, K = found.shape
    t = np.asarray(t, F)
    with np.errstate(invalid="ignore"):
        r = np.where(found, t if mutant == "uncapped" else np.minimum(t, reach), reach).astype(F)
    bits = r.view(np.uint32)
    is_back, is_open = found & ~front, ~found
    out = {"n_back": is_back.sum(1).astype(np.uint32), "n_front": front.sum(1).astype(np.uint32)}
    rows = np.arange(n)
    for name, mask, complement in (("B", is_back, False), ("F", front, False), ("O", front if mutant == "no_open" else (front | is_open), True)):
        exists, k = _least(bits, mask, K, complement, mutant)
        out[name] = (exists, k, r[rows, k])
    out["front"] = np.where(out["F"][0], out["F"][2], reach).astype(F)
    out["back"] = np.where(out["B"][0], out["B"][2], reach).astype(F)
    near = out["F"][0] & (out["F"][2] < F(params["min_front"]))
    out["state"] = np.where(out["n_back"] > params["max_back"], INSIDE, np.where(near, NEAR, CLEAR)).astype(np.uint32)
    return out


def place(probes, table, seed, params, cast, mutant=None, trail=None):
    """(moved probes, records) hiprz_place_probes writes for 1-d `probes` under `table` ((S, K, 4) float32): point_dtype and record_dtype
    (n,).  cast(rays (m, K) ray_dtype) -> (found, front, t), (m, K) each, is given the rays of the probes that are still moving.  trail: a
    list that receives (rays of all n probes, live) of every evaluation."""
    params = np.asarray(params).reshape(())
    assert params.dtype == params_dtype
    p = np.ascontiguousarray(probes).reshape(-1).view(point_dtype)
    n = len(p)
    ok = BR.valid(p).reshape(-1)
    d = directions(p, table, seed)
    H = p["position"].astype(F)
    P, o = H.copy(), np.zeros((n, 3), F)
    moves, stuck = np.zeros(n, np.uint32), np.zeros(n, bool)
    rec = {k: np.zeros(n, t) for k, t in (("state", np.uint32), ("n_back", np.uint32), ("n_front", np.uint32), ("front", F), ("back", F))}
    live = ok.copy()
    min_front, max_offset, half = F(params["min_front"]), params["max_offset"].astype(F), F(0.5)
    rows = np.arange(n)
    for _ in range(int(params["iterations"]) + 1):
        if not live.any():
            break
        rays = rays_from(p, P, d)
        if trail is not None:
            trail.append((rays, live.copy()))
        found, front, t = np.zeros(rays.shape, bool), np.zeros(rays.shape, bool), np.zeros(rays.shape, F)
        found[live], front[live], t[live] = cast(rays[live])
        e = evaluate(found, front, t, params, mutant)
        for k in rec:
            rec[k] = np.where(live, e[k], rec[k])
        live = live & (moves != params["iterations"]) & (e["state"] != CLEAR)
        (_, kb, rb), (has_f, kf, rf), (has_o, ko, ro) = e["B"], e["F"], e["O"]
        d_b, d_f, d_o = d[rows, kb], d[rows, kf], d[rows, ko]
        inside = e["state"] == INSIDE
        with np.errstate(all="ignore"):
            step_in = rb + ((F(1.0) if mutant == "full_step" else half) * min_front)
            dot = (d_o[:, 0] * d_f[:, 0] + d_o[:, 1] * d_f[:, 1]) + d_o[:, 2] * d_f[:, 2]
            away = has_o & (dot <= half)
            step_near = np.minimum(min_front - rf, half * ro)
            m = np.where(inside[:, None], d_b * step_in[:, None], d_o * step_near[:, None]).astype(F)
            gives_up = live & ~inside & ~away
            stuck |= gives_up
            live = live & ~gives_up
            to = (o + m).astype(F)
            if mutant == "length":
                beyond = np.sqrt((to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1]) + to[:, 2] * to[:, 2]) > max_offset.max()
            else:
                beyond = (np.abs(to) > max_offset[None, :]).any(1)
            stuck |= live & beyond
            live = live & ~beyond
            o = np.where(live[:, None], to, o)
            P = np.where(live[:, None], H + o, P).astype(F)
        moves = moves + live.astype(np.uint32)
    moved = p.copy()
    moved["position"][ok] = P[ok]
    records = np.zeros(n, record_dtype)
    records["offset"], records["front"], records["back"], records["n_back"], records["n_front"] = o, rec["front"], rec["back"], rec["n_back"], rec["n_front"]
    records["word"] = rec["state"] | np.where(stuck, np.uint32(STUCK), np.uint32(0)) | (moves << np.uint32(16))
    records[~ok] = np.zeros((), record_dtype)
    records["word"][~ok] = INVALID
    return moved, records


# --- the two rooms of tests/field_reference.py, seen from anywhere: the rooms are inward boxes, so from outside a room a ray sees the BACK
# of the face it enters through, from inside the FRONT of the face it leaves through; a ray along the gap between them misses ---
GAP_LO, GAP_HI, GAP_SHAPE = (-1.6, 0.5, -0.5), (1.6, 1.5, 0.5), (5, 2, 2)
GAP_PARAMS = dict(min_front=0.2, reach=4.0, max_offset=0.36, iterations=4)


def room_caster(rooms=FR.ROOMS):
    """cast() for closed inward boxes in float64: the nearest box face within (near, far) of each ray"""
    def cast(rays):
        o, d = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64)
        near, far = rays["near"].astype(np.float64), rays["far"].astype(np.float64)
        valid = np.isfinite(o).all(-1) & (np.abs((d * d).sum(-1) - 1.0) <= 0.01)
        best, front = np.full(o.shape[:-1], np.inf), np.zeros(o.shape[:-1], bool)
        for lo, hi in rooms:
            lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
            with np.errstate(all="ignore"):
                ta, tb = (lo - o) / d, (hi - o) / d
                t0, t1 = np.fmin(ta, tb), np.fmax(ta, tb)
                parallel_out = ((d == 0) & ((o < lo) | (o > hi))).any(-1)
                t0, t1 = np.where(d == 0, -np.inf, t0).max(-1), np.where(d == 0, np.inf, t1).min(-1)
            crosses = ~parallel_out & (t0 <= t1)
            for t, is_front in ((t0, False), (t1, True)):          # entering: the face's back; leaving: its front
                hit = crosses & (t > near) & (t < far) & (t < best)
                best, front = np.where(hit, t, best), np.where(hit, is_front, front)
        found = valid & np.isfinite(best)
        return found, found & front, np.where(found, best, 0.0).astype(F)
    return cast


def gap_scene(K=64, S=1):
    """(grid, probes (5, 2, 2), table, params) of the scene the issue sets: the four probes at x = 0 stand in the 0.2 gap between the rooms"""
    from rayzath_amd import field, place, probe
    probes = probe.grid(GAP_LO, GAP_HI, GAP_SHAPE, near=1e-3, far=1e3)
    return field.grid_of(GAP_LO, GAP_HI, GAP_SHAPE), probes, probe.sphere_directions(K, S), place.params(**GAP_PARAMS, max_back=K // 4)
