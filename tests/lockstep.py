"""Lockstep comparison with the CPU oracle, one path segment per pixel at a time.

Between two passes the whole per-pixel state of the renderer is the accumulator, the path depth and the ray's origin, direction, material
and colour; the random numbers are re-derived each pass from (seed, pass, pixel, depth).  So the oracle can CONTINUE every pass from the
device's own state (OracleRenderer.adopt): each pass compares one path segment per pixel from bit-identical inputs, and a path that one
libm ulp moved across an edge cannot drag its later segments along.  Per pass every pixel is

  discrete  the new path depth, the new ray material or the finished-count increment differ;
  far       not discrete, and the accumulator's rgb increment, the new origin, direction or colour differ by more than
            1e-4 * max(|reference|, 1) in some component;
  exact     every compared value agrees bit for bit

(the rest is "close": within the tolerance, not bit-equal).  Pass 0 also compares the first-hit depth buffer bit for bit.

The bar a device is held to comes from the oracle itself: `standin_counts` runs the same lockstep with the libm stand-ins of
oracle/Makefile (every inexact libm result moved one ulp down, up, or one of the two per argument) in the device's place — the worst case
for a library accurate to one ulp.  `caps` turns that into the rule of tests/test_lockstep_gpu.py: per scene discrete + far may not exceed
2 x the largest stand-in count + 2; over a sweep 2 x the largest stand-in total + one segment per 100 000.  The factor 2 covers a library
two ulps off; the additive terms are there because the stand-ins' count is 0 on most scenes and one legitimate event must not fail a test.
"""
import numpy as np

import oracle

REL = 1e-4
STANDINS = ("lo", "hi", "mix")
STANDINS_2 = ("lo2", "hi2", "mix2")
CONTINUOUS = ("origin", "direction", "color")


class OracleDevice:
    """An OracleRenderer in the device's place: render(n), read_accum(), read_state(), read_depth() (and render_counted); reset(),
    ray_count() and pass_count() for tests/packaging_sweep.py."""

    def __init__(self, renderer, threads=1):
        self.renderer, self.threads = renderer, threads

    def render(self, n):
        self.renderer.render(n, threads=self.threads)

    def reset(self):
        self.renderer.reset()

    def ray_count(self):
        return self.renderer.traced_rays

    def pass_count(self):
        return self.renderer.passes

    def render_counted(self, n):
        return self.renderer.render(n, threads=self.threads, counted=True)

    def read_accum(self):
        return self.renderer.accum

    def read_state(self):
        return self.renderer.state

    def read_depth(self):
        return self.renderer.depth


def _bits_equal(a, b):
    return np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)


def _beyond(value, ref):
    """|value - ref| > REL * max(|ref|, 1), in float64; a NaN on either side is beyond unless the bits agree"""
    value, ref = np.asarray(value, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        return ~(np.abs(value - ref) <= REL * np.maximum(np.abs(ref), 1.0))


def lockstep(device, ref, passes, counted=False, records=8, threads=1):
    """`device` and the OracleRenderer `ref` (freshly reset, same scene) through `passes` passes, the oracle continuing each pass from the
    device's state.  Returns dict(segments, exact, far, discrete, depth_mismatch (pixels of pass 0 whose first-hit depth is not bit-equal),
    depth (device, ref) of pass 0, per_pass (the three counts of every pass), worst (printable records of up to `records` discrete / far segments), counters (per pass (device, ref)
    when counted)."""
    out = dict(segments=0, exact=0, far=0, discrete=0, depth_mismatch=0, worst=[], counters=[], per_pass=[])
    h, w = ref.h, ref.w
    prev_acc = np.zeros((h, w, 4), np.float32)
    prev_state = None
    for p in range(passes):
        if p:
            ref.adopt(prev_acc, prev_state, p)
        if counted:
            out["counters"].append((device.render_counted(1), ref.render(1, threads=threads, counted=True)))
        else:
            device.render(1), ref.render(1, threads=threads)
        acc, st = device.read_accum(), device.read_state()
        racc, rst = ref.accum, ref.state
        if p == 0:
            depth, rdepth = device.read_depth(), ref.depth
            out["depth"] = (depth, rdepth)
            out["depth_mismatch"] = int((~_bits_equal(depth, rdepth)).sum())
        before = prev_acc.astype(np.float64)
        inc, rinc = acc.astype(np.float64) - before, racc.astype(np.float64) - before
        with np.errstate(invalid="ignore"):
            discrete = (st["depth"] != rst["depth"]) | (st["material"] != rst["material"]) | ~(inc[..., 3] == rinc[..., 3])
        far = _beyond(inc[..., :3], rinc[..., :3]).any(-1)
        exact = _bits_equal(acc, racc).all(-1) & (st["depth"] == rst["depth"]) & (st["material"] == rst["material"])
        for k in CONTINUOUS:
            far |= _beyond(st[k], rst[k]).any(-1)
            exact &= _bits_equal(st[k], rst[k]).all(-1)
        far &= ~discrete
        out["segments"] += h * w
        out["exact"] += int(exact.sum())
        out["far"] += int(far.sum())
        out["discrete"] += int(discrete.sum())
        out["per_pass"].append(dict(exact=int(exact.sum()), far=int(far.sum()), discrete=int(discrete.sum())))
        for kind, mask in (("discrete", discrete), ("far", far)):
            for y, x in zip(*np.nonzero(mask)):
                if len(out["worst"]) >= records:
                    break
                rec = {"pass": p, "pixel": (int(x), int(y)), "kind": kind}
                if prev_state is not None:
                    rec["input"] = {k: prev_state[k][y, x].tolist() for k in prev_state}
                rec["device"] = dict({k: st[k][y, x].tolist() for k in st}, increment=inc[y, x].tolist())
                rec["oracle"] = dict({k: rst[k][y, x].tolist() for k in rst}, increment=rinc[y, x].tolist())
                out["worst"].append(rec)
        prev_acc, prev_state = acc, st
    return out


def describe(result):
    """the offending segments of a lockstep result, one block per segment"""
    lines = []
    for rec in result["worst"]:
        lines.append(f"pass {rec['pass']} pixel {rec['pixel']} {rec['kind']}")
        for side in ("input", "device", "oracle"):
            if side in rec:
                lines.append(f"  {side:7s} " + ", ".join(f"{k}={v}" for k, v in rec[side].items()))
    return "\n".join(lines)


def bad(result):
    return result["far"] + result["discrete"]


_STANDIN = {}


def flat_scene(scene):
    """(FlatScene, hiprz_camera, hiprz_config, World, RenderConfig) of a scene of either module: a name is one of
    tests/tree_shape_scenes.py, anything else a seed (or a derived scene) of tests/generated_scenes.py"""
    if isinstance(scene, str):
        import tree_shape_scenes
        return tree_shape_scenes.flat_scene(scene)
    import generated_scenes
    return generated_scenes.flat_scene(scene)


def standin_counts(seed, mode=0, passes=None, names=STANDINS, threads=1):
    """{stand-in: lockstep result} of sweep scene `seed` (or of the scene named `seed`, see flat_scene) with each libm stand-in in the
    device's place, against the plain oracle in `mode`; computed once per (seed, mode, stand-in).  `threads` only shortens the wait:
    the oracle's frames do not depend on it."""
    import generated_scenes
    passes = passes or generated_scenes.PASSES
    flat, cam, cfg = flat_scene(seed)[:3]
    out = {}
    for name in names:
        key = (seed, mode, passes, name)
        if key not in _STANDIN:
            dev = oracle.OracleRenderer(flat, cam, cfg, lib=oracle.variant(name), mode=mode)
            ref = oracle.OracleRenderer(flat, cam, cfg, mode=mode)
            result = lockstep(OracleDevice(dev, threads=threads), ref, passes, records=0, threads=threads)
            dev.close(), ref.close()
            result.pop("depth", None)
            _STANDIN[key] = result
        out[name] = _STANDIN[key]
    return out


def scene_cap(seed, mode=0, passes=None, threads=1):
    """discrete + far segments a device may show on one scene: 2 x the largest count of a one-ulp stand-in, plus 2"""
    return 2 * max(bad(r) for r in standin_counts(seed, mode, passes, threads=threads).values()) + 2


def sweep_cap(seeds, mode=0, passes=None):
    """... and over a sweep: 2 x the largest sweep total of a one-ulp stand-in, plus one segment per 100 000"""
    totals = {name: 0 for name in STANDINS}
    segments = 0
    for seed in seeds:
        counts = standin_counts(seed, mode, passes)
        for name in STANDINS:
            totals[name] += bad(counts[name])
        segments += counts[STANDINS[0]]["segments"]
    return 2 * max(totals.values()) + segments // 100000
