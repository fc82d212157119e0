"""What tests/test_packaging_sweep_gpu.py compares, free of anything that needs a GPU: a renderer (rayzath_amd.engine.Context, or
lockstep.OracleDevice in its place) takes one scene through 8 passes in several call patterns, and after every call that ends on a pass
count the pass-by-pass render kept, everything that describes the frame — accumulator, first-hit depth, every field of the path state,
ray and pass counters — is compared with it bit for bit.  tests/test_lockstep_oracle.py drives the same functions with the oracle."""
import numpy as np

PASSES = 8
KEPT = (1, 3, 8)                          # pass counts at which the pass-by-pass render is kept
PATTERNS = ((8,), (1, 2, 5), (3, 5))      # render calls of a variant: every prefix sum that is in KEPT is compared


def snapshot(device):
    """everything that describes the frame of `device` now: {name: array or int}"""
    out = dict(accum=np.array(device.read_accum()), depth=np.array(device.read_depth()), rays=int(device.ray_count()), passes=int(device.pass_count()))
    for k, v in device.read_state().items():
        out["state." + k] = np.array(v)
    return out


def render_calls(device, calls):
    """`device` (a frame about to restart: freshly uploaded, or reset) through render(n) for n in `calls`: {passes so far: snapshot} at KEPT"""
    out, done = {}, 0
    for n in calls:
        device.render(n)
        done += n
        if done in KEPT:
            out[done] = snapshot(device)
    return out


def pass_by_pass(device):
    """the baseline: render(1) PASSES times"""
    return render_calls(device, (1,) * PASSES)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    # np.array_equal; a NaN (unequal to itself) passes only where the two hold the same bits
    return bool(np.array_equal(a, b) or np.array_equal(a.view(np.uint8), b.view(np.uint8)))


def differences(got, want):
    """[(passes, name, differing elements)] between two results of render_calls: every snapshot of `got` against `want`'s of the same
    pass count; empty when everything is equal bit for bit"""
    out = []
    for passes, snap in got.items():
        ref = want[passes]
        assert set(snap) == set(ref), (sorted(snap), sorted(ref))
        for name, value in snap.items():
            if isinstance(value, int):
                if value != ref[name]:
                    out.append((passes, name, f"{value} != {ref[name]}"))
            elif not _same_bits(value, ref[name]):
                n = int((value != ref[name]).sum()) if value.shape == ref[name].shape else -1
                out.append((passes, name, f"{n} of {value.size} elements"))
    return out


def compare_patterns(device, want, patterns=PATTERNS):
    """`device` (holding the scene, frame about to restart) through every call pattern against `want` (pass_by_pass of the baseline):
    [(pattern, passes, name, what)], empty when every pattern gives the baseline's frames"""
    out = []
    for k, calls in enumerate(patterns):
        if k:
            device.reset()
        got = render_calls(device, calls)
        assert set(got) == {n for n in np.cumsum(calls).tolist() if n in KEPT} and PASSES in got, calls
        out += [(calls, *d) for d in differences(got, want)]
    return out
