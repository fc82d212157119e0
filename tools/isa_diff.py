#!/usr/bin/env python3
"""Static comparison of two sets of gfx950 assembly files written by tools/isa.sh (one <unit>.s per device unit in each directory):
which kernels have the same body instruction for instruction (labels renumbered, comments dropped), and for those that differ the
static counts, VGPRs, scratch bytes and spilled VGPRs of both sides.  For the flagship resident kernel also where its scratch
instructions sit relative to the walk's barriers (the last four s_barrier before the kernel's final one).
usage: tools/isa_diff.py <parent dir> <branch dir> [flagship mangled-name prefix ...]"""
import glob, os, re, sys


def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    meta = {}
    for block in re.split(r"^\s*- \.agpr_count:", text, flags=re.M)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            grab = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1)) if re.search(rf"\.{key}:\s+(\d+)", block) else 0
            meta[name.group(1)] = {"vgpr": grab("vgpr_count"), "scratch": grab("private_segment_fixed_size"), "spilled": grab("vgpr_spill_count")}
    out = {}
    lines = text.split("\n")
    known, starts = set(names), {}
    for i, l in enumerate(lines):
        head = l.split(";")[0].strip()
        if head.endswith(":") and head[:-1] in known:
            starts[head[:-1]] = i
    for name in names:
        body, labels = [], {}
        for l in lines[starts[name] + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";")[0].strip()
            if not l or (l.startswith(".") and not l.startswith(".LBB")):
                continue
            l = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), l)
            body.append(l)
        out[name] = (body, meta.get(name, {}))
    return out


def counts(body):
    ins = [l for l in body if not l.endswith(":")]
    n = lambda pat: sum(1 for l in ins if re.match(pat, l))
    return {"instr": len(ins), "valu": n(r"v_"), "ds": n(r"ds_"), "gload": n(r"global_load"), "scratch_ops": n(r"scratch_(load|store)"),
            "div_fixup": n(r"v_div_fixup"), "v_sqrt": n(r"v_sqrt"), "v_rcp": n(r"v_rcp")}


def walk(body):
    bars = [i for i, l in enumerate(body) if l.startswith("s_barrier")]
    ops = [i for i, l in enumerate(body) if re.match(r"scratch_(load|store)", l)]
    if len(bars) < 5:
        return f"body {len(body)} lines, {len(bars)} barriers, scratch-ops at {ops}"
    w = bars[-5:-1]
    return (f"body {len(body)} lines, walk barriers at {w}: scratch-ops before {sum(i < w[0] for i in ops)}, between the walk's first and last "
            f"barrier {sum(w[0] <= i <= w[-1] for i in ops)}, behind {sum(i > w[-1] for i in ops)} (at {[i for i in ops if i > w[-1]]})")


parent_dir, branch_dir, flagships = sys.argv[1], sys.argv[2], sys.argv[3:]
differ = []
print("== per unit: kernels whose bodies are the parent's, instruction for instruction")
for path in sorted(glob.glob(os.path.join(branch_dir, "*.s"))):
    unit = os.path.basename(path)[:-2]
    b, p = kernels(path), kernels(os.path.join(parent_dir, unit + ".s"))
    same = [k for k in b if k in p and b[k][0] == p[k][0]]
    print(f"{unit}: {len(b)} kernels, {len(same)} identical to the parent's, {len(b) - len(same)} differ" + ("" if set(b) == set(p) else "  (the kernel SETS differ)"))
    differ += [(unit, k, p.get(k), b[k]) for k in b if k not in same]
for unit, k, p, b in differ:
    if any(k.startswith(f) for f in flagships):
        print(f"== {k[:70]}")
        for side, v in (("parent", p), ("branch", b)):
            print(f"   {side}: {walk(v[0])}")
print("== all kernels that differ: parent / branch")
for unit, k, p, b in differ:
    print(f"   {unit} {k[:70]}")
    if p:
        print(f"      parent {counts(p[0])} {p[1]}")
    print(f"      branch {counts(b[0])} {b[1]}")
