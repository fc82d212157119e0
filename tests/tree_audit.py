"""Invariants of one downloaded mesh tree, in numpy (no GPU, no library call).

audit(nodes, root, tris, kind, tri_first, n_tris, ...) returns a list of findings — empty when the tree is sound:

  exact boxes   every box equals the exact min / max over v1, v2, v3 of the triangles below it (min and max are exact in fp32: the
                comparison is == on values; -0 and +0 are the same value)
  leaf sizes    at most 4 (Morton) / `leaf_max` = 8 (SAH); Morton: no inner node with 4 or fewer triangles below it
  tiling        every walk ends inside the table and the leaves tile [tri_first, tri_first + n_tris) exactly
  side rule     the first child lies on the lower side (Morton: axis of the largest |cl - cr| of the children's box sums, partition
                type 2 - axis, cl <= cr; SAH: the largest box centre among the first child's triangles <= the smallest among the second
                child's on the node's axis, or — partition type 3 — children of count / 2 and count - count / 2 triangles)

mode = "enclose": boxes only have to enclose (the uploaded single leaf of a mesh of at most 4 triangles before a refit).
mode = "refit":   the side rule is not asserted (a refit keeps the topology); instead `before` = snapshot(...) taken before the refit must
                  hold the same set of (first triangle, count, partition type) and the same `refpos` over the mesh's range.

`tris` are the scene's triangles in DEVICE order (flat.tris[refpos]) with their current vertices; leaves index into them."""
import numpy as np

F = np.float32
LEAF, COUNT_MASK, PTYPE_SHIFT = 0x80000000, 0x1FFFFFFF, 29
MORTON, SAH = "morton", "sah"


def _collect(nodes, root, findings):
    """[(slot, first, count, ptype or -1, first child slot or -1)] bottom-up (children before parents), or None when the walk is broken"""
    seen, out, stack = set(), [], [(int(root), False)]
    span = {}
    while stack:
        slot, done = stack.pop()
        if done:
            begin = int(nodes[slot]["begin"])
            (f0, c0), (f1, c1) = span[begin], span[begin + 1]
            span[slot] = (min(f0, f1), c0 + c1)
            out.append((slot, span[slot][0], span[slot][1], (int(nodes[slot]["meta"]) >> PTYPE_SHIFT) & 3, begin))
            continue
        if not 0 <= slot < len(nodes):
            return findings.append(f"slot {slot} outside the node table")
        if slot in seen:
            return findings.append(f"slot {slot} is reached twice")
        seen.add(slot)
        meta, begin = int(nodes[slot]["meta"]), int(nodes[slot]["begin"])
        if meta & LEAF:
            span[slot] = (begin, meta & COUNT_MASK)
            out.append((slot, begin, meta & COUNT_MASK, -1, -1))
        else:
            stack += [(slot, True), (begin + 1, False), (begin, False)]
    return out


def node_set(nodes, root, tri_first=0):
    """{(first, count, leaf?, partition type or -1, first child's first, first child's count)} with positions relative to tri_first"""
    found = []
    rows = _collect(nodes, root, found)
    assert rows is not None, found
    span = {slot: (f - tri_first, c) for slot, f, c, _, _ in rows}
    return {(f - tri_first, c, p < 0, p) + (span[kid] if p >= 0 else (-1, -1)) for _, f, c, p, kid in rows}


def snapshot(nodes, root, refpos, tri_first, n_tris):
    """What a refit must keep: the set of (first triangle, count, partition type or -1 for a leaf) and the triangles' order."""
    found = []
    rows = _collect(nodes, root, found)
    assert rows is not None, found
    return {"topology": {(f, c, p) for _, f, c, p, _ in rows}, "refpos": np.array(refpos[tri_first:tri_first + n_tris])}


def audit(nodes, root, tris, kind, tri_first, n_tris, mode="built", leaf_max=None, before=None, refpos=None):
    assert kind in (MORTON, SAH) and mode in ("built", "refit", "enclose")
    leaf_max = leaf_max if leaf_max is not None else (4 if kind == MORTON else 8)
    findings = []
    rows = _collect(nodes, root, findings)
    if rows is None:
        return findings
    # tiling
    leaves = sorted((f, c) for _, f, c, p, _ in rows if p < 0)
    cursor = tri_first
    for f, c in leaves:
        if c == 0 or f != cursor:
            findings.append(f"leaves do not tile the range: leaf at {f} (+{c}) where {cursor} was due")
            return findings
        cursor += c
    if cursor != tri_first + n_tris:
        findings.append(f"leaves end at {cursor}, the mesh at {tri_first + n_tris}")
        return findings
    v = np.stack([tris["v1"], tris["v2"], tris["v3"]], 1)[tri_first:tri_first + n_tris].astype(F)
    tmn, tmx = v.min(1), v.max(1)
    cen = ((tmn + tmx) * F(0.5)).astype(F)
    box = {}
    for slot, f, c, ptype, kid in rows:
        a, b = f - tri_first, f - tri_first + c
        mn, mx = tmn[a:b].min(0), tmx[a:b].max(0)
        box[slot] = (mn, mx)
        have_mn, have_mx = nodes[slot]["bb_min"], nodes[slot]["bb_max"]
        if mode == "enclose":
            if not ((have_mn <= mn).all() and (have_mx >= mx).all()):
                findings.append(f"slot {slot}: box does not enclose its {c} triangles")
        elif not ((have_mn == mn).all() and (have_mx == mx).all()):
            findings.append(f"slot {slot}: box {have_mn.tolist()} {have_mx.tolist()} is not the exact box {mn.tolist()} {mx.tolist()} of its {c} triangles")
        if ptype < 0:
            if c > leaf_max:
                findings.append(f"slot {slot}: leaf of {c} triangles (at most {leaf_max})")
            continue
        if kind == MORTON and c <= 4:
            findings.append(f"slot {slot}: inner node over {c} triangles (a Morton subtree of 4 or fewer is one leaf)")
        if mode == "refit":
            continue
        if kind == MORTON:
            (lmn, lmx), (rmn, rmx) = box[kid], box[kid + 1]
            cl, cr = lmn + lmx, rmn + rmx
            axis = int(np.argmax(np.abs(cl - cr)))
            if ptype != 2 - axis:
                findings.append(f"slot {slot}: partition type {ptype}, the children differ most on axis {axis} (type {2 - axis})")
            elif not cl[axis] <= cr[axis]:
                findings.append(f"slot {slot}: the first child is on the upper side of axis {axis}")
    if mode != "refit" and kind == SAH:
        span = {slot: (f, c) for slot, f, c, _, _ in rows}
        for slot, f, c, ptype, kid in rows:
            if ptype < 0:
                continue
            (f0, c0), (f1, c1) = span[kid], span[kid + 1]
            if ptype == 3:
                if (c0, c1) != (c // 2, c - c // 2):
                    findings.append(f"slot {slot}: halved node of {c} with children of {c0} and {c1}")
                continue
            axis = 2 - ptype
            top = cen[f0 - tri_first:f0 - tri_first + c0, axis].max()
            bottom = cen[f1 - tri_first:f1 - tri_first + c1, axis].min()
            if not top <= bottom:
                findings.append(f"slot {slot}: first child reaches centre {top} on axis {axis}, the second starts at {bottom}")
    if mode == "refit":
        assert before is not None and refpos is not None
        if {(f, c, p) for _, f, c, p, _ in rows} != before["topology"]:
            findings.append("the refit changed the topology")
        if not np.array_equal(np.asarray(refpos[tri_first:tri_first + n_tris]), before["refpos"]):
            findings.append("the refit changed the triangle order")
    return findings
