"""Audit of a tree as the traversal kernels read it, record by record, in numpy and binary64 -- no GPU, no library.

    findings = audit(tree, tris, tri_mesh, info)

tree: the dict of Renderer.tree() / Emu.tree() (root, nodes [n, 16] float32, pairs [p, 24] float32, wide, nodes32 [n, 8] uint32 with grid_mn,
grid_scale, or None).  tris [T, 3, 3] float32: the scene's triangles by global index (extend_cases.scene_triangles), tri_mesh [T]: the mesh
of each (scene_meshes).  info: the builder's accel_info, or None.  The answer is a list of strings "<code>: <how many> ... <first places>", one
per kind of defect; empty means the tree is sound.

The layouts are decoded from their statements in rt_types.h, rt_nodeq.h and rt_wide.h, not through those headers:

    BVH2 node    q0 = (lc.x, lc.y, rc.x, rc.y), q1 = (lc.z, rc.z, lh.z, rh.z), q2 = (lh.x, lh.y, rh.x, rh.y), q3 = (link left, link right, 0, 0);
                 a child's box is [c - h, c + h]; h = kBoxHalfInf (2^59): unbounded on that axis
    wide node    q0 = (origin.xyz, meta), meta = ex | ey << 8 | ez << 16 | axis << 24 | kWideAllHit; q1 = (loX, loY, loZ, hiX), q2 = (hiY, hiZ, 0, 0),
                 child k's 8-bit coordinate in byte k; q3 = four links; child box = origin + {lo, hi} 2^(e - 128); kWideAllHit: no box is tested
    link         >= 0: node index; < 0: leaf, ~link = first_pair << 3 | n_pairs - 1
    pair record  24 floats, slot k in {0, 1}: p0 = f[0 + k, 2 + k, 4 + k], e1 = f[6 + k, 8 + k, 10 + k], e2 = f[12 + k, 14 + k, 16 + k],
                 global triangle = bits f[18 + k], mesh = bits f[20 + k], f[22], f[23] = 0
    32-B record  dwords 0 / 1 = x low / high planes (left child bits 0-15, right 16-31), 2 / 3 = y, 4 / 5 = z, 6 / 7 = the links; plane = mn + q scale

What is held:

  shape        every node is reached exactly once from the root, links are in range, a leaf has at most 4 pairs, the leaves' ranges tile the pair
               records from 0 (from 1 in wide trees, whose pair 0 is the reserved all-zero pair); wide slots: the used ones first, ascending
               along the node's axis, the unused ones with link kWideEmpty and lo = 255, hi = 0; the counts of accel_info
  pair slots   p0, e1 = float32(p1 - p0), e2 = float32(p2 - p0) and the mesh bit for bit those of the slot's triangle; a padding slot only as
               the last slot of a leaf, all zeros with id kNoTriangle
  presence     every triangle occupies a slot of some leaf
  containment  WITHOUT slack.  The path box of a leaf is the intersection of all child boxes on the way from the root (a ray reaches the leaf
               only through every one of them), evaluated in binary64.  "Parent contains child" is NOT an invariant of these trees and is not
               checked: every stored box is rounded outwards on its own and made directly from leaf boxes (segment tree / the builder's own
               boxes), so a child's stored box may stick out of its parent's by an ulp.  A triangle with one reference lies in its leaf's path
               box -- its vertices exactly, and grown by 0.99 x its pad (tri_box_pad restated in binary64 with kBoxPadRel x the scene diagonal;
               the 1 % covers the pad's own evaluation in binary32, ~1e-6 relative).  A numerically collinear triangle (sin^2 < 1e-8, decided
               in binary32 with the builders' own order of operations: the threshold is theirs) sits only under unbounded boxes.
  coverage     a triangle with several references: every point of the barycentric lattice of order 16 (vertices and edge points included)
               lies in the path box of one of its leaves, within 2^-40 x the scene diagonal (the rounding of the binary64 combination)
  32-B records the links are the 64-B record's; a plane lies at or outside the 64-B box's face, or -- where that face is outside the grid --
               on the grid's last plane

Deviations from the first statement of these invariants, with their reasons:
  * a wide node with kWideAllHit stores lo = 0, hi = 255 in ALL four slots (rt_wide.h, wide_pack: its planes are never read); its unused slots
    are recognised by their link alone.
  * wide slots ascend by the float32 sum mn + mx of the children's TRUE boxes; the stored planes are floor / ceil of those on the node's grid,
    so lo + hi of successive slots may step back by one grid unit (each of lo, hi is less than one unit from its true value: the sums differ
    by less than two), never by two -- plus the rounding of the two float32 sums themselves, an ulp of 2 |coordinate| between them.
"""
from __future__ import annotations

import numpy as np

K_NO_TRIANGLE = 0xFFFFFFFF
K_BOX_HALF_INF = float(2.0 ** 59)
K_WIDE_ALL_HIT = 1 << 26
K_WIDE_EMPTY = -1
K_BOX_PAD_REL = float(np.float32(2e-6))
LATTICE = 16
MAX_LEAF_PAIRS = 4


class Findings(list):
    def add(self, code, where, what=""):
        where = np.atleast_1d(np.asarray(where))
        if where.size:
            self.append(f"{code}: {where.size} {what}, first at {where[:6].tolist()}")

    def codes(self):
        return sorted({f.split(":")[0] for f in self})


def scene_meshes(sc):
    """[T] uint32: the mesh of every global triangle (the companion of extend_cases.scene_triangles)"""
    if not sc.meshes:
        return np.zeros(0, np.uint32)
    return np.concatenate([np.full(m.indices.shape[0], k, np.uint32) for k, m in enumerate(sc.meshes)])


# ------------------------------------------------------------------------------------------------ decoding

def _links(words):
    return words.view(np.uint32).astype(np.int64) - ((words.view(np.uint32).astype(np.int64) >> 31) << 32)


def decode_bvh2(nodes):
    """(lo, hi, links, unbounded): [n, 2, 3] float64 faces of the two child boxes (-inf / +inf on an unbounded axis), [n, 2] int64 links,
    [n, 2] bool: unbounded on every axis"""
    f = np.ascontiguousarray(nodes, np.float32)
    d = f.astype(np.float64)
    c = np.stack([np.stack([d[:, 0], d[:, 1], d[:, 4]], 1), np.stack([d[:, 2], d[:, 3], d[:, 5]], 1)], 1)
    h = np.stack([np.stack([d[:, 8], d[:, 9], d[:, 6]], 1), np.stack([d[:, 10], d[:, 11], d[:, 7]], 1)], 1)
    inf = h == K_BOX_HALF_INF
    lo, hi = np.where(inf, -np.inf, c - h), np.where(inf, np.inf, c + h)
    return lo, hi, _links(np.ascontiguousarray(f[:, 12:14])), inf.all(axis=2)


def decode_wide(nodes):
    """(lo, hi, links, unbounded, used, qlo, qhi, axis): [n, 4, 3] float64 faces, [n, 4] links, [n, 4] bool (the node is kWideAllHit),
    [n, 4] bool (the slot's link is not kWideEmpty), the stored bytes [n, 4, 3], the node's axis [n]"""
    f = np.ascontiguousarray(nodes, np.float32)
    u = f.view(np.uint32)
    origin = f[:, 0:3].astype(np.float64)
    meta = u[:, 3].astype(np.int64)
    e = np.stack([meta & 0xff, (meta >> 8) & 0xff, (meta >> 16) & 0xff], 1)
    axis = (meta >> 24) & 3
    allhit = (meta & K_WIDE_ALL_HIT) != 0
    scale = np.ldexp(1.0, (e - 128).astype(np.int32))                                     # [n, 3]
    lo_w = np.stack([u[:, 4], u[:, 5], u[:, 6]], 1).astype(np.int64)                      # [n, axis]
    hi_w = np.stack([u[:, 7], u[:, 8], u[:, 9]], 1).astype(np.int64)
    shifts = np.arange(4)[None, :, None] * 8
    qlo = (lo_w[:, None, :] >> shifts) & 0xff                                             # [n, slot, axis]
    qhi = (hi_w[:, None, :] >> shifts) & 0xff
    lo = origin[:, None, :] + qlo * scale[:, None, :]
    hi = origin[:, None, :] + qhi * scale[:, None, :]
    lo = np.where(allhit[:, None, None], -np.inf, lo)
    hi = np.where(allhit[:, None, None], np.inf, hi)
    links = _links(np.ascontiguousarray(f[:, 12:16]))
    return lo, hi, links, np.repeat(allhit[:, None], 4, 1), links != K_WIDE_EMPTY, qlo, qhi, axis


def decode_nodes32(nodes32, grid_mn, grid_scale):
    """(p_lo, p_hi, q_lo, q_hi, links): planes [n, 2, 3] float64 = mn + q scale, their grid coordinates, the links [n, 2] int64"""
    w = np.ascontiguousarray(nodes32, np.uint32)
    mn, sc = np.asarray(grid_mn, np.float64), np.asarray(grid_scale, np.float64)
    q_lo = np.stack([np.stack([w[:, 2 * a] & 0xffff, w[:, 2 * a] >> 16], 1) for a in range(3)], 2).astype(np.float64)
    q_hi = np.stack([np.stack([w[:, 2 * a + 1] & 0xffff, w[:, 2 * a + 1] >> 16], 1) for a in range(3)], 2).astype(np.float64)
    return mn + q_lo * sc, mn + q_hi * sc, q_lo, q_hi, _links(np.ascontiguousarray(w[:, 6:8]))


def decode_pairs(pairs):
    """per slot (2 per pair record, slot s = 2 pair + k): p0, e1, e2 [2 p, 3] float32, gid, mesh [2 p] uint32; and per pair the two spare words"""
    f = np.ascontiguousarray(pairs, np.float32).reshape(-1, 24)
    u = f.view(np.uint32)

    def slots(cols):
        return np.stack([f[:, cols], f[:, [c + 1 for c in cols]]], 1).reshape(-1, 3)
    p0, e1, e2 = slots([0, 2, 4]), slots([6, 8, 10]), slots([12, 14, 16])
    return p0, e1, e2, u[:, 18:20].reshape(-1), u[:, 20:22].reshape(-1), u[:, 22:24]


# ------------------------------------------------------------------------------------------------ the scene's side

def scene_diagonal(tris):
    t = np.asarray(tris, np.float64).reshape(-1, 3)
    return float(np.linalg.norm(t.max(axis=0) - t.min(axis=0))) if len(t) else 0.0


def _sin2_f32(tris):
    """sin^2 of the angle between the edges as tri_box_pad computes it (binary32, dot = x + (y + z), no contraction); and which triangles
    have an edge of length 0 (they keep the plain pad and are bounded)"""
    t = np.asarray(tris, np.float32)
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]

    def dot(a, b):
        return a[:, 0] * b[:, 0] + (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])
    l1, l2 = dot(e1, e1), dot(e2, e2)
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    with np.errstate(all="ignore"):
        s2 = dot(c, c) / (l1 * l2)
    zero_edge = ~(l1 > 0) | ~(l2 > 0)
    return s2, zero_edge


def triangle_pads(tris):
    """(pad [T] float64, collinear [T] bool): tri_box_pad with pad0 = kBoxPadRel x the scene diagonal, the pad in binary64"""
    s2_32, zero_edge = _sin2_f32(tris)
    collinear = ~zero_edge & ~(s2_32 >= np.float32(1e-8))
    t = np.asarray(tris, np.float64)
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    c = np.cross(e1, e2)
    with np.errstate(all="ignore"):
        s2 = (c * c).sum(1) / ((e1 * e1).sum(1) * (e2 * e2).sum(1))
    pad0 = K_BOX_PAD_REL * scene_diagonal(tris) + 1e-30
    with np.errstate(all="ignore"):
        pad = np.where(zero_edge | (s2 >= 1.0), pad0, pad0 / np.sqrt(s2))
    return np.where(collinear, pad0, pad), collinear


def lattice_weights(order=LATTICE):
    ij = [(i, j) for i in range(order + 1) for j in range(order + 1 - i)]
    w = np.array([[order - i - j, i, j] for i, j in ij], np.float64) / order
    return w                                                                               # [153, 3]


# ------------------------------------------------------------------------------------------------ the walk

def walk(tree, out):
    """Level by level from the root.  Returns (reach [n] visits per node, leaves: dict of first, count, lo, hi [L, 3], unbounded [L], depth [L],
    levels).  depth of a leaf = nodes on the way to it."""
    n = int(tree["n_nodes"])
    n_pairs = int(tree["n_pairs"])
    wide = bool(tree["wide"])
    root = int(tree["root"])
    reach = np.zeros(n, np.int64)
    L = {"first": [], "count": [], "lo": [], "hi": [], "unb": [], "depth": []}

    def add_leaves(links, lo, hi, unb, depth):
        code = -links - 1
        L["first"].append(code >> 3); L["count"].append((code & 7) + 1)
        L["lo"].append(lo); L["hi"].append(hi); L["unb"].append(unb); L["depth"].append(np.full(len(links), depth, np.int64))

    levels = 0
    if root < 0:
        add_leaves(np.array([root], np.int64), np.full((1, 3), -np.inf), np.full((1, 3), np.inf), np.array([True]), 0)
    elif root >= n:
        out.add("shape.link", [root], "root link out of range")
    else:
        if wide:
            clo, chi, links, cunb, used, qlo, qhi, axis = decode_wide(tree["nodes"])
        else:
            clo, chi, links, cunb = decode_bvh2(tree["nodes"])
            used = np.ones_like(links, bool)
        idx = np.array([root], np.int64)
        lo, hi, unb = np.full((1, 3), -np.inf), np.full((1, 3), np.inf), np.array([True])
        visited = 0
        while idx.size:
            levels += 1
            visited += idx.size
            if visited > 4 * n + 64 or levels > 4096:
                out.add("shape.reach", [int(idx[0])], "the walk does not end (a link leads back up)")
                break
            reach += np.bincount(idx, minlength=n)
            k = links.shape[1]
            plo = np.maximum(lo[:, None, :], clo[idx]).reshape(-1, 3)
            phi = np.minimum(hi[:, None, :], chi[idx]).reshape(-1, 3)
            punb = (unb[:, None] & cunb[idx]).reshape(-1)
            ln = links[idx].reshape(-1)
            us = used[idx].reshape(-1)
            parent = np.repeat(idx, k)
            inner = us & (ln >= 0)
            bad = inner & (ln >= n)
            out.add("shape.link", parent[bad], "child links beyond the node records")
            leaf = us & (ln < 0)
            if leaf.any():
                add_leaves(ln[leaf], plo[leaf], phi[leaf], punb[leaf], levels)
            go = inner & ~bad
            idx, lo, hi, unb = ln[go], plo[go], phi[go], punb[go]
    leaves = {k: (np.concatenate(v) if v else np.zeros((0, 3) if k in ("lo", "hi") else 0, np.float64 if k in ("lo", "hi") else (bool if k == "unb" else np.int64)))
              for k, v in L.items()}
    out.add("shape.reach", np.nonzero(reach != 1)[0], "nodes not reached exactly once from the root")
    out.add("shape.leaf-size", np.nonzero(leaves["count"] > MAX_LEAF_PAIRS)[0], f"leaves of more than {MAX_LEAF_PAIRS} pairs")
    beyond = leaves["first"] + leaves["count"] > n_pairs
    out.add("shape.link", leaves["first"][beyond], "leaf ranges beyond the pair records")
    return reach, leaves, levels


def _check_wide_slots(tree, out):
    clo, chi, links, cunb, used, qlo, qhi, axis = decode_wide(tree["nodes"])
    n = links.shape[0]
    allhit = cunb[:, 0]
    n_used = used.sum(1)
    out.add("shape.wide-empty", np.nonzero((used != (np.arange(4)[None, :] < n_used[:, None])).any(1))[0], "wide nodes with an unused slot in front of a used one")
    empty_ok = (qlo == 255).all(2) & (qhi == 0).all(2)
    allhit_ok = (qlo == 0).all(2) & (qhi == 255).all(2)
    out.add("shape.wide-empty", np.nonzero((~used & ~empty_ok & ~allhit[:, None]).any(1))[0], "unused wide slots without lo = 255, hi = 0")
    out.add("shape.wide-empty", np.nonzero((allhit[:, None] & ~allhit_ok).any(1))[0], "kWideAllHit nodes whose planes are not lo = 0, hi = 255")
    out.add("shape.wide-empty", np.nonzero((used & ~allhit[:, None] & (qlo > qhi).any(2)).any(1))[0], "used wide slots with lo > hi")
    key = np.take_along_axis(qlo + qhi, axis[:, None, None].clip(0, 2), axis=2)[:, :, 0]   # [n, 4] along the node's axis
    both = used[:, 1:] & used[:, :-1] & ~allhit[:, None]
    # the order is that of float32(mn + mx): each sum is rounded by half an ulp at most -- in grid units of the node, next to nothing in a scene
    # around the origin, several units in one that stands 1e6 away
    f = np.ascontiguousarray(tree["nodes"], np.float32)
    e = (f.view(np.uint32)[:, 3].astype(np.int64)[:, None] >> (8 * np.arange(3))[None, :]) & 0xff
    scale = np.take_along_axis(np.ldexp(1.0, (e - 128).astype(np.int32)), axis[:, None].clip(0, 2), axis=1)[:, 0]
    org = np.take_along_axis(f[:, 0:3].astype(np.float64), axis[:, None].clip(0, 2), axis=1)[:, 0]
    with np.errstate(all="ignore"):
        ulps = np.spacing((2.0 * np.abs(org) + 510.0 * scale).astype(np.float32)).astype(np.float64) / scale
    ulps = np.where(np.isfinite(ulps), ulps, 0.0)
    out.add("shape.wide-order", np.nonzero((both & (key[:, 1:] <= key[:, :-1] - 2 - ulps[:, None])).any(1))[0], "wide nodes whose slots do not ascend along the axis")
    out.add("shape.wide-order", np.nonzero(axis > 2)[0], "wide nodes with axis 3")
    del n


def audit(tree, tris, tri_mesh, info=None):
    out = Findings()
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    tri_mesh = np.asarray(tri_mesh, np.uint32)
    T = tris.shape[0]
    n, n_pairs, wide = int(tree["n_nodes"]), int(tree["n_pairs"]), bool(tree["wide"])
    if T == 0:
        return out
    if tree["nodes"].shape[0] != n or tree["pairs"].shape[0] != n_pairs:
        out.add("shape.count", [n, n_pairs], "records returned differ from the counts")
        return out
    reach, leaves, levels = walk(tree, out)
    if wide and n:
        _check_wide_slots(tree, out)

    # ---- the leaves' ranges tile the pair records
    base = 1 if wide else 0
    order = np.argsort(leaves["first"], kind="stable")
    first, count = leaves["first"][order], leaves["count"][order]
    if len(first) == 0:
        out.add("shape.tiling", [0], "no leaf")
    else:
        if first[0] != base:
            out.add("shape.tiling", [int(first[0])], f"the first leaf does not start at pair {base}")
        out.add("shape.tiling", first[1:][first[1:] != (first + count)[:-1]], "leaf ranges overlap or leave a gap")
        if first[-1] + count[-1] != n_pairs:
            out.add("shape.tiling", [int(first[-1] + count[-1])], f"the leaves end short of or beyond the {n_pairs} pair records")

    # ---- pair slots
    p0, e1, e2, gid, mesh, spare = decode_pairs(tree["pairs"])
    out.add("slot.spare", np.nonzero(spare.any(1))[0], "pair records with a nonzero spare word")
    if wide and n_pairs:
        if tree["pairs"][0].view(np.uint32).any():
            out.add("slot.padding", [0], "the reserved pair 0 of a wide tree is not all zeros")
    is_pad = gid == K_NO_TRIANGLE
    if wide:
        is_pad[:2] = False                                    # (pair 0 was judged above)
    live = ~is_pad
    if wide:
        live[:2] = False
    out.add("slot.id", np.nonzero(live & (gid >= T))[0], "slots with a triangle id beyond the scene")
    live &= gid < T
    g = gid[live].astype(np.int64)
    want_p0 = tris[g, 0]
    want_e1, want_e2 = tris[g, 1] - tris[g, 0], tris[g, 2] - tris[g, 0]                   # binary32 subtraction
    same = ((p0[live].view(np.uint32) == want_p0.view(np.uint32)) & (e1[live].view(np.uint32) == want_e1.view(np.uint32))
            & (e2[live].view(np.uint32) == want_e2.view(np.uint32))).all(1)
    out.add("slot.vertices", np.nonzero(live)[0][~same], "slots whose p0 / e1 / e2 are not their triangle's")
    out.add("slot.mesh", np.nonzero(live)[0][mesh[live] != tri_mesh[g]], "slots whose mesh word is not their triangle's")
    pad_zero = ~(p0.view(np.uint32).any(1) | e1.view(np.uint32).any(1) | e2.view(np.uint32).any(1)) & (mesh == K_NO_TRIANGLE)
    out.add("slot.padding", np.nonzero(is_pad & ~pad_zero)[0], "padding slots that are not all zeros with id and mesh kNoTriangle")

    # ---- references: (slot, leaf) through the leaves that lie inside the pair records
    ok = (leaves["first"] >= 0) & (leaves["first"] + leaves["count"] <= n_pairs)
    lf = np.nonzero(ok)[0]
    per = 2 * leaves["count"][lf]
    ref_leaf = np.repeat(lf, per)
    start = np.cumsum(per) - per
    within = np.arange(per.sum()) - np.repeat(start, per)
    ref_slot = np.repeat(2 * leaves["first"][lf], per) + within
    last = within == np.repeat(per, per) - 1
    pads_here = is_pad[ref_slot]
    out.add("slot.padding", ref_slot[pads_here & ~last], "padding slots that are not the last slot of their leaf")
    keep = live[ref_slot]
    ref_leaf, ref_slot = ref_leaf[keep], ref_slot[keep]
    ref_tri = gid[ref_slot].astype(np.int64)
    n_refs = np.bincount(ref_tri, minlength=T)

    # ---- presence
    out.add("presence", np.nonzero(n_refs == 0)[0], "triangles in no leaf")

    # ---- counts
    if info is not None:
        if int(info["n_nodes"]) != n or int((reach > 0).sum()) != n:
            out.add("count.n_nodes", [int(info["n_nodes"]), n, int((reach > 0).sum())], "accel_info / records / reached")
        depth = 0 if n == 0 else (3 * levels if wide else int(leaves["depth"].max(initial=0)))
        if int(info["max_depth"]) != depth:
            out.add("count.max_depth", [int(info["max_depth"]), depth], "accel_info / recomputed")
        if int(info["n_leaves"]) != len(leaves["first"]):
            out.add("count.n_leaves", [int(info["n_leaves"]), len(leaves["first"])], "accel_info / recomputed")
        if int(info["n_references"]) and int(info["n_references"]) != int((~is_pad[2 if wide else 0:]).sum()):
            out.add("count.n_references", [int(info["n_references"]), int((~is_pad[2 if wide else 0:]).sum())], "accel_info / slots that are not padding")
        if int(info["node_children"]) != (4 if wide else 2):
            out.add("count.node_children", [int(info["node_children"])], "accel_info against the tree's layout")

    # ---- containment
    pad, collinear = triangle_pads(tris)
    diag = scene_diagonal(tris)
    V = tris.astype(np.float64)
    single = n_refs[ref_tri] == 1
    st, sl = ref_tri[single], ref_leaf[single]
    lo, hi = leaves["lo"][sl], leaves["hi"][sl]
    vmin, vmax = V[st].min(axis=1), V[st].max(axis=1)
    out.add("contain.vertices", st[((vmin < lo) | (vmax > hi)).any(1)], "triangles with a vertex outside their leaf's path box")
    grown = 0.99 * pad[st][:, None]
    bounded = ~collinear[st]
    out.add("contain.pad", st[bounded & ((vmin - grown < lo) | (vmax + grown > hi)).any(1)], "triangles whose box grown by 0.99 pad leaves the path box")
    out.add("contain.collinear", ref_tri[collinear[ref_tri] & ~leaves["unb"][ref_leaf]], "numerically collinear triangles under a bounded box")

    # ---- coverage of cut triangles
    multi = ~single
    if multi.any():
        mt, ml = ref_tri[multi], ref_leaf[multi]
        o = np.argsort(mt, kind="stable")
        mt, ml = mt[o], ml[o]
        W = lattice_weights()
        slack = 2.0 ** -40 * diag
        starts = np.nonzero(np.r_[True, mt[1:] != mt[:-1]])[0]
        uncovered = []
        chunk = 4096                                         # triangles per step
        for a in range(0, len(starts), chunk):
            s0 = starts[a]
            s1 = starts[a + chunk] if a + chunk < len(starts) else len(mt)
            t_, l_ = mt[s0:s1], ml[s0:s1]
            pts = np.einsum("pk,rkc->rpc", W, V[t_])                                          # [refs, 153, 3]
            inside = ((pts >= (leaves["lo"][l_] - slack)[:, None, :]) & (pts <= (leaves["hi"][l_] + slack)[:, None, :])).all(2)
            cov = np.logical_or.reduceat(inside, starts[a:a + chunk] - s0, axis=0)
            uncovered.append(mt[starts[a:a + chunk]][~cov.all(1)])
        out.add("cover", np.concatenate(uncovered), "cut triangles with lattice points in none of their leaves' path boxes")

    # ---- 32-B records
    if tree.get("nodes32") is not None and not wide and n:
        blo, bhi, links64, _ = decode_bvh2(tree["nodes"])
        p_lo, p_hi, q_lo, q_hi, links32 = decode_nodes32(tree["nodes32"], tree["grid_mn"], tree["grid_scale"])
        out.add("rec32.links", np.nonzero((links32 != links64).any(1))[0], "32-B records whose links differ from the 64-B record's")
        bad_lo = np.where(q_lo > 0, p_lo > blo, False) | (q_lo > q_hi)
        bad_hi = np.where(q_hi < 65535, p_hi < bhi, False)
        out.add("rec32.planes", np.nonzero((bad_lo | bad_hi).any(axis=(1, 2)))[0], "32-B records with a plane inside the 64-B box")
    return out
