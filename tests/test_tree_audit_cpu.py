"""The auditor of built trees (tests/tree_audit.py) is checked before a GPU sees it: it reports nothing on the trees of the CPU harness --
the device builders' steps run as loops (NORI_EMU_BUILDER=lbvh | ploc) and the host's SAH builder, both layouts, every case of
tests/tree_cases.py -- and it names every defect seeded into a copy of a clean tree's arrays."""
import time

import numpy as np
import pytest

from tests import tree_cases
from tests.tree_audit import audit, decode_bvh2, decode_pairs, decode_wide, triangle_pads

BUILDERS = ("lbvh", "ploc", "sah")
LAYOUTS = ("bvh2", "bvh4q")


def _audit_case(name, builder, layout):
    tris, mesh = tree_cases.geometry(name)
    tree, info = tree_cases.emu_tree(name, builder, layout)
    return tree, info, audit(tree, tris, mesh, info)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("group", ["tiny", "small", "cut", "table"])
def test_the_harness_trees_are_sound(group, builder, layout):
    for name in tree_cases.GROUPS[group]:
        tree, info, found = _audit_case(name, builder, layout)
        assert found == [], f"{name}, {builder}, {layout}: {found}"
        if builder != "sah":
            assert info["n_references"] >= len(tree_cases.geometry(name)[0])
        if name == "giant-dust-cut" and builder == "ploc":
            assert info["n_references"] > 2 * info["n_triangles"]        # the knobs reached the builder: every triangle is cut


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("builder", BUILDERS)
def test_the_largest_tree_is_sound_and_audited_in_seconds(builder, layout):
    name = tree_cases.GROUPS["large"][0]
    tris, mesh = tree_cases.geometry(name)
    tree, info = tree_cases.emu_tree(name, builder, layout)
    t0 = time.perf_counter()
    found = audit(tree, tris, mesh, info)
    dt = time.perf_counter() - t0
    print(f"[tree audit] {name} {builder} {layout}: {tree['n_nodes']} nodes, {tree['n_pairs']} pairs audited in {dt:.2f} s")
    assert found == []
    assert dt < 10.0, "the audit is vectorised level by level: a 200 000-triangle tree takes seconds"


# ------------------------------------------------------------------------------------------------ seeded defects

def _clean(name, builder, layout):
    tris, mesh = tree_cases.geometry(name)
    tree, info = tree_cases.emu_tree(name, builder, layout)
    assert audit(tree, tris, mesh, info) == []
    return tree, info, tris, mesh


def _copy(tree):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tree.items()}


def _codes(tree, info, tris, mesh):
    return audit(tree, tris, mesh, info).codes()


def _leaf_paths(tree):
    """per leaf: (first pair, pairs, list of (node, child) on the way from the root) -- a plain recursive walk, for placing defects"""
    wide = bool(tree["wide"])
    links = (decode_wide(tree["nodes"]) if wide else decode_bvh2(tree["nodes"]))[2]
    out, stack = [], [(int(tree["root"]), [])]
    while stack:
        i, path = stack.pop()
        for k in range(links.shape[1]):
            ln = int(links[i, k])
            if wide and ln == -1:
                continue
            if ln >= 0:
                stack.append((ln, path + [(i, k)]))
            else:
                out.append(((~ln) >> 3, ((~ln) & 7) + 1, path + [(i, k)]))
    return out


def _slot_gid(tree):
    return decode_pairs(tree["pairs"])[3]


H_COL = {(0, 0): 8, (0, 1): 9, (0, 2): 6, (1, 0): 10, (1, 1): 11, (1, 2): 7}      # BVH2 half extents: (child, axis) -> float of the record
C_COL = {(0, 0): 0, (0, 1): 1, (0, 2): 4, (1, 0): 2, (1, 1): 3, (1, 2): 5}


@pytest.fixture(scope="module")
def soup():
    return _clean("soup-1023", "ploc", "bvh2")


@pytest.fixture(scope="module")
def soup_wide():
    return _clean("soup-1023", "ploc", "bvh4q")


@pytest.fixture(scope="module")
def cut():
    return _clean("giant-dust-cut", "ploc", "bvh2")


def test_untouched_copies_stay_silent(soup, soup_wide, cut):
    for tree, info, tris, mesh in (soup, soup_wide, cut):
        assert audit(_copy(tree), tris, mesh, info) == []


def test_a_slot_with_its_neighbours_triangle_id_is_named(soup):
    tree, info, tris, mesh = soup
    t = _copy(tree)
    u = t["pairs"].view(np.uint32)
    gid = _slot_gid(tree)
    pair = next(p for p in range(tree["n_pairs"]) if gid[2 * p] != 0xFFFFFFFF and gid[2 * p + 1] != 0xFFFFFFFF and gid[2 * p] != gid[2 * p + 1])
    u[pair, 18] = u[pair, 19]                                  # slot a now names slot b's triangle: one lost, one doubled, one mismatch
    codes = _codes(t, info, tris, mesh)
    assert "presence" in codes and "slot.vertices" in codes
    found = audit(t, tris, mesh, info)
    assert any(f.startswith("presence: 1 ") for f in found) and any(f.startswith("slot.vertices: 1 ") for f in found)


def test_a_half_extent_shrunk_by_twice_the_pad_is_named(soup):
    tree, info, tris, mesh = soup
    pad, _ = triangle_pads(tris)
    gid = _slot_gid(tree)
    lo, hi, _, _ = decode_bvh2(tree["nodes"])
    V = tris.astype(np.float64)
    for first, cnt, path in _leaf_paths(tree):
        g = int(gid[2 * first])
        node, child = path[-1]
        # an axis on which this triangle's vertex is the extreme of the leaf's stored box, up to its pad
        for a in range(3):
            if hi[node, child, a] - V[g, :, a].max() <= 1.01 * pad[g] and np.isfinite(hi[node, child, a]):
                for shrink, want in ((2.0 * pad[g], "contain.vertices"), (0.5 * pad[g], "contain.pad")):
                    t = _copy(tree)
                    # lower the upper face: centre and half extent both by shrink / 2
                    t["nodes"][node, H_COL[(child, a)]] = np.float32(np.nextafter(np.float32(t["nodes"][node, H_COL[(child, a)]] - np.float32(shrink)), np.float32(-np.inf)))
                    codes = _codes(t, info, tris, mesh)
                    assert "contain.pad" in codes, (g, a, codes)
                    if want == "contain.vertices":
                        assert "contain.vertices" in codes, (g, a, codes)
                return
    raise AssertionError("no leaf whose box is tight around its first triangle")


def test_child_links_exchanged_across_subtrees_are_named(soup):
    tree, info, tris, mesh = soup
    t = _copy(tree)
    links = decode_bvh2(tree["nodes"])[2]
    root = int(tree["root"])
    a, b = int(links[root, 0]), int(links[root, 1])
    assert a >= 0 and b >= 0
    u = t["nodes"].view(np.uint32)
    u[a, 12], u[b, 12] = u[b, 12].copy(), u[a, 12].copy()    # the left children of the root's two children change places
    codes = _codes(t, info, tris, mesh)
    assert "shape.reach" not in codes and "shape.tiling" not in codes and "presence" not in codes
    assert "contain.vertices" in codes


def test_a_duplicated_link_is_named(soup):
    tree, info, tris, mesh = soup
    t = _copy(tree)
    links = decode_bvh2(tree["nodes"])[2]
    node = next(i for i in range(tree["n_nodes"]) if links[i, 0] >= 0 and links[i, 1] >= 0)
    u = t["nodes"].view(np.uint32)
    u[node, 13] = u[node, 12]
    found = audit(t, tris, mesh, info)
    assert "shape.reach" in found.codes() and "presence" in found.codes()


def test_a_leaf_count_raised_by_one_is_named(soup, soup_wide):
    for tree, info, tris, mesh in (soup, soup_wide):
        t = _copy(tree)
        first, cnt, path = next(lf for lf in _leaf_paths(tree) if lf[1] < 4 and lf[0] + lf[1] < tree["n_pairs"])
        node, child = path[-1]
        u = t["nodes"].view(np.uint32)
        u[node, 12 + child] = np.uint32((~((first << 3) | cnt)) & 0xFFFFFFFF)          # count - 1 -> count
        assert "shape.tiling" in _codes(t, info, tris, mesh)


def test_a_32b_plane_moved_inwards_is_named(soup):
    tree, info, tris, mesh = soup
    assert tree["records_32b"] == 1
    w = tree["nodes32"]
    node = next(i for i in range(tree["n_nodes"]) if 0 < (w[i, 0] & 0xffff) < 65535)
    t = _copy(tree)
    t["nodes32"][node, 0] += 1                                 # the left child's low x plane one grid step up
    assert _codes(t, info, tris, mesh) == ["rec32.planes"]
    t = _copy(tree)
    t["nodes32"][node, 6] ^= 8
    assert "rec32.links" in _codes(t, info, tris, mesh)


def test_a_wide_hi_byte_lowered_is_named(soup_wide):
    tree, info, tris, mesh = soup_wide
    assert tree["wide"] == 1
    lo, hi, links, allhit, used, qlo, qhi, axis = decode_wide(tree["nodes"])
    gid = _slot_gid(tree)
    V = tris.astype(np.float64)
    n_named = 0
    for first, cnt, path in _leaf_paths(tree):
        node, child = path[-1]
        g = [int(x) for x in gid[2 * first:2 * (first + cnt)] if x != 0xFFFFFFFF]
        for a in range(3):
            step = (hi[node, child, a] - lo[node, child, a]) / max(int(qhi[node, child, a] - qlo[node, child, a]), 1)
            if qhi[node, child, a] > qlo[node, child, a] and max(V[k, :, a].max() for k in g) > hi[node, child, a] - step:
                t = _copy(tree)
                u = t["nodes"].view(np.uint32)
                col = 7 + a                                    # hiX, hiY, hiZ = dwords 7, 8, 9
                u[node, col] -= np.uint32(1 << (8 * child))
                assert "contain.vertices" in _codes(t, info, tris, mesh), (node, child, a)
                n_named += 1
                break
        if n_named >= 5:
            break
    assert n_named >= 5


def test_a_gap_between_the_parts_of_a_cut_triangle_is_named(cut):
    tree, info, tris, mesh = cut
    gid = _slot_gid(tree)
    refs = np.bincount(gid[gid != 0xFFFFFFFF].astype(np.int64), minlength=len(tris))
    lo, hi, _, _ = decode_bvh2(tree["nodes"])
    giant = int(np.argmax(refs))
    assert refs[giant] > 1
    for first, cnt, path in _leaf_paths(tree):
        if giant in gid[2 * first:2 * (first + cnt)].tolist():
            node, child = path[-1]
            a = int(np.argmax(hi[node, child] - lo[node, child]))
            t = _copy(tree)
            t["nodes"][node, H_COL[(child, a)]] *= np.float32(0.5)      # this part's box to half its width around the same centre
            codes = _codes(t, info, tris, mesh)
            assert "cover" in codes, codes
            return
    raise AssertionError("the cut triangle is in no leaf")


def test_wide_slot_order_and_empty_slots_are_named(soup_wide):
    tree, info, tris, mesh = soup_wide
    lo, hi, links, allhit, used, qlo, qhi, axis = decode_wide(tree["nodes"])
    node = next(i for i in range(tree["n_nodes"]) if used[i].sum() == 4 and (qlo[i, 3, axis[i]] + qhi[i, 3, axis[i]]) - (qlo[i, 0, axis[i]] + qhi[i, 0, axis[i]]) > 4)
    t = _copy(tree)
    u = t["nodes"].view(np.uint32)

    def swap_bytes(word, a, b):
        x, y = (word >> (8 * a)) & 0xff, (word >> (8 * b)) & 0xff
        return (word & ~((0xff << (8 * a)) | (0xff << (8 * b)))) | (x << (8 * b)) | (y << (8 * a))
    for col in range(4, 10):
        u[node, col] = np.uint32(swap_bytes(int(u[node, col]), 0, 3))
    u[node, 12], u[node, 15] = u[node, 15].copy(), u[node, 12].copy()          # slots 0 and 3 exchanged whole: still a sound tree, wrong order
    assert _codes(t, info, tris, mesh) == ["shape.wide-order"]
    node = next(i for i in range(tree["n_nodes"]) if used[i].sum() < 4)
    t = _copy(tree)
    t["nodes"].view(np.uint32)[node, 7] |= np.uint32(1 << 24)                 # the unused slot 3: hi x = 1
    assert _codes(t, info, tris, mesh) == ["shape.wide-empty"]


def test_counts_of_accel_info_are_held(soup):
    tree, info, tris, mesh = soup
    for key in ("n_nodes", "max_depth", "n_references"):
        wrong = dict(info); wrong[key] += 1
        assert _codes(tree, wrong, tris, mesh) == ["count." + key]
