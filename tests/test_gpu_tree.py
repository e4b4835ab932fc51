"""The tree the HIP kernels of lbvh.hip built, read back from device memory (Renderer.tree() -> nori_hip_debug_tree) and audited node by node,
triangle by triangle (tests/tree_audit.py; the auditor itself is checked in tests/test_tree_audit_cpu.py), and held bit for bit against the
tree of the CPU harness that runs the same steps as loops (tests/emu/emu_builder.h).  Rays only sample a tree; this reads all of it."""
import time

import numpy as np
import pytest

from nori_amd._capi import NoriError
from nori_amd.render import Renderer
from tests import scenes, tree_cases
from tests.tree_audit import audit

pytestmark = pytest.mark.gpu

LBVH, AUTO, PLOC, HOST = 1, 2, 3, 0
DEVICE_BUILDS = [(b, lay) for b in (LBVH, PLOC, AUTO) for lay in ("bvh2", "bvh4q")]
TREE_KEYS = ("root", "n_nodes", "n_pairs", "wide", "records_32b", "nodes", "nodes32", "grid_mn", "grid_scale", "pairs")


def _bits(a):
    return None if a is None else (np.ascontiguousarray(a).view(np.uint32) if isinstance(a, np.ndarray) else a)


def differing(a, b):
    """the keys in which two tree dicts differ, compared as bit patterns"""
    out = []
    for k in TREE_KEYS:
        x, y = _bits(a[k]), _bits(b[k])
        same = (x is None and y is None) or (x is not None and y is not None and (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y))
        if not same:
            where = ""
            if isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.shape == y.shape and x.ndim == 2:
                rows = np.nonzero((x != y).any(1))[0]
                where = f" ({rows.size} records, first {rows[:4].tolist()})"
            out.append(k + where)
    return out


def _build(r, name, builder, layout):
    """(tree, accel_info) of case `name` built in context r"""
    _, env = tree_cases.case(name)
    with tree_cases.knobs(dict(env, **({"NORI_HIP_ACCEL_LAYOUT": layout} if layout else {}))):
        r.build_accel(builder)
    return r.tree(), r.accel_info()


def _audit_all(names):
    for name in names:
        sc, _ = tree_cases.case(name)
        tris, mesh = tree_cases.geometry(name)
        with Renderer(0) as r:
            r.upload(sc, build=False)
            for builder, layout in DEVICE_BUILDS + [(HOST, None)]:
                tree, info = _build(r, name, builder, layout)
                assert info["built_on_device"] == (0 if builder == HOST else 1), (name, builder, layout)
                if layout == "bvh4q" and len(tris) > 4:
                    assert tree["wide"] == 1 and info["node_children"] == 4, (name, builder)
                if layout == "bvh2":
                    assert tree["wide"] == 0
                found = audit(tree, tris, mesh, info)
                assert found == [], f"{name}, builder {builder}, {layout}: {found}"
                if name == "giant-dust-cut" and builder in (PLOC, AUTO):
                    assert info["n_references"] > 2 * info["n_triangles"]      # the knobs reached the builder: every triangle is cut


@pytest.mark.parametrize("group", ["tiny", "small", "cut", "table"])
def test_the_kernels_trees_are_sound(group):
    """5a: every case of tests/tree_cases.py through the radix tree, PLOC and the default builder, as BVH2 and as wide nodes, and once through
    the host's builder (the uploaded tree read back): the audit finds nothing."""
    _audit_all(tree_cases.GROUPS[group])


@pytest.mark.parametrize("builder,layout", DEVICE_BUILDS + [(HOST, None)])
def test_the_largest_tree_is_sound(builder, layout):
    name = tree_cases.GROUPS["large"][0]
    sc, _ = tree_cases.case(name)
    tris, mesh = tree_cases.geometry(name)
    with Renderer(0) as r:
        r.upload(sc, build=False)
        tree, info = _build(r, name, builder, layout)
    assert info["built_on_device"] == (0 if builder == HOST else 1)
    t0 = time.perf_counter()
    found = audit(tree, tris, mesh, info)
    print(f"[tree audit] {name} builder {builder} {layout}: {tree['n_nodes']} nodes, {tree['n_pairs']} pairs audited in {time.perf_counter() - t0:.2f} s")
    assert found == []


@pytest.mark.parametrize("layout", ["bvh2", "bvh4q"])
@pytest.mark.parametrize("builder,emu_builder", [(LBVH, "lbvh"), (PLOC, "ploc")])
@pytest.mark.parametrize("name", tree_cases.SAME_AS_HARNESS)
def test_the_kernels_tree_is_the_harnesss_tree(name, builder, emu_builder, layout):
    """5b: "same steps, same arithmetic, the same tree" (lbvh.hip): root, node records, 32-B records and their grid, pair records of the device's
    tree equal the harness's bit for bit -- no field is exempt, no tolerance on a float."""
    sc, _ = tree_cases.case(name)
    want, want_info = tree_cases.emu_tree(name, emu_builder, layout)
    with Renderer(0) as r:
        r.upload(sc, build=False)
        got, info = _build(r, name, builder, layout)
    assert info["built_on_device"] == 1
    for k in ("n_nodes", "n_leaves", "max_depth", "n_references", "node_children", "node_records_32b"):
        assert info[k] == want_info[k], (k, info[k], want_info[k])
    assert differing(got, want) == []


def test_the_wave_per_treelet_form_builds_the_serial_forms_tree():
    """5c: NORI_HIP_TREELET_SERIAL=0 and 1 (two sweeps): the same tree, record for record, on the 30 000-triangle soup of
    test_treelet_wave_builds_the_tree_of_the_serial_form, which compares five numbers of it."""
    sc = scenes.soup_scene(30000, seed=11, width=16, height=16)
    trees = []
    with Renderer(0) as r:
        r.upload(sc, build=False)
        for serial in ("0", "1"):
            with tree_cases.knobs({"NORI_HIP_TREELET_SERIAL": serial, "NORI_HIP_TREELET_SWEEPS": "2"}):
                r.build_accel(PLOC)
            assert r.accel_info()["built_on_device"] == 1
            trees.append(r.tree())
    assert trees[0]["n_nodes"] > 10000
    assert differing(trees[0], trees[1]) == []


def test_two_contexts_build_one_tree():
    """5d: two contexts, the default builder, the pa5 table (cut triangles, re-insertion conflicts settled by 64-bit maxima): bit-equal trees."""
    sc, _ = tree_cases.case("table")
    trees = []
    for _ in range(2):
        with Renderer(0) as r:
            r.upload(sc, builder=AUTO)
            info = r.accel_info()
            assert info["built_on_device"] == 1 and info["n_references"] > info["n_triangles"]
            trees.append(r.tree())
    assert differing(trees[0], trees[1]) == []


def test_no_tree_is_refused_and_the_context_stays_usable():
    """5e: nori_hip_debug_tree before build_accel is an invalid argument with a message; afterwards the context builds, reads back, audits."""
    name = "soup-257"
    sc, _ = tree_cases.case(name)
    tris, mesh = tree_cases.geometry(name)
    with Renderer(0) as r:
        with pytest.raises(NoriError, match="INVALID_ARGUMENT.*debug_tree"):
            r.tree()
        r.upload(sc, build=False)
        with pytest.raises(NoriError, match="INVALID_ARGUMENT.*debug_tree"):
            r.tree()
        r.build_accel(AUTO)
        assert audit(r.tree(), tris, mesh, r.accel_info()) == []
