"""wf_extend ray by ray against the linear scan (Renderer.extend -> nori_hip_debug_extend; cases and expectations: tests/extend_cases.py).

The traversal kernel of the wavefront engine -- the hand-written gfx950 node loop over the 32-B node records, the LDS stack with its
global spill column and the `full` fallback, the LDS image of hot nodes, the select-form leaf step, the refill logic (static and
dynamic chunks, shadow ray then continuation ray of one path on one lane, hit records written late), the wide-node step -- is given
rays made for the places where a tree walk is at its limit, as stored path slots of all four kinds interleaved, through the launch a
render of the same scene makes.  EVERY hit record is compared with the oracle's as uint32 words: there is no tolerance.  The only
exemption is fuzz_intersect.ill_posed, it is counted, and the count must be 0 (as in test_fuzz_intersect_short)."""
import numpy as np
import pytest

from nori_amd import NoriError
from nori_amd import _capi as capi
from tests import extend_cases as xc
from tests.test_gpu_wavefront import _with_env

pytestmark = pytest.mark.gpu

NO_ASM = {"NORI_HIP_WF_NO_ASM_LOOP": 1}


def trace(sc, slots, builder=0, layout="bvh2", env=None, count=False, options=None):
    """(accel_info, records [n, 4] uint32, counts) of one Renderer.extend on a fresh context; env is set for the build of the tree
    (the LDS image's knobs are read there) and for the launch (the scheduling knobs)"""
    from nori_amd.render import Renderer

    def run():
        r = Renderer(0)
        try:
            r.set_option("accel_layout", layout)
            for k, v in (options or {}).items():
                r.set_option(k, v)
            r.upload(sc, builder=builder)
            res, counts = r.extend(slots["o"], slots["dir_a"], slots["dir_b"], slots["maxt_b"], slots["flags"], count_traversal=count)
            return r.accel_info(), xc.records_of(res), counts
        finally:
            r.close()
    return _with_env(env or {}, run)


def check(what, sc, slots, got, want, counts):
    bad, tolerated = xc.exempted(sc, slots, got, want)
    print(f"[extend] {what}: {len(want)} records, {len(bad)} differ, {tolerated} exempted as ill-posed; counts {counts}")
    assert not bad, (what, bad[:5], [(slots["cls"][r], slots["slot"][r]) for r in bad[:5]], got[bad[:5]], want[bad[:5]])
    assert tolerated == 0, f"{what}: {tolerated} rays needed the ill-posed exemption"
    for k, v in xc.expected_counts(slots).items():
        assert counts[k] == v, (what, k, counts[k], v)


@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e3])
@pytest.mark.parametrize("kind", xc.KINDS)
def test_asm_loop_shallow_trees(kind, scale):
    """Host-built trees (builder 0) of every scene kind at every size: the hand-written node loop with its stack in LDS wherever the
    tree has 32-B records and is no deeper than 16 entries -- every kind but `degenerate`, whose zero-area triangles sit in unbounded
    boxes, has such sizes -- and whatever else the render would run for the other sizes (a root that is a leaf; the 64-B nodes; the
    spilling stack for the host's deepest trees)."""
    qualified = []
    for n in xc.SIZES:
        sc, slots, want = xc.case("kind", kind, n, scale)
        info, got, counts = trace(sc, slots, builder=0)
        assert info["node_children"] == 2 and info["built_on_device"] == 0
        check(f"asm shallow {kind} x{n} scale {scale} (32-B records {info['node_records_32b']}, depth {info['max_depth']})", sc, slots, got, want, counts)
        if info["node_records_32b"] == 1 and info["max_depth"] + 1 <= 16:
            qualified.append(n)
    assert (qualified == []) if kind == "degenerate" else (len(qualified) >= 3), qualified


DEEP_ENVS = {"image": {}, "no image": {"NORI_HIP_NO_TOP_IMAGE": 1}, "3 cached nodes": {"NORI_HIP_TOP_NODES": 3}}


@pytest.mark.parametrize("image", list(DEEP_ENVS))
@pytest.mark.parametrize("builder", [1, 3])
def test_asm_loop_deep_trees(builder, image):
    """The device builders' trees of the 30000-triangle soup are deeper than the LDS stack: LdsStackHybrid, the spill column and the
    `full` fallback to trav_inner_step_q -- with the LDS image, without it, and with three cached nodes."""
    sc, slots, want = xc.case("deep")
    info, got, counts = trace(sc, slots, builder=builder, env=DEEP_ENVS[image])
    assert info["node_records_32b"] == 1 and info["node_children"] == 2 and info["max_depth"] + 1 > 16 and info["built_on_device"] == 1
    check(f"asm deep builder {builder}, {image} (depth {info['max_depth']})", sc, slots, got, want, counts)


@pytest.mark.parametrize("name,builder", [("deep", 1), ("deep", 3), ("soup", 0), ("sheets", 0), ("degenerate", 0)])
def test_compiler_loop_on_64_byte_nodes(name, builder):
    """The same trees under NORI_HIP_WF_NO_ASM_LOOP=1 (trav_inner_step on the 64-B nodes, LdsStackW with and without the spill), and a
    `degenerate` scene, whose tree has no 32-B records, so that the render takes this loop by itself.  (`sheets`: the case that found
    trav_inner_step holding a box's near side to an unwidened limit -- 48 records of far-origin rays named another of several
    coplanar triangles than the scan; rt_trace.h.)"""
    sc, slots, want = xc.case("deep") if name == "deep" else xc.case("kind", name, 3000, 1.0)
    info, got, counts = trace(sc, slots, builder=builder, env={} if name == "degenerate" else NO_ASM)
    assert info["node_children"] == 2 and info["node_records_32b"] == (0 if name == "degenerate" else 1)
    if name == "deep":
        assert info["max_depth"] + 1 > 16
    check(f"compiler loop {name} builder {builder} (depth {info['max_depth']})", sc, slots, got, want, counts)


@pytest.mark.parametrize("name,builder", [("soup", 0), ("deep", 1)])
def test_counting_kernels(name, builder):
    """count_traversal: the kernels a counting render runs write the same records; on a tree with 32-B records they walk those
    (trav_inner_step_q, the C++ statement of the hand-written loop), and count other node / triangle tests than the 64-B form --
    two different conservative supersets of the boxes (test_traversal_counters_are_those_of_the_timed_tree_form)."""
    sc, slots, want = xc.case("deep") if name == "deep" else xc.case("kind", name, 3000, 1.0)
    info, got, cq = trace(sc, slots, builder=builder, count=True)
    assert info["node_records_32b"] == 1
    check(f"counting, 32-B records, {name}", sc, slots, got, want, cq)
    _, got64, c64 = trace(sc, slots, builder=builder, count=True, env=NO_ASM)
    check(f"counting, 64-B nodes, {name}", sc, slots, got64, want, c64)
    _, _, plain = trace(sc, slots, builder=builder)
    assert plain["n_node_tests"] == 0 and plain["n_tri_tests"] == 0
    for c in (cq, c64):
        assert c["n_node_tests"] > 0 and c["n_tri_tests"] > 0
    assert (cq["n_node_tests"], cq["n_tri_tests"]) != (c64["n_node_tests"], c64["n_tri_tests"])


@pytest.mark.parametrize("name,n,scale,builder", [("soup", 3000, 37.5, 0), ("sheets", 500, 1.0, 0), ("stacked", 3000, 1e-3, 0), ("mixed", 33, 1e3, 0),
                                                  ("dups", 500, 37.5, 2), ("mixed", 3000, 1.0, 2), ("deep", 0, 1.0, 2), ("deep", 0, 1.0, 0)])
def test_wide_nodes(name, n, scale, builder):
    """accel_layout = bvh4q: trav_wide_step on BVH4 nodes with quantised child boxes, host- and device-built, plain and counting."""
    sc, slots, want = xc.case("deep") if name == "deep" else xc.case("kind", name, n, scale)
    info, got, counts = trace(sc, slots, builder=builder, layout="bvh4q")
    assert info["node_children"] == 4 and info["built_on_device"] == (1 if builder == 2 else 0)
    check(f"wide {name} x{n} scale {scale} builder {builder}", sc, slots, got, want, counts)
    _, got, counts = trace(sc, slots, builder=builder, layout="bvh4q", count=True)
    check(f"wide, counting, {name} x{n} scale {scale} builder {builder}", sc, slots, got, want, counts)
    assert counts["n_node_tests"] > 0 and counts["n_tri_tests"] > 0


def test_scheduling_changes_no_byte():
    """One soup of 500 triangles.  Fewer paths than a wave, one more and one fewer than a wave, a thousand: all-static chunks, most
    waves without a path.  NORI_HIP_WF_STATIC=0: the chunk size of the dynamic schedule -- and, with more paths than the persistent
    grid's static chunks cover, waves that claim dynamic chunks.  Refill, leaf and repeat thresholds at both ends of their ranges.
    All of these write the bytes of the default, which are the oracle's."""
    import torch
    sc, slots, want = xc.case("kind", "soup", 500, 1.0)
    _, default, counts = trace(sc, slots)
    check("scheduling, default", sc, slots, default, want, counts)
    for n in (1, 63, 64, 65, 1000):
        s = xc.take(slots, n)
        _, got, counts = trace(sc, s)
        check(f"scheduling, {n} paths", sc, s, got, want[:n], counts)
    s = xc.take(slots, 20000)
    w = want[np.arange(20000) % len(want)]
    _, got, counts = trace(sc, s, env={"NORI_HIP_WF_STATIC": 0})
    check("scheduling, 20000 paths, no static limit", sc, s, got, w, counts)
    # one workgroup of 16 waves per CU, 64 paths per wave handed out statically: the rest is claimed with the atomic
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 16 * 64 + 60000
    s = xc.take(slots, n)
    w = want[np.arange(n) % len(want)]
    _, got, counts = trace(sc, s, env={"NORI_HIP_WF_STATIC": 0, "NORI_HIP_WF_EXTEND_WGS_PER_CU": 1})
    assert np.array_equal(got, w)
    assert {k: counts[k] for k in ("n_closest_rays", "n_shadow_rays")} == xc.expected_counts(s)
    for env in ({"NORI_HIP_WF_REFILL": 1}, {"NORI_HIP_WF_REFILL": 64}, {"NORI_HIP_WF_LEAF": 1}, {"NORI_HIP_WF_LEAF": 64},
                {"NORI_HIP_WF_INNER_REPEAT": 1}, {"NORI_HIP_WF_INNER_REPEAT": 65}):
        _, got, counts = trace(sc, slots, env=env)
        assert np.array_equal(got, default), env
        check(f"scheduling, {env}", sc, slots, got, want, counts)


def test_empty_slots_and_the_empty_scene():
    sc, slots, want = xc.case("kind", "soup", 500, 1.0)
    nothing = dict(slots, flags=np.zeros_like(slots["flags"]))
    _, got, counts = trace(sc, nothing)
    assert (got == capi.EXTEND_SENTINEL).all()                            # every sentinel in place
    assert counts == {"n_closest_rays": 0, "n_shadow_rays": 0, "n_node_tests": 0, "n_tri_tests": 0}
    # the empty scene: miss / unoccluded for every kind of slot, both rays of a slot counted
    sc, slots, want = xc.case("empty")
    used = slots["flags"] != 0
    assert (want[used] == xc.MISS).all() and (want[~used] == capi.EXTEND_SENTINEL).all()
    for layout in ("bvh2", "bvh4q"):
        info, got, counts = trace(sc, slots, layout=layout)
        assert info["n_triangles"] == 0
        check(f"empty scene, {layout}", sc, slots, got, want, counts)
    # no slot at all: nothing is launched
    _, got, counts = trace(sc, xc.take(slots, 0))
    assert got.shape == (0, 4) and counts["n_closest_rays"] == 0 and counts["n_shadow_rays"] == 0


def test_refusals_leave_the_context_usable():
    """NORI_ERR_INVALID_ARGUMENT before anything is launched -- more rays than the context's pool may hold, a flag word that is none
    of the four, a ray outside the kernel's domain (a stored ray is finite and has a direction) -- and after each of them a good
    call on the same context gives the right records."""
    from nori_amd.render import Renderer
    sc, slots, want = xc.case("kind", "soup", 33, 1.0)
    r = Renderer(0).upload(sc, builder=0)

    def good(n=240):
        s = xc.take(slots, n)
        res, counts = r.extend(s["o"], s["dir_a"], s["dir_b"], s["maxt_b"], s["flags"])
        check("after a refusal", sc, s, xc.records_of(res), want[:n], counts)

    def refused(s, match):
        with pytest.raises(NoriError, match="NORI_ERR_INVALID_ARGUMENT") as e:
            r.extend(s["o"], s["dir_a"], s["dir_b"], s["maxt_b"], s["flags"])
        assert match in str(e.value), str(e.value)

    good()
    r.set_option("wavefront_paths", 256)
    refused(xc.take(slots, 257), "the pool of this context may hold 256")
    good(256)
    for word in (2, 4, 5, 7, 8, 0x101, 0x80000001):
        s = xc.take(slots, 240)
        s["flags"][17] = word
        refused(s, "flags[17]")
        good()
    a_slot = int(np.nonzero(slots["slot"][:240] == xc.SLOT_A)[0][0])
    b_slot = int(np.nonzero(slots["slot"][:240] == xc.SLOT_B)[0][0])
    for key, row, col, value in (("o", a_slot, 1, np.nan), ("o", b_slot, 0, np.inf), ("dir_a", a_slot, 2, np.nan), ("dir_a", a_slot, 0, -np.inf),
                                 ("dir_b", b_slot, 1, np.inf), ("maxt_b", b_slot, None, np.nan), ("maxt_b", b_slot, None, -np.inf)):
        s = xc.take(slots, 240)
        if col is None:
            s[key][row] = value
        else:
            s[key][row, col] = value
        refused(s, f"slot {row} ")
        good()
    for key, row in (("dir_a", a_slot), ("dir_b", b_slot)):
        s = xc.take(slots, 240)
        s[key][row] = np.float32([0.0, -0.0, 0.0])
        refused(s, f"slot {row} ")
        good()
    # what the flags do not name is not read: an empty slot may hold anything
    s = xc.take(slots, 240)
    e = int(np.nonzero(s["flags"] == 0)[0][0])
    s["o"][e] = np.nan; s["dir_a"][e] = 0.0; s["dir_b"][e] = np.inf
    res, counts = r.extend(s["o"], s["dir_a"], s["dir_b"], s["maxt_b"], s["flags"])
    check("garbage in an empty slot", sc, s, xc.records_of(res), want[:240], counts)
    # without flags every slot takes the kind the given directions make
    from tests.backends import Oracle
    o = Oracle(sc)
    s = xc.take(slots, 240)
    for da, db, word in ((s["dir_a"], None, 1), (None, s["dir_b"], 6), (s["dir_a"], s["dir_b"], 3)):
        kind = dict(s, flags=np.full(240, word, np.uint32))
        res, counts = r.extend(s["o"], da, db, None if db is None else s["maxt_b"])
        check(f"default flags {word}", sc, kind, xc.records_of(res), xc.expected_records(o, sc, kind), counts)
    o.close()
    r.close()
