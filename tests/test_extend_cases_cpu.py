"""tests/extend_cases.py on the CPU: the generator is deterministic and makes what it claims, and the device headers compiled for
the host (tests/emu) give the oracle's records on its rays for both node layouts -- which also checks the expectation code of
tests/test_gpu_extend.py before a GPU sees it."""
import numpy as np
import pytest

from nori_amd import _capi as capi
from tests import extend_cases as xc
from tests.backends import Emu, Oracle

# every kind at every size, the scales going round
CPU_CASES = [(kind, n, xc.SCALES[(i + j) % len(xc.SCALES)]) for j, kind in enumerate(xc.KINDS) for i, n in enumerate(xc.SIZES)]


def test_generator_is_deterministic():
    for kind, n, scale in (("soup", 33, 1.0), ("sheets", 500, 1e-3)):
        a, b = xc.kind_scene(kind, n, scale, seed=5), xc.kind_scene(kind, n, scale, seed=5)
        assert len(a.meshes) == len(b.meshes)
        for ma, mb in zip(a.meshes, b.meshes):
            assert np.array_equal(ma.positions.view(np.uint32), mb.positions.view(np.uint32)) and np.array_equal(ma.indices, mb.indices)
        sa, sb = xc.make_slots(11, xc.scene_triangles(a), scale), xc.make_slots(11, xc.scene_triangles(b), scale)
        other = xc.make_slots(12, xc.scene_triangles(a), scale)
        for k in sa:
            view = (lambda x: x.view(np.uint32)) if sa[k].dtype == np.float32 else (lambda x: x)
            assert np.array_equal(view(sa[k]), view(sb[k])), k
        assert not np.array_equal(sa["o"], other["o"])


@pytest.mark.parametrize("kind,n,scale", [c for c in CPU_CASES if c[1] in (1, 33, 3000)] + [("empty", 0, 1.0)])
def test_every_class_and_slot_kind_is_present_and_is_what_it_claims(kind, n, scale):
    sc, s, want = xc.case("empty") if kind == "empty" else xc.case("kind", kind, n, scale)
    tris = xc.scene_triangles(sc) if kind != "empty" else xc.scene_triangles(xc.kind_scene("soup", 33, 1.0, seed=5))
    N = xc.N_RAYS
    counts = np.zeros((6, 4), np.int64)
    np.add.at(counts, (s["cls"], s["slot"]), 1)
    assert (counts == N // 24).all()                                     # six classes of equal size, every slot kind in each
    assert len(set(np.diff(np.nonzero(s["slot"] == xc.SLOT_EMPTY)[0]))) > 1      # interleaved, not in blocks
    assert set(np.unique(s["flags"])) == {0, 1, 3, 6}
    fa, fb = (s["flags"] & capi.F_HAS_A) != 0, (s["flags"] & capi.F_HAS_B) != 0
    for d, used in ((s["dir_a"], fa), (s["dir_b"], fb)):
        assert np.isfinite(d[used]).all() and (np.abs(d[used]).max(axis=1) > 0.5).all()      # finite, unit-ish, never zero
    assert np.isfinite(s["o"]).all() and not np.isnan(s["maxt_b"]).any() and (s["maxt_b"] > 0).all()
    finite_maxt = np.isfinite(s["maxt_b"])
    assert not finite_maxt[~fb].any() and 0.3 < finite_maxt[fb].mean() < 0.7
    ba = s["slot"] == xc.SLOT_BA
    # an independent direction each (with a handful of vertices two draws often aim at the same one)
    assert (s["dir_a"][ba].view(np.uint32) != s["dir_b"][ba].view(np.uint32)).any(axis=1).mean() > (0.7 if n == 0 or n >= 33 else 0.4)
    verts = tris.reshape(-1, 3)
    vbits = {v.tobytes() for v in verts}
    # C: axis-parallel, through a vertex's binary32 coordinates exactly, half with -0.0 in the idle components
    c = np.nonzero(s["cls"] == 2)[0]
    assert all(s["c_vertex"][i].tobytes() in vbits for i in c)
    idle = np.array([[k for k in range(3) if k != a] for a in s["c_axis"][c]])
    rows = np.arange(len(c))[:, None]
    assert np.array_equal(s["o"][c][rows, idle].view(np.uint32), s["c_vertex"][c][rows, idle].view(np.uint32))
    assert (s["o"][c][np.arange(len(c)), s["c_axis"][c]] != s["c_vertex"][c][np.arange(len(c)), s["c_axis"][c]]).all()
    for d in (s["dir_a"][c], s["dir_b"][c]):
        assert (np.abs(d[np.arange(len(c)), s["c_axis"][c]]) == 1.0).all() and (d[rows, idle] == 0.0).all()
        neg = np.signbit(d[rows, idle])
        assert (neg[:, 0] == neg[:, 1]).all() and 0.3 < neg[:, 0].mean() < 0.7
    # D: 4000 scene sizes away
    dist = np.linalg.norm(s["o"][s["cls"] == 3].astype(np.float64), axis=1) / scale
    assert np.allclose(dist, 4000.0, rtol=1e-6)
    # E: one component of the class's direction is a zero of either sign or a denormal of either sign
    e = s["cls"] == 4
    special = {np.float32(x).tobytes() for x in (0.0, -0.0, 1e-42, -1e-42)}
    seen = set()
    for d in s["dir_b"][e]:
        hit = [x.tobytes() for x in d if x.tobytes() in special]
        assert hit
        seen.update(hit)
    assert seen == special
    # F: the origin is a vertex, bit for bit, in about half of the rays
    on_vertex = np.mean([o.tobytes() in vbits for o in s["o"][s["cls"] == 5]])
    assert 0.3 < on_vertex < 0.7
    # A: the primary direction points at a vertex
    a = np.nonzero(s["cls"] == 0)[0][:50]
    for i in a:
        to = verts.astype(np.float64) - s["o"][i].astype(np.float64)
        cosang = (to @ s["dir_b"][i].astype(np.float64)) / np.maximum(np.linalg.norm(to, axis=1), 1e-300)
        assert cosang.max() > 1 - 1e-6
    # the expectation: empty slots keep the sentinel, everything else was written
    empty = s["slot"] == xc.SLOT_EMPTY
    assert (want[empty] == capi.EXTEND_SENTINEL).all() and (want[~empty, 0] != capi.EXTEND_SENTINEL).all()
    only_b = s["slot"] == xc.SLOT_B
    assert (want[only_b, :3] == xc.MISS[:3]).all() and ((want[only_b, 3] & capi.EXTEND_MISS_A) == capi.EXTEND_MISS_A).all()
    assert xc.expected_counts(s) == {"n_closest_rays": N // 2, "n_shadow_rays": N // 2}
    if kind == "empty":
        assert (want[~empty] == xc.MISS).all()
    elif n >= 33:
        hit = (want[:, 3] & capi.EXTEND_MISS_A) != capi.EXTEND_MISS_A
        assert hit[fa].mean() > 0.05 and (want[fb, 3] >> 31).mean() > 0.05      # the rays do meet the scene


@pytest.mark.parametrize("layout", ["bvh2", "bvh2, 64-B nodes", "bvh4q"])
@pytest.mark.parametrize("kind,n,scale", CPU_CASES + [("sheets", 3000, 1.0), ("empty", 0, 1.0)])
def test_emu_gives_the_oracles_records(monkeypatch, layout, kind, n, scale):
    """The tree walk of the device headers (rt_trace.h, compiled for the host) against the linear scan, record for record and bit for
    bit, with no ray exempted: BVH2 trees through their 32-B records where they have them (trav_inner_step_q, what the harness walks
    by default) and through the 64-B nodes (trav_inner_step: the megakernel, wf_finish, the batch twins, wf_extend's compiler loop),
    and wide nodes.  (sheets x3000 at scale 1: where the 64-B step once culled the box of a hit that ties with the current one, for
    origins 4000 scene sizes away -- the limit it holds a box's near side to is now widened like the far side.)"""
    monkeypatch.setenv("NORI_HIP_ACCEL_LAYOUT", layout.split(",")[0])
    if "64-B" in layout:
        monkeypatch.setenv("NORI_EMU_NODEQ", "0")
    sc, slots, want = xc.case("empty") if kind == "empty" else xc.case("kind", kind, n, scale)
    e = Emu(sc)
    if kind != "empty" and n >= 8:
        assert e.accel_info()["node_children"] == (4 if layout == "bvh4q" else 2)
    if "64-B" in layout:
        assert e.accel_info()["node_records_32b"] == 0
    got = xc.expected_records(e, sc, slots)
    e.close()
    bad, tolerated = xc.exempted(sc, slots, got, want)
    print(f"[extend cpu] {kind} x{n} scale {scale} {layout}: {len(bad)} records differ, {tolerated} exempted")
    assert not bad, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert tolerated == 0


def test_the_deep_soup_on_the_cpu():
    """The 30000-triangle case of the GPU tests (its device-built trees are deeper than the LDS stack): host-built tree, 64-B nodes."""
    sc, slots, want = xc.case("deep")
    e = Emu(sc)
    got = xc.expected_records(e, sc, slots)
    e.close()
    bad, tolerated = xc.exempted(sc, slots, got, want)
    assert not bad and tolerated == 0
    tri = want[slots["flags"] != 0, 3] & capi.EXTEND_MISS_A
    assert len(sc.meshes) == 2 and ((tri >= 30000) & (tri < 30002)).sum() > 0      # some hits lie in the second mesh: the offset counts
