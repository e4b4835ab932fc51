"""Scenes, rays and expected hit records for wf_extend driven ray by ray (Renderer.extend -> nori_hip_debug_extend), no GPU needed.

A case is a scene (fuzz_intersect.make_meshes: soup, duplicated, degenerate, sheet, stacked and mixed triangles at several sizes and
coordinate scales; the 30000-triangle soup whose device-built trees are deeper than the LDS stack; the empty scene) and a set of
path slots as wf_shade would store them: an origin, a continuation ray (slot A, closest hit) and / or a shadow ray (slot B, any hit),
or nothing.  The rays come in six classes of equal size, made where a tree walk is at its limits:

    A  aimed at a triangle vertex from a shell of radius 0.3 - 2.5 scene units
    B  aimed at a point of a triangle edge: parameter 0, 1/4, 1/2, 1 or random
    C  parallel to an axis, through the binary32 coordinates of a vertex exactly; half carry -0.0 in the two idle components
    D  origins 4000 scene sizes away, aimed at triangle centroids
    E  one direction component 0.0, -0.0, 1e-42 or -1e-42 (a denormal)
    F  origin exactly on a vertex or inside a triangle, random direction

Every ray has mint = 1e-4 unscaled, as every stored ray has.  The expected record of a slot comes from the linear scan of
tests/backends.Oracle (expected_records); the same function takes the CPU emulation of the device headers in its place, which is how
tests/test_extend_cases_cpu.py checks the expectation code before a GPU sees it."""
from __future__ import annotations

import functools

import numpy as np

from nori_amd import _capi as capi
from nori_amd.scene import Bsdf, Camera, Integrator, Mesh, RFilter, Scene
from tests import fuzz_intersect, scenes

KINDS = ("soup", "dups", "degenerate", "sheets", "stacked", "mixed")
SIZES = (1, 2, 3, 5, 8, 33, 500, 3000)
SCALES = (1.0, 1e-3, 1e3, 37.5)
CLASSES = "ABCDEF"
SLOT_EMPTY, SLOT_A, SLOT_B, SLOT_BA = range(4)
SLOT_FLAGS = np.array([0, capi.F_HAS_A, capi.F_HAS_B | capi.F_END_AFTER_B, capi.F_HAS_A | capi.F_HAS_B], np.uint32)
MINT = np.float32(1e-4)      # kEpsilon: mint of every stored ray, whatever the scene's scale
N_RAYS = 6000
MISS = np.array([0x7F800000, 0, 0, capi.EXTEND_MISS_A], np.uint32)      # (inf, 0, 0, kMissA)


def _camera():
    return Camera(16, 16, 45.0, to_world=scenes.lookat((0, 0, 4), (0, 0, 0), (0, 1, 0)))


def kind_scene(kind, n, scale, seed):
    """fuzz_intersect.make_meshes(kind, n, scale) as a scene (one to three meshes, no texture coordinates, no normals)."""
    rng = np.random.default_rng([seed, KINDS.index(kind), n, int(round(scale * 1000))])
    return Scene(fuzz_intersect.make_meshes(rng, kind, n, scale), _camera(), RFilter(), Integrator("normals"), 1)


def deep_scene():
    """The 30000-triangle soup (and its light) of test_hand_written_node_loop_equals_the_compilers: the device builders' trees of it
    are deeper than wf_extend's LDS stack."""
    sc = scenes.soup_scene(30000, seed=3, width=16, height=16, integrator="normals")
    v, f = scenes.quad((-3, 3, -3), (3, 3, -3), (3, 3, 3), (-3, 3, 3))
    sc.meshes.append(Mesh(v, f, bsdf=Bsdf("diffuse", (0, 0, 0)), radiance=(5.0, 5.0, 5.0), name="light"))
    return sc


def empty_scene():
    return Scene([], _camera(), RFilter(), Integrator("normals"), 1)


def scene_triangles(sc):
    """[T, 3, 3] float32: the scene's triangles in the order of their global indices (a mesh's follow those of the meshes before it)."""
    if not sc.meshes:
        return np.zeros((0, 3, 3), np.float32)
    return np.concatenate([m.positions[m.indices.astype(np.int64)] for m in sc.meshes]).astype(np.float32)


def _unit(d):
    d = np.asarray(d, np.float64)
    ln = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(ln > 0, d / np.where(ln > 0, ln, 1.0), np.array([0.0, 0.0, 1.0]))
    return d


def _shell(rng, m, lo, hi, scale):
    o = rng.normal(size=(m, 3))
    return o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(lo, hi, (m, 1)) * scale


def _class_rays(rng, c, m, tris, scale):
    """m rays of class c: (origins, primary directions, secondary directions from the same origins -- same class where the class
    is a property of the direction --, class data) as float32 arrays."""
    T = tris.astype(np.float64)
    nt = T.shape[0]
    pick = lambda: rng.integers(0, nt, m)      # noqa: E731
    verts = lambda: T[pick(), rng.integers(0, 3, m)]      # noqa: E731
    extra = None
    if c == "A":
        o = _shell(rng, m, 0.3, 2.5, scale)
        d1, d2 = _unit(verts() - o), _unit(verts() - o)
    elif c == "B":
        o = _shell(rng, m, 0.3, 2.5, scale)

        def edge_point():
            t, e = pick(), rng.integers(0, 3, m)
            a, b = T[t, e], T[t, (e + 1) % 3]
            s = np.where(rng.integers(0, 2, m) == 0, rng.choice([0.0, 0.25, 0.5, 1.0], m), rng.uniform(0, 1, m))[:, None]
            return a + s * (b - a)
        d1, d2 = _unit(edge_point() - o), _unit(edge_point() - o)
    elif c == "C":
        v = verts().astype(np.float32)
        axis = rng.integers(0, 3, m)
        side = rng.choice([-1.0, 1.0], m)
        o = v.copy()
        o[np.arange(m), axis] = (v[np.arange(m), axis].astype(np.float64) + side * rng.uniform(0.05, 2.5, m) * scale).astype(np.float32)

        def axis_dir(sign, negzero):
            d = np.where(negzero[:, None], np.float32(-0.0), np.float32(0.0)) * np.ones((m, 3), np.float32)
            d[np.arange(m), axis] = sign
            return d
        towards = (-side).astype(np.float32)
        d1 = axis_dir(towards, np.arange(m) % 2 == 1)                       # through the vertex, half with -0.0 in the idle components
        d2 = axis_dir(towards * rng.choice([-1.0, 1.0], m).astype(np.float32), rng.integers(0, 2, m) == 1)
        extra = (v, axis)
        return o, d1, d2, extra
    elif c == "D":
        far = rng.normal(size=(m, 3))
        o = far / np.linalg.norm(far, axis=1, keepdims=True) * 4000.0 * scale
        o32 = o.astype(np.float32).astype(np.float64)                      # aimed from where the ray really starts
        d1, d2 = _unit(T[pick()].mean(axis=1) - o32), _unit(T[pick()].mean(axis=1) - o32)
        o = o32
    elif c == "E":
        o = _shell(rng, m, 0.0, 2.5, scale)

        def special():
            d = _unit(rng.uniform(-1, 1, (m, 3)) * scale - o).astype(np.float32)
            minor = np.argsort(np.abs(d), axis=1)[np.arange(m), rng.integers(0, 2, m)]      # not the dominant one: the direction stays unit-ish
            d[np.arange(m), minor] = rng.choice(np.array([0.0, -0.0, 1e-42, -1e-42], np.float32), m)
            return d
        return o.astype(np.float32), special(), special(), extra
    elif c == "F":
        t = pick()
        w = rng.dirichlet([1.0, 1.0, 1.0], m).astype(np.float32)
        inside = (w[:, :1] * tris[t, 0] + w[:, 1:2] * tris[t, 1] + w[:, 2:] * tris[t, 2]).astype(np.float32)
        o = np.where((rng.integers(0, 2, m) == 0)[:, None], tris[t, rng.integers(0, 3, m)], inside)
        d1, d2 = _unit(rng.normal(size=(m, 3))), _unit(rng.normal(size=(m, 3)))
    else:
        raise ValueError(c)
    return np.asarray(o, np.float32), d1.astype(np.float32), d2.astype(np.float32), extra


def make_slots(seed, tris, scale, n=N_RAYS):
    """n path slots on the triangles `tris` [T, 3, 3] (T >= 1): dict of o [n, 3], dir_a [n, 3], dir_b [n, 3], maxt_b [n], flags [n]
    (uint32, capi.F_*), cls [n] (index into CLASSES), slot [n] (SLOT_*) -- and, for class C, c_vertex [n, 3] / c_axis [n] (the
    vertex and axis a ray was laid through; zeros elsewhere).  Every (class, slot kind) pair occurs n / 24 times, interleaved in a
    drawn order.  Slots A: maxt inf.  Slots B: half a finite maxt drawn as fuzz_intersect.make_rays draws it, half inf.  Slots
    B + A: the shadow ray takes the primary direction of the class, the continuation ray an independent second one."""
    assert n % 24 == 0 and len(tris) >= 1
    rng = np.random.default_rng([seed, 77])
    combo = rng.permutation(n) % 24
    cls, slot = (combo % 6).astype(np.int32), (combo // 6).astype(np.int32)
    o, d1, d2 = (np.zeros((n, 3), np.float32) for _ in range(3))
    c_vertex, c_axis = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    for k, c in enumerate(CLASSES):
        idx = np.nonzero(cls == k)[0]
        o[idx], d1[idx], d2[idx], extra = _class_rays(rng, c, len(idx), tris, scale)
        if extra is not None:
            c_vertex[idx], c_axis[idx] = extra
    has_b = (slot == SLOT_B) | (slot == SLOT_BA)
    maxt = np.full(n, np.inf, np.float32)
    finite = has_b & (rng.integers(0, 2, n) == 0)
    maxt[finite] = (rng.uniform(0.05, 3.0, int(finite.sum())) * scale).astype(np.float32)
    dir_a = np.where((slot == SLOT_A)[:, None], d1, d2)
    return {"o": o, "dir_a": dir_a, "dir_b": d1.copy(), "maxt_b": maxt, "flags": SLOT_FLAGS[slot].copy(), "cls": cls, "slot": slot,
            "c_vertex": c_vertex, "c_axis": c_axis}


def take(slots, n):
    """the first n slots (and n copies of the set in a row for n beyond it)"""
    m = len(slots["flags"])
    idx = np.arange(n) % m
    return {k: v[idx].copy() for k, v in slots.items()}


def rays_of(slots, which):
    """(indices of the slots that have ray `which` ("a" / "b"), those rays as capi.RAY_DTYPE records)"""
    bit = capi.F_HAS_A if which == "a" else capi.F_HAS_B
    idx = np.nonzero(slots["flags"] & bit)[0]
    rays = np.zeros(len(idx), dtype=capi.RAY_DTYPE)
    rays["o"] = slots["o"][idx]
    rays["d"] = slots["dir_a" if which == "a" else "dir_b"][idx]
    rays["mint"] = MINT
    rays["maxt"] = np.inf if which == "a" else slots["maxt_b"][idx]
    return idx, rays


def expected_records(backend, sc, slots):
    """[n, 4] uint32: the bits of the hit record wf_extend owes every slot -- (t, u, v) of the closest hit of the continuation ray and
    its GLOBAL triangle index, (inf, 0, 0) and kMissA without a hit or without that ray; bit 31 of the word: the shadow ray's answer;
    the sentinel where the slot is empty.  `backend`: tests.backends.Oracle(sc) (the linear scan) or anything with its intersect()."""
    n = len(slots["flags"])
    rec = np.full((n, 4), capi.EXTEND_SENTINEL, np.uint32)
    rec[slots["flags"] != 0] = MISS
    tri_offset = np.concatenate([[0], np.cumsum([m.indices.shape[0] for m in sc.meshes])]).astype(np.int64)
    ia, ra = rays_of(slots, "a")
    if len(ia):
        its = backend.intersect(ra)
        hit = its["mesh"] != capi.NO_HIT
        rows = ia[hit]
        rec[rows, 0] = its["t"][hit].view(np.uint32)
        rec[rows, 1] = np.ascontiguousarray(its["uv"][hit, 0]).view(np.uint32)
        rec[rows, 2] = np.ascontiguousarray(its["uv"][hit, 1]).view(np.uint32)
        rec[rows, 3] = (tri_offset[its["mesh"][hit].astype(np.int64)] + its["tri"][hit]).astype(np.uint32)
    ib, rb = rays_of(slots, "b")
    if len(ib):
        occluded = backend.intersect(rb, True)["mesh"] != capi.NO_HIT
        rec[ib[occluded], 3] |= np.uint32(capi.EXTEND_OCCLUDED_B)
    return rec


def expected_counts(slots):
    return {"n_closest_rays": int(((slots["flags"] & capi.F_HAS_A) != 0).sum()), "n_shadow_rays": int(((slots["flags"] & capi.F_HAS_B) != 0).sum())}


def records_of(extend_result):
    """Renderer.extend's (t, u, v, tri, occluded) as the [n, 4] uint32 records the kernel wrote"""
    t, u, v, tri, occ = extend_result
    word = tri.astype(np.uint32) | (occ.astype(np.uint32) << np.uint32(31))
    return np.stack([t.view(np.uint32), u.view(np.uint32), v.view(np.uint32), word], axis=1)


def exempted(sc, slots, got, want):
    """(rows that differ and are NOT ill-posed, number of differing rows the exemption of fuzz_intersect.ill_posed covers): a record
    may differ in its closest hit only where the continuation ray runs within 2e-3 rad of the plane of a triangle one side reports --
    there the reference's own t is rounding noise.  A differing shadow bit, or an empty slot that was written, is never exempt."""
    tris = [m.positions[m.indices.astype(np.int64)] for m in sc.meshes]
    tri_offset = np.concatenate([[0], np.cumsum([m.indices.shape[0] for m in sc.meshes])]).astype(np.int64)

    def as_hit(word):
        g = int(word) & capi.EXTEND_MISS_A
        if g == capi.EXTEND_MISS_A or g >= tri_offset[-1]:
            return {"mesh": 0xFFFFFFFF, "tri": 0}
        mesh = int(np.searchsorted(tri_offset, g, side="right") - 1)
        return {"mesh": mesh, "tri": g - int(tri_offset[mesh])}
    bad, tolerated = [], 0
    for r in np.nonzero((got != want).any(axis=1))[0]:
        same_shadow = (got[r, 3] ^ want[r, 3]) & np.uint32(capi.EXTEND_OCCLUDED_B) == 0
        if slots["flags"][r] & capi.F_HAS_A and same_shadow and fuzz_intersect.ill_posed({"d": slots["dir_a"][r]}, as_hit(got[r, 3]), as_hit(want[r, 3]), tris):
            tolerated += 1
        else:
            bad.append(int(r))
    return bad, tolerated


@functools.lru_cache(maxsize=None)
def case(name, *args):
    """(scene, slots, expected records) of a named case, computed once per process and shared: ("kind", kind, n, scale), ("deep",),
    ("empty",) -- the empty scene's rays are made on the triangles of a soup that is not in the scene."""
    from tests.backends import Oracle
    if name == "kind":
        kind, n, scale = args
        sc = kind_scene(kind, n, scale, seed=5)
        slots = make_slots(KINDS.index(kind) * 100 + SIZES.index(n), scene_triangles(sc), scale)
    elif name == "deep":
        sc = deep_scene()
        slots = make_slots(901, scene_triangles(sc), 1.0)
    elif name == "empty":
        sc = empty_scene()
        slots = make_slots(902, scene_triangles(kind_scene("soup", 33, 1.0, seed=5)), 1.0)
    else:
        raise ValueError(name)
    o = Oracle(sc)
    want = expected_records(o, sc, slots)
    o.close()
    return sc, slots, want
