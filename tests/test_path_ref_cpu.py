"""tests/path_ref.py checked without a GPU: byte for byte against the CPU oracle's Li on scenes with all four BSDF types (code it
shares nothing with: materials, eta, measures, MIS), against the two diffuse-only restatements (medium_ref.walk, restated_li) where
a fog or a sky is set, and -- on the very inputs tests/test_gpu_paths.py renders (tests/path_cases.py) -- that every branch under
test is reached by at least 8 paths and that taking it wrongly changes the radiance of at least 8 paths."""
from __future__ import annotations

import numpy as np
import pytest

from nori_amd.scene import Bsdf
from tests import light_cases as lc, medium_ref as mr, path_cases as pc, path_ref as pr, scenes
from tests.backends import Oracle

F = np.float32
PATHS = pc.PATHS
N_RAYS = 400
ORACLE_CAP = 300      # (no fog: the paths of these scenes end within 60 vertices; the walker asserts the cap)
ORACLE_SCENES = {
    "mirror_glass": lambda i: scenes.cornell_box(48, 32, 1, i, sphere_bsdfs=[Bsdf("mirror"), Bsdf("dielectric")]),
    "rough_glass": lambda i: scenes.cornell_box(48, 32, 1, i, sphere_bsdfs=[Bsdf("microfacet", (0.2, 0.3, 0.1), 0.2), Bsdf("dielectric")]),
    "R5": lambda i: lc.regime("R5", i),      # six lights, one of them with vertex normals; a microfacet and a diffuse sphere
}


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("integrator", PATHS)
@pytest.mark.parametrize("name", list(ORACLE_SCENES))
def test_walk_equals_the_oracle_path_for_path(name, integrator):
    sc = ORACLE_SCENES[name](integrator)
    assert all(m.normals is not None for m in sc.meshes if m.name.startswith("sphere"))
    o = Oracle(sc, use_bvh=True)
    rays, ss, sq = lc.li_inputs(o, sc, N_RAYS, seed=5)
    want = o.li(rays, ss, sq)
    f = Oracle.pcg32_floats(ss, sq, ORACLE_CAP * pr.DRAWS_PER_VERTEX)
    got, nc, ns, ev = pr.walk(o, sc, integrator, rays, f, max_vertices=ORACLE_CAP)
    assert got.tobytes() == want.tobytes(), (name, integrator, int((got != want).any(axis=1).sum()))
    assert (want > 0).any() and nc > N_RAYS and (ns > 0) == (integrator != "path_mats")
    # the comparison is about something: glass and roulette with eta != 1, vertex normals, microfacet emitter samples, a light with normals
    hit = lambda k: int((ev[k] > 0).sum())
    assert hit("hit_vertex_normals") >= 8
    if name != "R5":
        assert hit("rr_eta") >= 8
    if name != "mirror_glass" and integrator != "path_mats":
        assert hit("nee_microfacet_area") >= 8
    if name == "R5" and integrator != "path_mats":
        assert hit("pick_light_normals") >= 8
    assert all(not ev[k].any() for k in ("medium_vertex_prev_discrete", "env_escape_weighted", "env_escape_after_discrete", "shadow_tr_surface", "nee_textured"))


# ------------------------------------------------------------------ 2. against the two diffuse-only restatements
class CpuTwins:
    """what medium_ref.walk and restated_li ask of a renderer, from the CPU backends"""

    def __init__(self, scene):
        self.oracle, self.tables = Oracle(scene, use_bvh=True), pr.emitter_tables(scene)

    def intersect(self, rays, shadow=False):
        return self.oracle.intersect(rays, shadow=shadow)

    def warp(self, name, sample, param=0.0):
        return Oracle.warp(name, sample, param)

    def emitter_tables(self):
        return self.tables


def floor_inputs(sc, s, width, height, count):
    from tests import lens_ref as lr
    idx = np.arange(width * height, dtype=np.uint64)
    f = Oracle.pcg32_floats(idx, np.full(idx.shape, s, np.uint64), count)
    ps, _ = lr.camera_samples(width, height, s)
    return Oracle(sc).sample_rays(ps), f


@pytest.mark.parametrize("integrator", PATHS)
@pytest.mark.parametrize("g", [0.6, 0.0])
def test_walk_equals_medium_ref_on_the_lit_floor(integrator, g):
    from nori_amd.scene import Medium
    from tests import test_gpu_medium as tm
    med = Medium(tm.FOG.sigma_t, tm.FOG.albedo, g)
    ref = mr.Medium(med.sigma_t, med.albedo, med.g)
    sc = tm.lit_floor_scene(integrator, med)
    twins = CpuTwins(sc)
    rays, f = floor_inputs(sc, 3, tm.W, tm.H, 4 + tm.CAP * mr.DRAWS_PER_VERTEX)
    for floats in (f[:, 4:], f):
        want, nc, ns = mr.walk(twins, sc, ref, integrator, rays, floats, max_vertices=tm.CAP)
        got, gc, gs, ev = pr.walk(twins.oracle, sc, integrator, rays, floats, medium=med, max_vertices=tm.CAP)
        assert got.tobytes() == want.tobytes() and (gc, gs) == (nc, ns), (integrator, g, int((got != want).any(axis=1).sum()))
        assert (want > 0).any() and int(ev["vertices"].sum()) == nc


@pytest.mark.parametrize("integrator", PATHS)
def test_walk_equals_restated_li_on_the_floor_under_a_sky(integrator):
    from tests import test_gpu_envmap as te
    env = te.environment(7, "zeros")
    ref = te.ref_of(env)
    sc = te.floor_scene(integrator, env)
    twins = CpuTwins(sc)
    rays, f = floor_inputs(sc, 3, te.W, te.H, 4 + pr.MAX_VERTICES * pr.DRAWS_PER_VERTEX)
    for floats in (f[:, 4:], f):
        want, hit = te.restated_li(twins, sc, ref, integrator, rays, floats)
        got, nc, ns, _ = pr.walk(twins.oracle, sc, integrator, rays, floats, env=env)
        assert got.tobytes() == want.tobytes(), (integrator, int((got != want).any(axis=1).sum()))
        assert 0.5 < hit.mean() < 0.95 and (want[~hit] > 0).any() and (want[hit] > 0).any()
        assert nc == te.W * te.H + int(hit.sum())


# ------------------------------------------------------------------ 3. the GPU tests' inputs reach every branch
@pytest.mark.parametrize("integrator", PATHS)
@pytest.mark.parametrize("case", list(pc.CASES))
def test_inputs_of_the_gpu_cases_reach_every_branch(case, integrator):
    sc = pc.scene_of(case, integrator)
    assert (sc.medium is None) != (sc.environment is None) and sc.rfilter.type == "box"
    assert (sc.camera.width, sc.camera.height) == (pc.W, pc.H)
    assert lc.fits(lc.table_counts(sc)) == (case not in pc.OUTSIDE_LDS)
    L, nc, ns, ev = pc.reference(case, integrator)
    assert L.shape == (pc.N_PATHS, 3) and (L > 0).any()
    counts = {k: int((ev[k] > 0).sum()) for k in pc.COUNTERS}
    li_longest = int(pc.reference(case, integrator, True)[3]["vertices"].max())      # the stream drawn from the start (nori_hip_li) walks other paths
    print(case, integrator, "longest path", int(ev["vertices"].max()), "/", li_longest, counts)
    wanted = pc.applicable(sc, integrator)
    for k in pc.COUNTERS:
        if k in wanted:
            assert counts[k] >= 8, (case, integrator, k, counts[k])      # paths, not events: at least 8 PATHS take the branch
        else:
            assert counts[k] == 0, (case, integrator, k, counts[k])      # and a branch the scene does not have is never taken
    assert max(int(ev["vertices"].max()), li_longest) <= pc.LONGEST and 2 * pc.LONGEST < pc.CAP


def test_every_branch_is_reached_outside_the_lds_too():
    """what the two boxes reach between them is every counter; the LDSTAB = false scenes have no glass, texture or light with
    normals, and reach every other one"""
    reach = lambda cases: {k for c in cases for i in PATHS for k in pc.applicable(pc.scene_of(c, i), i)}
    assert reach(["fog_box", "sky_box"]) == set(pc.COUNTERS) == set(pr.EVENTS) - set(pr.FUZZ_EVENTS)
    assert reach(pc.OUTSIDE_LDS) == set(pc.COUNTERS) - {"rr_eta", "medium_vertex_after_specular", "medium_vertex_inside_glass", "env_escape_after_discrete",
                                                     "nee_textured", "pick_light_normals"}


def test_every_kind_of_case_is_there():
    kinds = {c: pc.scene_of(c, "path_mis") for c in pc.CASES}
    types = lambda sc: {m.bsdf.type for m in sc.meshes}
    assert types(kinds["fog_box"]) == {"diffuse", "mirror", "dielectric"} and types(kinds["sky_box"]) == {"diffuse", "microfacet", "dielectric"}
    assert kinds["fog_box"].medium.g == 0.6 and kinds["fog_r3"].medium is not None and kinds["sky_r4"].environment is not None
    assert kinds["sky_box_lens"].camera.aperture_radius > 0 and all(kinds[c].camera.aperture_radius == 0 for c in pc.CASES if c != "sky_box_lens")
    assert sorted(b for _, b in pc.CASES.values()) == [0, 0, 0, 0, 2]      # the default (device-built) tree for one, the host's for the others
    for c in ("fog_box", "sky_box"):
        assert any(m.albedo_texture is not None for m in kinds[c].meshes) and sum(m.radiance is not None for m in kinds[c].meshes) == 1


# ------------------------------------------------------------------ 4. a wrong branch changes these paths
@pytest.mark.parametrize("name", list(pc.SHOWN_ON))      # (path_ref.FUZZ_MUTATIONS: tests/test_path_fuzz_cpu.py, on its rounds)
def test_every_departure_changes_paths_the_gpu_renders(name):
    counters = pr.MUTATIONS[name]
    counters = (counters,) if isinstance(counters, str) else counters
    shown = {}
    for case in pc.CASES:
        for integrator in (PATHS if case in pc.SHOWN_ON[name] else PATHS[2:]):
            L, _, _, ev = pc.reference(case, integrator)
            M, _, _, _ = pc.walk(case, integrator, mutate=name)
            differs = (L.view(np.uint32) != M.view(np.uint32)).any(axis=1)
            reached = sum(ev[k] for k in counters) > 0
            assert not (differs & ~reached).any(), (name, case, integrator)      # only paths that took the branch can change
            print(name, case, integrator, int(differs.sum()), "of", int(reached.sum()), "paths that took the branch differ")
            if integrator == "path_mis":
                shown[case] = int(differs.sum())
    for case in pc.SHOWN_ON[name]:
        assert shown[case] >= 8, (name, case, shown[case])
