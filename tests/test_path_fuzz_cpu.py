"""What the committed rounds of tests/path_fuzz.py (SEEDS) are worth, shown without a GPU: every path of every round ends well under
the walker's cap, the rounds between them reach every counter of path_ref.EVENTS and show every departure of path_ref.MUTATIONS,
they hold every kind of draw the generator has, and in the rounds with neither fog nor sky the CPU oracle's Li is a second witness
of the walker.  The same for the lit rounds (LIT_SEEDS: the round of the seed with drawn delta lights) against
tests/delta_lights_ref.py's counters and departures.  tests/test_gpu_path_fuzz.py renders these very rounds and compares bytes."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

from tests import delta_lights_ref as dl, path_cases as pc, path_fuzz as pf, path_ref as pr

SEEDS = pf.SEEDS


def _paths(ev, k):
    return int((ev[k] > 0).sum())


def test_seed_list():
    lo, hi = min(SEEDS + tuple(pf.SKIPPED)), max(SEEDS + tuple(pf.SKIPPED))
    assert sorted(SEEDS + tuple(pf.SKIPPED)) == list(range(lo, hi + 1)) and not set(SEEDS) & set(pf.SKIPPED)      # consecutive, minus SKIPPED
    assert 24 <= len(SEEDS) <= 40 and 8 * len(pf.SKIPPED) <= hi + 1 - lo
    assert 2 * pf.LONGEST <= pc.CAP == 256
    for seed, longest in pf.SKIPPED.items():      # a seed is skipped for one reason only, and the reason is measured
        assert pf.longest_path(seed) == longest > pf.LONGEST, (seed, pf.longest_path(seed))
    print("SKIPPED", pf.SKIPPED, "LONGEST", pf.LONGEST)


def test_every_path_of_every_round_ends():
    """(the walker asserts that no path is alive at path_cases.CAP; here: none takes more than LONGEST, half of it)"""
    longest = {seed: pf.longest_path(seed) for seed in SEEDS}
    print("longest path per seed", longest, "of all", max(longest.values()), "LONGEST", pf.LONGEST)
    assert max(longest.values()) <= pf.LONGEST, longest
    for seed in SEEDS:
        L, nc, ns, ev = pf.reference(seed)
        sc = pf.scene_of(seed)[0]
        assert L.shape == (sc.camera.width * sc.camera.height, 3) and int(ev["vertices"].sum()) == nc
        assert ns == 0 or sc.integrator.type != "path_mats"


def test_every_counter_is_reached():
    total = {k: sum(_paths(pf.reference(seed)[3], k) for seed in SEEDS) for k in pr.EVENTS}
    rounds = {k: [seed for seed in SEEDS if _paths(pf.reference(seed)[3], k) >= 8] for k in pr.FUZZ_EVENTS}
    print("paths per counter over SEEDS", total)
    print("rounds with at least 8 paths", rounds)
    assert set(pr.FUZZ_EVENTS) < set(pr.EVENTS) and set(pc.COUNTERS) | set(pr.FUZZ_EVENTS) == set(pr.EVENTS)
    for k in pr.EVENTS:
        assert total[k] >= 8, (k, total[k])
    for k in pr.FUZZ_EVENTS:
        assert len(rounds[k]) >= 2, (k, rounds[k])


@pytest.mark.parametrize("name", list(pr.MUTATIONS))
def test_every_departure_changes_paths_of_the_rounds(name):
    """under each round's own integrator; a round is walked again only where its reference took the branch (no other path can
    change: asserted on the walked rounds), and no further once 8 paths are shown twice over"""
    counters = pr.MUTATIONS[name]
    counters = (counters,) if isinstance(counters, str) else counters
    shown = {}
    for seed in SEEDS:
        L, _, _, ev = pf.reference(seed)
        reached = sum(ev[k] for k in counters) > 0
        if not reached.any():
            continue
        M = pf.walk(seed, mutate=name)[0]
        differs = (L.view(np.uint32) != M.view(np.uint32)).any(axis=1)
        assert not (differs & ~reached).any(), (name, seed)
        shown[seed] = int(differs.sum())
        if sum(shown.values()) >= 16:
            break
    print(name, "paths changed per round", shown)
    assert sum(shown.values()) >= 8, (name, shown)
    assert set(pr.FUZZ_MUTATIONS) | set(pc.SHOWN_ON) == set(pr.MUTATIONS)


def test_the_rounds_hold_every_kind_of_draw():
    rounds = [pf.scene_of(seed) for seed in SEEDS]
    scenes_ = [sc for sc, _, _ in rounds]
    meshes = [(sc, m) for sc in scenes_ for m in sc.meshes]
    assert {m.bsdf.type for _, m in meshes} == {"diffuse", "mirror", "dielectric", "microfacet"}
    assert {(m.bsdf.int_ior, m.bsdf.ext_ior) for _, m in meshes if m.bsdf.type == "dielectric"} == {(i, e) for i in pf.INT_IORS for e in pf.EXT_IORS}
    assert {m.bsdf.alpha for _, m in meshes if m.bsdf.type == "microfacet"} == set(pf.ALPHAS)
    textured = [(sc.textures[m.albedo_texture], m) for sc, m in meshes if m.albedo_texture is not None]
    assert {(t.filter, t.wrap) for t, _ in textured if t.kind == "image"} == {(f, w) for f in ("nearest", "bilinear") for w in ("repeat", "clamp")}
    assert {t.kind for t, _ in textured} == {"image", "checkerboard"} and {t.texels.shape[:2] for t, _ in textured if t.kind == "image"} == set(pf.IMAGE_SHAPES)
    for sc in scenes_:      # at least half of a round's textured meshes have texcoords, and they differ at the corners of every triangle
        tm = [m for m in sc.meshes if m.albedo_texture is not None]
        assert 2 * sum(m.texcoords is not None for m in tm) >= len(tm)
        for m in tm:
            if m.texcoords is not None:
                c = m.texcoords[m.indices.astype(np.int64)]
                assert all((c[:, i] != c[:, j]).any(axis=1).all() for i, j in ((0, 1), (1, 2), (2, 0)))
    assert any(m.texcoords is not None and m.name.startswith("sphere") for _, m in textured) and any(m.texcoords is None for _, m in textured)
    fog, sky = [sc for sc in scenes_ if sc.medium is not None], [sc for sc in scenes_ if sc.environment is not None]
    assert fog and sky and any(sc.medium is None and sc.environment is None for sc in scenes_) and not any(sc.medium is not None and sc.environment is not None for sc in scenes_)
    assert {float(sc.medium.g) for sc in fog} == set(pf.GS)
    assert {round(1.0 / (sc.medium.sigma_t * pf.SIZE), 6) for sc in fog} == set(pf.FREE_PATHS)
    assert any(max(sc.medium.albedo) == 1.0 for sc in fog) and any(min(sc.medium.albedo) == 0.0 for sc in fog)
    assert any(sc.camera.aperture_radius > 0 for sc in fog) and any(sc.camera.aperture_radius > 0 for sc in sky)
    lit = lambda sc: [m for m in sc.meshes if m.radiance is not None]
    only_sky = [sc for sc in sky if not lit(sc)]
    assert only_sky and any({m.bsdf.type for m in sc.meshes} & {"mirror", "dielectric", "microfacet"} for sc in only_sky)
    assert any(sc.integrator.type != "path_mats" for sc in only_sky)
    assert any("mirror" in {m.bsdf.type for m in sc.meshes} for sc in sky)
    assert {sc.environment.texels.shape[0] for sc in sky} == set(pf.MAP_SIZES) and any((sc.environment.texels == 0).all(axis=2).any() for sc in sky)
    lights = [m for sc in scenes_ for m in lit(sc)]
    assert any(m.normals is not None for m in lights) and any(max(m.bsdf.albedo) > 0 for m in lights) and any(m.name == "light_away" for m in lights)
    assert {b for _, b, _ in rounds} == {0, 1, 2} and {sc.integrator.type for sc in scenes_} == set(pf.PATHS)
    assert {b for (sc, b, _) in rounds if sc.environment is not None} >= {1, 2}      # the device's builders together with a sky
    assert {kn["S"] for _, _, kn in rounds} == set(pf.SAMPLE_INDICES)
    assert {kn["closed"] for _, _, kn in rounds} == {True, False} and any(kn["inside_glass"] for _, _, kn in rounds)
    for sc in scenes_:
        w, h = sc.camera.width, sc.camera.height
        assert 9 <= w <= 40 and 9 <= h <= 40 and (w % 16 or h % 16) and sc.rfilter.type == "box" and sc.sample_count == 1 and sc.n_triangles <= 800


def test_the_oracle_is_a_second_witness_where_there_is_neither_fog_nor_sky():
    """Oracle.li equals the walker byte for byte.  The oracle knows no textures: where a plain round has some, both sides walk
    the round without them (its geometry, BSDFs, lights, lens rays and streams)."""
    from tests.backends import Oracle
    plain = [seed for seed in SEEDS if pf.scene_of(seed)[0].medium is None and pf.scene_of(seed)[0].environment is None]
    assert len(plain) >= 8
    as_is = 0
    for seed in plain:
        sc = pf.scene_of(seed)[0]
        idx, seq, f, rays = pf.inputs(seed)
        if any(m.albedo_texture is not None for m in sc.meshes):
            sc = dataclasses.replace(sc, meshes=[dataclasses.replace(m, albedo_texture=None) for m in sc.meshes], textures=[])
            o = Oracle(sc, use_bvh=True)
            got = pc.walk_scene(sc, o, pf.inputs(seed), sc.integrator.type, True)[0]
        else:
            o, got, as_is = pf.oracle_of(seed), pf.walk(seed, True)[0], as_is + 1
        want = o.li(rays, idx, seq)
        assert got.tobytes() == want.tobytes(), (pf.describe(seed), int((got != want).any(axis=1).sum()))
    print("plain rounds", plain, "of them without a texture", as_is)


# ------------------------------------------------------------------ the lit rounds: scene_of(seed) with drawn delta lights
LIT = pf.LIT_SEEDS


def test_lit_seed_list():
    run = sorted(LIT + tuple(pf.LIT_SKIPPED))
    assert run == list(range(36, 60)) and not set(LIT) & set(pf.LIT_SKIPPED) and not set(run) & set(SEEDS + tuple(pf.SKIPPED))
    assert 8 * len(pf.LIT_SKIPPED) <= len(run)      # at most one round in eight
    for seed, longest in pf.LIT_SKIPPED.items():      # a seed is skipped for one reason only, and the reason is measured
        assert pf.longest_path(seed, lit=True) == longest > pf.LONGEST, (seed, pf.longest_path(seed, lit=True))
    print("LIT_SKIPPED", pf.LIT_SKIPPED, "LONGEST", pf.LONGEST)


def test_a_lit_round_is_its_plain_round_with_lights():
    """geometry, materials, textures, kind, lens, camera, builder, S and knobs are scene_of(seed)'s; the inputs and the oracle are shared"""
    for seed in LIT:
        (sc, b, kn), (lit, lb, lkn) = pf.scene_of(seed), pf.lit_scene_of(seed)
        assert lit.meshes is sc.meshes and lit.textures is sc.textures and lit.camera is sc.camera and lit.medium is sc.medium and lit.environment is sc.environment
        assert lb == b and {k: lkn[k] for k in kn} == kn and not sc.lights
        assert lit.integrator.type == ("path_ems", "path_mis")[seed % 2] and len(lit.lights) == pf.light_count_of(seed) == len(lkn["light_classes"])
        assert not (lit.medium is not None and any(l.type == "directional" for l in lit.lights))      # (the setter refuses it)


def test_every_path_of_every_lit_round_ends():
    longest = {seed: pf.longest_path(seed, lit=True) for seed in LIT}
    print("longest path per lit seed", longest, "of all", max(longest.values()), "LONGEST", pf.LONGEST)
    assert max(longest.values()) <= pf.LONGEST, longest
    brightest = {}
    for seed in LIT:
        L, nc, ns, ev = pf.reference(seed, lit=True)
        sc = pf.lit_scene_of(seed)[0]
        assert L.shape == (sc.camera.width * sc.camera.height, 3) and int(ev["vertices"].sum()) == nc and ns > 0
        assert np.isfinite(L).all()
        brightest[seed] = float(L.max())
    print("largest L per lit seed", brightest)


def test_every_light_counter_is_reached_in_two_lit_rounds():
    names = dl.EVENTS + dl.FUZZ_EVENTS
    rounds = {k: [seed for seed in LIT if _paths(pf.reference(seed, lit=True)[3], k) >= 8] for k in names}
    for seed in LIT:
        print(seed, {k: _paths(pf.reference(seed, lit=True)[3], k) for k in names})
    print("lit rounds with at least 8 paths", rounds)
    for k in names:
        assert len(rounds[k]) >= 2, (k, rounds[k])


@pytest.mark.parametrize("name", list(dl.MUTATIONS))
def test_every_light_departure_changes_paths_of_the_lit_rounds(name):
    """the loop of test_every_departure_changes_paths_of_the_rounds over the lit rounds and delta_lights_ref.MUTATIONS"""
    counters = dl.MUTATIONS[name]
    counters = (counters,) if isinstance(counters, str) else counters
    shown = {}
    for seed in LIT:
        L, _, _, ev = pf.reference(seed, lit=True)
        reached = sum(ev[k] for k in counters) > 0
        if not reached.any() or (name == "env_at_unshifted_index" and pf.lit_scene_of(seed)[0].environment is None):
            continue
        M = pf.walk(seed, mutate=name, lit=True)[0]
        differs = (L.view(np.uint32) != M.view(np.uint32)).any(axis=1)
        assert not (differs & ~reached).any(), (name, seed)
        shown[seed] = int(differs.sum())
        if sum(shown.values()) >= 16:
            break
    print(name, "paths changed per lit round", shown)
    assert sum(shown.values()) >= 8, (name, shown)


def test_the_lit_rounds_hold_every_kind_of_light_draw():
    rounds = [pf.lit_scene_of(seed) for seed in LIT]
    kinds_of = {}
    for sc, _, kn in rounds:
        kinds_of.setdefault(len(sc.lights), []).append(kn["kind"])
    print("light counts -> kinds", kinds_of)
    assert set(kinds_of) == set(pf.LIGHT_COUNTS)
    assert all(len(set(v)) >= 2 for v in kinds_of.values())                               # every count under at least two kinds
    assert len(kinds_of[4096]) >= 2
    assert sum(kn["kind"] == "fog" and len(sc.lights) >= 17 for sc, _, kn in rounds) >= 2
    assert {l.type for sc, _, _ in rounds for l in sc.lights} == {"point", "spot", "directional"}
    for seed, (sc, _, kn) in zip(LIT, rounds):
        classes, cones = kn["light_classes"], kn["light_cones"]
        assert len(classes) == len(cones) == len(sc.lights)
        for l, c, k in zip(sc.lights, classes, cones):
            assert (c == -1) == (l.type == "directional") and (k != -1) == (l.type == "spot")
            assert all(0.0 == x or 0.2 <= x <= 6.0 for x in l.intensity)
            if l.type == "spot":
                assert (l.cos_inner, l.cos_outer) == pf.cone_cosines(*pf.CONES[k]) and np.float32(l.cos_outer) <= np.float32(l.cos_inner)
        if len(sc.lights) >= 8:                                                            # in turn: all of them
            assert set(classes) - {-1} == set(range(len(pf.POSITION_CLASSES))), pf.describe(seed, True)
        # the positions are what their class says
        eye = sc.camera.to_world[:3, 3]
        verts = np.concatenate([m.positions for m in sc.meshes if m.name.startswith("sphere")])
        for l, c in zip(sc.lights, classes):
            p = np.array(l.position, np.float32)
            name = pf.POSITION_CLASSES[c] if c >= 0 else None
            if name == "in_a_wall_plane":
                assert p[1] == 2.0 or abs(p[0]) == 1.0
            elif name in ("just_inside_a_wall", "just_outside_a_wall"):
                off = np.concatenate([np.abs(np.abs(p[[0, 2]]) - 1.0), np.abs(p[1:2]), np.abs(p[1:2] - 2.0)]).min()
                outside = (np.abs(p[[0, 2]]) > 1.0).any() or p[1] < 0.0 or p[1] > 2.0
                assert 4e-5 < off < 6e-5 and outside == (name == "just_outside_a_wall")
            elif name == "at_a_sphere_vertex":
                assert (verts == p).all(axis=1).any()
            elif name == "at_the_eye":
                assert (p == eye).all()
            elif name == "above_the_box":
                assert p[1] == 5.0
    every = [l for sc, _, _ in rounds for l in sc.lights]
    assert {(l.cos_inner, l.cos_outer) for l in every if l.type == "spot"} == {pf.cone_cosines(*c) for c in pf.CONES}
    black = sum(not any(l.intensity) for l in every) / len(every)
    one_zero = sum(sorted(x == 0 for x in l.intensity) == [False, False, True] for l in every) / len(every)
    print("black lights", black, "one channel at zero", one_zero)
    assert 0.07 < black < 0.13 and 0.10 < one_zero < 0.18                                   # a tenth; a further seventh of all
    # a light at the centroid of a glass body, and of an opaque one
    inside = {m.bsdf.type for sc, _, kn in rounds for l, c in zip(sc.lights, kn["light_classes"]) if c == 5
              for m in sc.meshes if m.name.startswith("sphere") and np.abs(m.positions.astype(np.float64).mean(axis=0) - l.position).max() < 1e-6}
    assert "dielectric" in inside and inside - {"dielectric"}, inside
    # the combinations: the device's builders, a lens, the last sample index, fog, a sky as the only other light
    assert {b for _, b, _ in rounds} == {0, 1, 2}
    assert any(sc.camera.aperture_radius > 0 for sc, _, _ in rounds) and any(kn["S"] == (1 << 32) - 1 for _, _, kn in rounds)
    assert any(kn["S"] == 1 << 31 for _, _, kn in rounds) and any(kn["inside_glass"] for _, _, kn in rounds)
    assert any(sc.medium is not None for sc, _, _ in rounds)
    assert any(sc.environment is not None and not any(m.radiance is not None for m in sc.meshes) for sc, _, _ in rounds)
    assert {sc.integrator.type for sc, _, _ in rounds} == {"path_ems", "path_mis"}
    for sc, _, _ in rounds:
        w, h = sc.camera.width, sc.camera.height
        assert w <= 40 and h <= 40 and sc.n_triangles <= 800 and sc.sample_count == 1 and len(sc.lights) <= 4096
