"""What the committed rounds of tests/path_fuzz.py (SEEDS) are worth, shown without a GPU: every path of every round ends well under
the walker's cap, the rounds between them reach every counter of path_ref.EVENTS and show every departure of path_ref.MUTATIONS,
they hold every kind of draw the generator has, and in the rounds with neither fog nor sky the CPU oracle's Li is a second witness
of the walker.  tests/test_gpu_path_fuzz.py renders these very rounds and compares bytes."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

from tests import path_cases as pc, path_fuzz as pf, path_ref as pr

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
