"""Delta lights (point, spot, directional) on the device, against tests/delta_lights_ref.py: the twin bit for bit, one diffuse quad
under one point light against the closed form, whole paths byte for byte -- nori_hip_li, the megakernel's and the wavefront
engine's frames, with equal ray counts -- on a box with mirror, glass, microfacet, a textured wall and an area emitter, with an
environment, in fog, and with the delta lights as the only lights, and on three scenes of many area lights whose emitter tables lie
outside the LDS (one per delta-light set); a light nearer than 2 kEpsilon; path_ems against path_mis statistically; unsetting, the upload
and every refusal.  tests/test_delta_lights_cpu.py shows without a GPU that the inputs used here (tests/delta_light_cases.py) reach
every new branch and that a branch taken wrongly changes their radiance."""
from __future__ import annotations

import numpy as np
import pytest

from nori_amd import NoriError, _capi
from nori_amd.render import DeviceGroup, Renderer
from nori_amd.scene import Light, Medium
from tests import delta_light_cases as dc, delta_lights_ref as dl, light_cases as lc, path_cases as pc, stat_harness as sh
from tests.backends import Oracle

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24
ENGINES = ("megakernel", "wavefront")


def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=1).sum())


# ------------------------------------------------------------------ 1. the twin
@pytest.mark.parametrize("n_lights", (1, 3, 257))
def test_the_twin_equals_incident_bit_for_bit(renderer_factory, n_lights):
    sc = dc.scene_of("a_each_type", "path_mis")
    r = renderer_factory(sc, build=False)
    rng = np.random.default_rng(n_lights)
    # a spot whose cones are the float32 c of two chosen points, and the same with a hard edge at the first
    base = Light("spot", (0.2, 1.9, -0.1), (0.3, -1.0, 0.2), (4.0, 3.0, 2.0), 0.5, 0.25)
    pts = rng.uniform((-1, 0, -1), (1, 1.5, 1), (64, 3)).astype(F)
    _, dirs, *_ = dl.incident_full([base], np.zeros(64, np.int64), pts)
    c = dl.dot(dl.Lights([base]).direction[[0] * 64], -dirs)
    order = np.argsort(c)
    lo, hi = int(order[20]), int(order[44])
    assert c[lo] < c[hi]
    edge = Light("spot", base.position, base.direction, base.intensity, float(c[hi]), float(c[lo]))
    hard = Light("spot", base.position, base.direction, base.intensity, float(c[hi]), float(c[hi]))
    lights = {1: [edge], 3: [Light("point", (0.3, 1.5, -0.2), intensity=(5, 4, 3)), dc.SUN, hard], 257: dc.many(255) + [hard, edge]}[n_lights]
    assert len(lights) == n_lights
    r.set_lights(lights)
    stored = r.lights
    ref = dl.Lights(lights)
    assert len(stored) == n_lights
    assert np.array([l.direction for l in stored], F).tobytes() == ref.direction.tobytes()      # normalised in float32, zero where unused
    assert np.array([l.position for l in stored], F).tobytes() == ref.position.tobytes()
    assert [l.type for l in stored] == [l.type for l in lights]
    # every light at random points; the last index at the 64 chosen points (c equal to a cone exactly at lo and hi); a point AT each
    # light that has a position
    m = 4096
    index = np.concatenate([rng.integers(0, n_lights, m), np.full(64, n_lights - 1), np.arange(n_lights)])
    p = np.concatenate([rng.uniform((-1.5, -0.5, -1.5), (1.5, 2.5, 1.5), (m, 3)).astype(F), pts, ref.position])
    got = r.light_incident(index, p)
    want = dl.incident(lights, index, p)
    for name, g, w in zip(("dir", "maxt", "radiance"), got, want):
        bad = int((g.view(np.uint32) != w.view(np.uint32)).reshape(len(index), -1).any(axis=1).sum())
        print(n_lights, name, bad, "of", len(index), "differ")
        assert g.tobytes() == w.tobytes(), (name, bad)
    # what the chosen points must show: full intensity AT the inner cone, nothing AT the outer (the edge light), and the hard
    # edge dark at its cone exactly (c <= cos_outer is asked first)
    if n_lights != 3:
        rad = got[2][m:m + 64]
        assert (rad[hi] == F(base.intensity)).all() and not rad[lo].any() and rad[order[21], 0] > 0
        assert ((rad[order[21:44], 0] > 0) & (rad[order[21:44], 0] <= 4)).all()
    else:
        rad = got[2][m:m + 64]
        assert len(set(c.tolist())) == 64
        assert (rad[order[45:]] == F(base.intensity)).all() and not rad[order[:45]].any()      # the hard edge: dark up to c == cos_outer, fully lit above
    at = slice(m + 64, None)
    has_pos = ref.type != dl.DIRECTIONAL
    assert not got[2][at][has_pos].any() and not got[1][at][has_pos].any()      # a point at the light: no sample
    with pytest.raises(NoriError, match="INVALID_ARGUMENT.*light index"):
        r.light_incident([n_lights], np.zeros((1, 3), F))


# ------------------------------------------------------------------ 2. one diffuse quad under one point light
def quad_inputs(sc):
    return pc.inputs_of(sc, 0)


def test_a_diffuse_quad_under_a_point_light_against_the_closed_form(renderer_factory):
    scs = {i: dc.quad_scene(i) for i in dc.INTEGRATORS}
    idx, seq, f, rays = quad_inputs(scs["path_mis"])
    assert rays.shape[0] == 4096
    oracle = Oracle(scs["path_mis"], use_bvh=True)
    li = {}
    for integ, sc in scs.items():
        r = renderer_factory(sc)
        assert [l.type for l in r.lights] == ["point"]
        want, nc, ns, ev = dl.walk(oracle, sc, integ, rays, f, max_vertices=dc.CAP)
        li[integ] = r.li(rays, idx, seq)
        assert li[integ].tobytes() == want.tobytes(), (integ, differing(li[integ], want))
    assert li["path_ems"].tobytes() == li["path_mis"].tobytes()      # the only light is a delta light: weight 1 under both
    # rho / pi  I cos(theta) / d^2 in binary64 at the oracle's float32 hit point.  Rounded operations on the way, u = 2^-24 each,
    # first order: dvec u; dist2 (three products, two sums of positive terms) 3 u on top of dvec's 2 u = 5 u; dist 2.5 u + u;
    # dir.y = dvec.y / dist: u + 3.5 u + u = 5.5 u, and wo.z IS dir.y (the quad's frame is the axes: products with 0 and 1);
    # the divisor dist2 pdfPick with pdfPick = 1: 5 u; the quotient 5.5 u + 5 u + u = 11.5 u; f = albedo kInvPi: the constant's u and the
    # product's; f R: u; times the quotient: u.  16 u in all; T = 1, w = 1 and L = 0 + Ld add nothing.
    its = oracle.intersect(rays, shadow=False)
    hit = its["mesh"] != 0xFFFFFFFF
    assert hit.sum() > 3500
    p = its["p"].astype(np.float64)
    dv = np.array(dc.QUAD_LIGHT.position, F).astype(np.float64) - p
    d2 = (dv * dv).sum(1)
    cos = dv[:, 1] / np.sqrt(d2)
    expect = np.array(dc.RHO, F).astype(np.float64) / np.pi * np.array(dc.QUAD_LIGHT.intensity, F).astype(np.float64) * (cos / d2)[:, None]
    got = li["path_mis"].astype(np.float64)
    rel = np.abs(got[hit] / expect[hit] - 1)
    print("quad: largest relative deviation", rel.max() / U, "u of 16 u allowed")
    assert rel.max() <= 16 * U * 1.01
    assert not got[~hit].any()


def test_the_umbra_of_an_occluder_is_exactly_zero_with_equal_ray_counts(renderer_factory):
    sc = dc.quad_scene("path_mis", occluder=True)
    idx, seq, f, rays = quad_inputs(sc)
    oracle = Oracle(sc, use_bvh=True)
    want, nc, ns, ev = dl.walk(oracle, sc, "path_mis", rays, f[:, 4:], max_vertices=dc.CAP)
    # the umbra: camera rays that reach the quad (mesh 0) where the light is behind the occluder, by plain geometry in binary64
    its = oracle.intersect(rays, shadow=False)
    on_quad = its["mesh"] == 0
    p = its["p"].astype(np.float64)
    lp = np.array(dc.QUAD_LIGHT.position, F).astype(np.float64)
    t = (1.0 - p[:, 1]) / (lp[1] - p[:, 1])
    q = p + (lp - p) * t[:, None]
    inside = on_quad & (q[:, 0] > 0.01) & (q[:, 0] < 0.59) & (q[:, 2] > -0.49) & (q[:, 2] < 0.09)      # (a margin of 0.01 off the occluder's edges)
    assert inside.sum() > 50
    r = renderer_factory(sc)
    for engine in ENGINES:
        r.set_option("engine", engine)
        frame, st = r.render_host(spp_count=1, spp_begin=0)
        got = frame[..., :3].reshape(-1, 3)
        assert got.tobytes() == want.tobytes(), (engine, differing(got, want))
        assert (st["n_closest_rays"], st["n_shadow_rays"]) == (nc, ns), engine
        assert not got[inside].any() and (got[on_quad & ~inside] > 0).any()


def test_a_light_nearer_than_two_epsilon_leaves_an_empty_shadow_interval(renderer_factory):
    """The header's rule for dist < 2 kEpsilon: maxt = dist - kEpsilon lies below the shadow ray's mint (below 0 for dist < kEpsilon),
    no t satisfies mint <= t <= maxt, the ray is traced and counted and the sample is added.  256 rays aimed at the quad around the
    foot of a point light 3e-5 above it, at 0 to 4e-4 from the foot: both sides of dist = kEpsilon and of dist = 2 kEpsilon."""
    near = Light("point", position=(0.3, 3e-5, -0.2), intensity=(1e-8, 2e-8, 3e-8))
    k = np.arange(256)
    rad, ang = 4e-4 * k / 256, 2.399963 * k
    target = np.stack([0.3 + rad * np.cos(ang), np.zeros(256), -0.2 + rad * np.sin(ang)], 1)
    idx, seq = k.astype(np.uint64), np.full(256, 7, np.uint64)
    f = Oracle.pcg32_floats(idx, seq, 4 + dc.CAP * dl.DRAWS_PER_VERTEX)
    for integ in dc.INTEGRATORS:
        sc = dc.quad_scene(integ)
        sc.lights = [near]
        oracle = Oracle(sc, use_bvh=True)
        rays = oracle.sample_rays(np.full((256, 2), 32.0, F)).copy()
        d = target - rays["o"].astype(np.float64)
        rays["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
        want, nc, ns, ev = dl.walk(oracle, sc, integ, rays, f, max_vertices=dc.CAP)
        below_eps = int(((ev["delta_empty_interval"] > 0) & (np.linalg.norm(target - near.position, axis=1) < 1e-4)).sum())
        print(integ, "paths with maxt < mint:", int((ev["delta_empty_interval"] > 0).sum()), "of them with maxt < 0:", below_eps, "shadow rays", ns)
        assert (ev["delta_empty_interval"] > 0).sum() >= 64 and below_eps >= 16 and (ev["delta_shadow"] > ev["delta_empty_interval"]).sum() >= 64
        assert (want[ev["delta_empty_interval"] > 0] > 0).all()      # lit: nothing lies in an empty interval
        got = renderer_factory(sc).li(rays, idx, seq)
        print(integ, differing(got, want), "of 256 paths differ")
        assert got.tobytes() == want.tobytes(), (integ, differing(got, want))


# ------------------------------------------------------------------ 3., 4. whole paths, byte for byte
@pytest.mark.parametrize("integrator", dc.INTEGRATORS)
@pytest.mark.parametrize("case", list(dc.CASES))
def test_paths_equal_the_reference_bit_for_bit(renderer_factory, case, integrator):
    sc = dc.scene_of(case, integrator)
    r = renderer_factory(sc)
    assert len(r.lights) == len(sc.lights) and (r.medium is not None) == (sc.medium is not None) and (r.environment_size > 0) == (sc.environment is not None)
    assert (r.emitter_tables()["n_emitters"] == 0) == case.endswith(("lights_only", "lights_only_sky"))
    # the emitter tables: in the LDS, or -- the OUTSIDE_LDS cases -- read from global memory (wf_shade's LDSTAB = false variants)
    assert lc.fits(lc.table_counts(sc)) == (case not in dc.OUTSIDE_LDS)
    if case in dc.OUTSIDE_LDS:
        assert not lc.fits(lc.table_counts(sc))
    w, h = dc.size_of(case)
    # 1. Li of the stated rays, its stream seeded like the render's and drawn from the start: 1024 paths of each of four samples
    per = dc.N_LI // len(dc.SAMPLES)
    for s in dc.SAMPLES:
        idx, seq, f, rays = dc.inputs(case, s)
        want_li, _, _, _ = dc.reference(case, integrator, s, True, per)
        got_li = r.li(rays[:per], idx[:per], seq[:per])
        assert got_li.tobytes() == want_li.tobytes(), (case, integrator, s, differing(got_li, want_li))
    # 2. both engines' frames of one sample per pixel under the box filter, four samples: a pixel is Li of its path
    frames = {}
    for s in dc.SAMPLES:
        want, nc, ns, _ = dc.reference(case, integrator, s)
        assert (want > 0).any() and nc > w * h and ns > 0
        for engine in ENGINES:
            r.set_option("engine", engine)
            frame, st = r.render_host(spp_count=1, spp_begin=s)
            assert st["engine"] == ENGINES.index(engine) and st["n_camera_samples"] == w * h and frame.shape == (h, w, 4)
            got = frame[..., :3].reshape(-1, 3)
            print(case, integrator, engine, s, ":", differing(got, want), "paths differ; rays", st["n_closest_rays"], st["n_shadow_rays"], "want", nc, ns)
            assert got.tobytes() == want.tobytes(), (case, integrator, engine, s, differing(got, want))
            assert (st["n_closest_rays"], st["n_shadow_rays"]) == (nc, ns), (case, integrator, engine, s)
            assert st["n_invalid"] == 0
            if engine == "wavefront":
                assert st["wf_record"] == "full"
            frames[engine, s] = frame
    # 3. a quarter of the samples in flight: regeneration, many passes, wf_finish
    r.set_option("wavefront_paths", w * h // 4)
    small, st = r.render_host(spp_count=1, spp_begin=dc.SAMPLES[-1])
    assert st["engine"] == 1 and st["n_invalid"] == 0
    assert small.tobytes() == frames["wavefront", dc.SAMPLES[-1]].tobytes()


# ------------------------------------------------------------------ 5. path_ems against path_mis, statistically
@pytest.mark.parametrize("case", list(dc.STAT_CASES))
def test_path_ems_and_path_mis_agree_statistically(renderer_factory, case):
    """Both estimate the same integral.  64 samples per pixel of the 48 x 32 frame under each; the per-pixel differences of luminance
    (independent across pixels, mean 0 if both are unbiased) go to Student's t-test at the harness's own level of 0.01, two tests.
    The box is the bitwise cases' with ONE change: its area emitter has no vertex normals.  With path_cases.box's leaning normals
    the two integrators estimate different integrals -- an emitter sample converts area to solid angle with the shading normal's
    cosine, a BSDF-sampled hit does not -- and the test says so: on light set (a) the means are 1.25397 and 1.26386, p = 0.0004,
    from the device and, to every digit, from the CPU walker alone; with the geometric normal the walker gives p = 0.52."""
    lum = {}
    for integ in dc.INTEGRATORS:
        r = renderer_factory(dc.STAT_CASES[case](integ))
        assert len(r.lights) == 3
        frame, st = r.render_host(spp_count=64, spp_begin=16)
        assert st["n_invalid"] == 0
        rgb = (frame[..., :3] / frame[..., 3:4]).reshape(-1, 3)
        lum[integ] = sh.luminance(rgb)
    diff = lum["path_ems"] - lum["path_mis"]
    ok, info = sh.students_t_test(diff, 0.0, 0.01, 2)
    print(case, info, "means", lum["path_ems"].mean(), lum["path_mis"].mean())
    assert ok, info
    assert lum["path_mis"].mean() > 0.1


# ------------------------------------------------------------------ 6. unsetting, the upload, errors, the group
def test_unsetting_gives_back_the_bytes_of_a_context_without_lights_and_an_upload_resets(renderer_factory):
    import dataclasses
    lit = dc.scene_of("a_each_type", "path_mis")
    plain = dataclasses.replace(lit, lights=[])
    never, st0 = renderer_factory(plain).render_host(spp_count=2)
    r = renderer_factory(lit)
    with_lights, st1 = r.render_host(spp_count=2)
    assert with_lights.tobytes() != never.tobytes() and st1["n_shadow_rays"] != st0["n_shadow_rays"]
    r.set_lights([])
    assert r.lights == []
    for engine in ENGINES:
        r.set_option("engine", engine)
        again, st = r.render_host(spp_count=2)
        assert st["n_shadow_rays"] == st0["n_shadow_rays"] and st["n_closest_rays"] == st0["n_closest_rays"]
        if engine == ENGINES[st0["engine"]]:
            assert again.tobytes() == never.tobytes()
    r.set_lights(lit.lights)
    assert len(r.lights) == 3
    r.upload(plain)      # an upload resets them
    assert r.lights == []
    with pytest.raises(NoriError, match="NOT_READY.*no lights set"):
        r.light_incident([0], np.zeros((1, 3), F))


def test_every_refusal_comes_with_its_message(renderer_factory):
    import dataclasses
    fresh = Renderer(0)
    try:
        with pytest.raises(NoriError, match="NOT_READY.*no scene uploaded"):
            fresh.set_lights([dc.POINT])
    finally:
        fresh.close()
    lit = dc.scene_of("a_each_type", "path_mis")
    r = renderer_factory(lit)
    stored = r.lights
    nan, inf = float("nan"), float("inf")
    bad = [
        (Light("point", (nan, 0, 0)), "position is not finite"),
        (Light("point", (0, 0, 0), intensity=(1, inf, 1)), "intensity is not finite"),
        (Light("point", (0, 0, 0), intensity=(1, -0.5, 1)), "intensity is negative"),
        (Light("directional", direction=(0, 0, 0)), "direction has zero length"),
        (Light("spot", direction=(0, nan, 0), cos_inner=0.5, cos_outer=0.2), "direction is not finite"),
        (Light("spot", direction=(0, -1, 0), cos_inner=0.2, cos_outer=0.5), "cos_outer <= cos_inner"),
        (Light("spot", direction=(0, -1, 0), cos_inner=1.5, cos_outer=0.5), "cos_outer <= cos_inner"),
        (Light("spot", direction=(0, -1, 0), cos_inner=nan, cos_outer=0.5), "cosine of the cone is not finite"),
    ]
    for light, word in bad:
        with pytest.raises(NoriError, match="INVALID_ARGUMENT.*set_lights: light 1: .*" + word):
            r.set_lights([dc.POINT, light])
        assert r.lights == stored      # a failed call leaves the stored lights as they were
    arr = (_capi.LightDesc * 1)(dc.POINT.desc())
    arr[0].type = 3
    assert r._lib.nori_hip_set_lights(r._h, 1, arr) == -1 and b"unknown type 3" in r._lib.nori_hip_last_error(r._h)
    with pytest.raises(NoriError, match="INVALID_ARGUMENT.*4097 lights, at most 4096"):
        r.set_lights([dc.INSIDE] * 4097)
    r.set_lights([dc.INSIDE] * 4096)
    assert len(r.lights) == 4096
    r.set_lights(lit.lights)
    # NORI_SEED_NORI_BLOCK
    with pytest.raises(NoriError, match="UNSUPPORTED.*NORI_SEED_NORI_BLOCK renders no delta lights"):
        r.render_host(seed_mode=_capi.SEED_NORI_BLOCK)
    # a directional light and a medium exclude each other, whichever comes first
    with pytest.raises(NoriError, match="UNSUPPORTED.*set_medium.*directional light"):
        r.set_medium(pc.FOG)
    assert r.medium is None and r.lights == stored
    r.set_lights([dc.INSIDE, dc.SPOT])
    r.set_medium(pc.FOG)
    with pytest.raises(NoriError, match="UNSUPPORTED.*set_lights: a directional light in a context with a medium"):
        r.set_lights([dc.SUN])
    assert [l.type for l in r.lights] == ["point", "spot"] and r.medium is not None
    # every integrator but path_ems and path_mis
    for integ in ("path_mats", "whitted", "simple", "ao", "normals"):
        q = renderer_factory(dc.box(integ, []))
        with pytest.raises(NoriError, match="UNSUPPORTED.*only path_ems and path_mis render delta lights"):
            q.set_lights([dc.POINT])
        assert q.lights == []


def test_the_group_sets_and_renders_lights(renderer_factory):
    sc = dc.scene_of("a_each_type", "path_mis")
    one, _ = renderer_factory(sc).render_host()
    g = DeviceGroup([0])
    try:
        g.upload(sc)
        frame, _, _ = g.render_host()
        assert frame.tobytes() == one.tobytes()
        g.set_lights([])
        dark, _, _ = g.render_host()
        assert dark.tobytes() != one.tobytes()
        with pytest.raises(NoriError, match="intensity is negative"):
            g.set_lights([Light("point", intensity=(-1, 0, 0))])
    finally:
        g.close()
