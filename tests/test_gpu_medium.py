"""The homogeneous medium on the GPU (include/nori_hip.h, "Homogeneous participating medium") against the numpy restatement of
tests/medium_ref.py: the operator twins and whole paths bit for bit on both engines, Beer-Lambert attenuation, the white furnace,
both engines on a scene with every kind of surface, the estimators against each other, unsetting, errors, the command line.
Every test here needs nori_hip_set_medium, which the commit before this feature does not have."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nori_amd import NoriError, _capi, host
from nori_amd.render import DeviceGroup, Renderer
from nori_amd.scene import Bsdf, Camera, Integrator, Medium, Mesh, RFilter, Scene
from tests import lens_ref as lr, medium_ref as mr, scenes, stat_harness as sh

pytestmark = pytest.mark.gpu

F = np.float32
ENGINES = ("megakernel", "wavefront")
PATHS = ("path_mats", "path_ems", "path_mis")
KEYS = ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid")
W, H = 24, 17
FOG = Medium(0.4, (0.9, 0.6, 0.3), 0.6)


def quad(v, albedo, radiance=None, name=""):
    return Mesh(np.array(v, F), np.array([(0, 1, 2), (0, 2, 3)], np.uint32), bsdf=Bsdf("diffuse", albedo), radiance=radiance, name=name)


def lit_floor_scene(integrator="path_mis", medium=FOG, spp=1):
    """a diffuse floor and, above it, an emitter quad of two unequal triangles that faces down; seen from above at a slant, so the
    top rows look past the floor into the fog"""
    s = 6.0
    floor = quad([(-s, 0, -s), (-s, 0, s), (s, 0, s), (s, 0, -s)], (0.7, 0.45, 0.2), name="floor")
    light = quad([(-1, 3, -1), (1.5, 3, -1), (1, 3, 1.2), (-1, 3, 0.8)], (0.5, 0.5, 0.5), (6.0, 5.0, 4.0), "light")
    cam = Camera(W, H, 50.0, to_world=scenes.lookat((0.3, 2.0, 4.0), (0.0, 0.0, -1.5), (0.0, 1.0, 0.0)))
    return Scene([floor, light], cam, RFilter("box"), Integrator(integrator), spp, medium=medium)


def directions(n=400, seed=2):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], F)
    return np.concatenate([axes, d])


# ------------------------------------------------------------------ 1. the twins, bit for bit
@pytest.mark.parametrize("g", [0.0, 1e-3, 0.6, -0.99])
def test_twins_bit_for_bit(renderer_factory, g):
    med = Medium(0.4, (0.9, 0.6, 0.3), g)
    ref = mr.Medium(med.sigma_t, med.albedo, med.g)
    r = renderer_factory(lit_floor_scene(medium=med))
    log, exp, sincos = mr.device_functions(r)
    got = r.medium
    assert got is not None and F(got.g) == ref.g and F(got.sigma_t) == ref.sigma_t and got.albedo == tuple(float(x) for x in ref.albedo)
    rng = np.random.default_rng(9)
    xi = np.concatenate([np.array([0.0, 1.0 - 2.0 ** -24, 2.0 ** -23, 0.5], F), rng.random(2000, dtype=F)])
    s = r.medium_distance(xi)
    assert s.tobytes() == mr.distance(ref, xi, log).tobytes(), int((s != mr.distance(ref, xi, log)).sum())
    assert s[0] == 0 and not np.signbit(s[0]) and np.isfinite(s).all() and (s >= 0).all()
    dist = np.concatenate([np.array([0.0, 1e-4, 1e3, 1e9], F), s, rng.uniform(0, 30, 500).astype(F)])
    tr = r.medium_transmittance(dist)
    assert tr.tobytes() == mr.transmittance(ref, dist, exp).tobytes()
    assert tr[0] == 1 and (tr <= 1).all() and (tr >= 0).all()
    d = directions()
    n = d.shape[0]
    xs = rng.random((n, 2), dtype=F)
    xs[:8] = [(0, 0), (1 - 2.0 ** -24, 0), (0, 1 - 2.0 ** -24), (1 - 2.0 ** -24, 1 - 2.0 ** -24), (0.5, 0.25), (0.5, 0.5), (0.5, 0.75), (2.0 ** -23, 0.5)]
    wo, pdf = r.phase_sample(d, xs)
    wwo, wpdf = mr.hg_sample(ref, d, xs, sincos)
    assert wo.tobytes() == wwo.tobytes(), int((wo != wwo).any(axis=1).sum())
    assert pdf.tobytes() == wpdf.tobytes(), int((pdf != wpdf).sum())
    assert np.isfinite(wo).all() and np.isfinite(pdf).all() and (pdf > 0).all()
    assert np.abs(np.linalg.norm(wo.astype(np.float64), axis=1) - 1).max() < 1e-5
    # what phase_sample returns for a direction is what phase_eval says of it, byte for byte
    assert r.phase_eval(d, wo).tobytes() == pdf.tobytes()
    other = np.roll(d, 7, axis=0)
    pe = r.phase_eval(d, other)
    assert pe.tobytes() == mr.hg_eval(ref, mr.dot(d, other)).tobytes()
    if ref.g == 0:
        assert (pe == mr.KINVFOURPI).all()


# ------------------------------------------------------------------ 2. whole paths, restated
# Russian roulette renormalises the throughput, so a path survives a vertex with the probability of the largest albedo component
# at most: 0.9 here (the medium's; the surfaces' are below it).  The walker's default cap of 64 vertices would be exceeded by
# 0.9^61 = 0.16 % of the paths that stay in the fog -- about 8 of the 4896 paths below.  At 200 vertices it is 0.9^197 = 1e-9.
CAP = 200


@pytest.mark.parametrize("g", [0.6, 0.0])
def test_restated_paths_bit_for_bit(renderer_factory, g):
    med = Medium(FOG.sigma_t, FOG.albedo, g)
    ref = mr.Medium(med.sigma_t, med.albedo, med.g)
    renderers = {i: renderer_factory(lit_floor_scene(i, med)) for i in PATHS}
    r0 = renderers["path_mis"]
    log, exp, sincos = mr.device_functions(r0)
    idx = np.arange(W * H, dtype=np.uint64)
    for s in (0, 3):
        f = r0.pcg32_floats(idx, np.full(idx.shape, s, np.uint64), 4 + CAP * mr.DRAWS_PER_VERTEX)
        ps, _ = lr.camera_samples(W, H, s, r0.pcg32_floats)
        rays = r0.sample_rays(ps)
        for integrator in PATHS:
            r = renderers[integrator]
            sc = r.scene
            want, nc, ns = mr.walk(r, sc, ref, integrator, rays, f[:, 4:], log, exp, sincos, max_vertices=CAP)
            assert np.isfinite(want).all() and (want > 0).any() and nc > W * H
            assert (ns > 0) == (integrator != "path_mats")
            # Li of the stated rays, its stream seeded like the render's and drawn from the start
            want_li, _, _ = mr.walk(r, sc, ref, integrator, rays, f, log, exp, sincos, max_vertices=CAP)
            got_li = r.li(rays, idx, np.full(idx.shape, s, np.uint64))
            assert got_li.tobytes() == want_li.tobytes(), (integrator, s, int((got_li != want_li).any(axis=1).sum()))
            for engine in ENGINES:
                r.set_option("engine", engine)
                frame, st = r.render_host(spp_count=1, spp_begin=s)
                assert st["engine"] == ENGINES.index(engine) and st["n_invalid"] == 0 and st["n_camera_samples"] == W * H
                assert frame.shape == (H, W, 4) and (frame[..., 3] == 1).all()
                got = frame[..., :3].reshape(-1, 3)
                assert got.tobytes() == want.tobytes(), (integrator, engine, s, g, int((got != want).any(axis=1).sum()))
                assert (st["n_closest_rays"], st["n_shadow_rays"]) == (nc, ns), (integrator, engine, s)
                if engine == "wavefront":
                    assert st["wf_record"] == "full"      # a medium: the one general variant, on the full record


# ------------------------------------------------------------------ 3. Beer-Lambert
def test_absorbing_fog_attenuates_an_emitter_by_the_transmittance(renderer_factory):
    rad = np.array([3.0, 2.0, 1.0], F)
    wall = quad([(-40, -40, -3), (40, -40, -3), (40, 40, -3), (-40, 40, -3)], (0.0, 0.0, 0.0), tuple(float(x) for x in rad), "wall")      # faces +z
    cam = Camera(W, H, 50.0, to_world=scenes.lookat((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)))
    med = Medium(0.5, (0.0, 0.0, 0.0), 0.6)
    sc = Scene([wall], cam, RFilter("box"), Integrator("path_mats"), 256, medium=med)
    r = renderer_factory(sc)
    _, exp, _ = mr.device_functions(r)
    yy, xx = np.mgrid[0:H, 0:W]
    centres = np.stack([xx.ravel() + 0.5, yy.ravel() + 0.5], -1).astype(F)
    its = r.intersect(r.sample_rays(centres))
    assert (its["mesh"] == 0).all()
    tr = mr.transmittance(mr.Medium(med.sigma_t, med.albedo, med.g), its["t"], exp).astype(np.float64)
    assert 0.1 < tr.min() < tr.max() < 0.3
    for engine in ENGINES:
        r.set_option("engine", engine)
        frame, st = r.render_host()
        assert st["n_invalid"] == 0 and st["n_closest_rays"] == st["n_camera_samples"] == W * H * 256 and st["n_shadow_rays"] == 0
        assert (frame[..., 3] == 256).all()
        mean = (frame[..., :3] / frame[..., 3:]).reshape(-1, 3).astype(np.float64)
        for c in range(3):
            ok, info = sh.students_t_test(mean[:, c] / (rad[c] * tr) - 1.0, 0.0, 0.01, 6)
            print(engine, c, info)
            assert ok, (engine, c, info)


# ------------------------------------------------------------------ 4. the white furnace
def furnace_scene(integrator, spp=64, size=32, half=0.2):
    """a closed cube of 12 inward-facing triangles, every one an emitter of radiance 1 and diffuse albedo 0.5, the camera inside,
    filled with a medium that absorbs nothing: the uniform radiance 1 / (1 - 0.5) = 2 solves the surface balance L = 1 + 0.5 L and
    the transport equation alike, whatever the cube's size.

    The size is chosen for path_ems.  Its emitter sample at a medium vertex is a point-to-area sample, cosY / dist^2 over a constant
    density, and a vertex can lie anywhere in the volume: near a wall the second moment behaves like int r^-4 r^2 dr and diverges.
    Every wall emits here, so path_ems's pixel variance is carried by rare vertices next to a wall, and the number of medium vertices
    per path grows with the optical thickness sigma_t * edge.  Measured on an MI355X, 64 spp, mean / variance of the pixel luminance
    (path_mats, path_ems, path_mis): half edge 1.5: 1.9985 / 0.026, 1.9552 / 5.77, 2.0079 / 0.028; 0.75: 1.9963 / 0.017,
    1.9656 / 2.09, 2.0018 / 0.017; 0.4: 1.9989 / 0.011, 2.1234 / 7.61, 1.9986 / 0.012; 0.2: 1.9994 / 0.0065, 2.0109 / 0.67,
    2.0001 / 0.0074.  path_mats and path_mis are within 0.4 % at every size; path_ems's mean of 1024 pixels has a standard error
    of 3.7 % at half edge 1.5 and 1.3 % at 0.2, where a third of the free flights still end in the medium (1 - exp(-0.4))."""
    a = 1.5
    v = np.array([(x, y, z) for x in (-a, a) for y in (-a, a) for z in (-a, a)], F)
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = []
    for q in faces:
        for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
            n = np.cross(v[t[1]] - v[t[0]], v[t[2]] - v[t[0]])
            tris.append(t if np.dot(n, v[list(t)].mean(axis=0)) < 0 else (t[0], t[2], t[1]))      # the normal points at the centre
    scale = F(half / a)
    cube = Mesh(v * scale, np.array(tris, np.uint32), bsdf=Bsdf("diffuse", (0.5, 0.5, 0.5)), radiance=(1.0, 1.0, 1.0), name="cube")
    to_world = scenes.lookat((0.2, 0.1, 0.3), (0.0, -0.3, -1.0), (0.0, 1.0, 0.0)).copy()
    to_world[:3, 3] *= scale
    cam = Camera(size, size, 70.0, to_world=to_world)
    return Scene([cube], cam, RFilter("box"), Integrator(integrator), spp, medium=Medium(1.0, (1.0, 1.0, 1.0), 0.6))


@pytest.mark.parametrize("integrator", PATHS)
def test_white_furnace(renderer_factory, integrator):
    r = renderer_factory(furnace_scene(integrator))
    frame, st = r.render_host()
    assert st["n_invalid"] == 0 and (frame[..., 3] == 64).all()
    lum = sh.luminance((frame[..., :3] / frame[..., 3:]).reshape(-1, 3))
    ok, info = sh.students_t_test(lum, 2.0, 0.01, 3)
    print(integrator, info)
    assert ok, info
    assert abs(info["mean"] / 2.0 - 1) < 0.02


# ------------------------------------------------------------------ 5. both engines, every kind of surface
def fog_box(integrator="path_mis", spp=4, medium=True):
    """test_gpu_envmap.box_scene's box without the environment -- a mirror and a glass sphere, an image texture on the back wall --
    in a fog whose mean free path is the box's size"""
    from tests.test_gpu_envmap import box_scene
    sc = box_scene(integrator, spp, env=False)
    if medium:
        pts = np.concatenate([m.positions for m in sc.meshes])
        extent = float((pts.max(axis=0) - pts.min(axis=0)).max())
        sc.medium = Medium(1.0 / extent, (0.9, 0.8, 0.7), 0.6)
    return sc


@pytest.mark.parametrize("integrator", PATHS)
def test_both_engines_trace_the_same_bits(renderer_factory, integrator):
    r = renderer_factory(fog_box(integrator))
    frames, stats = {}, {}
    for engine in ENGINES:
        r.set_option("engine", engine)
        frames[engine], stats[engine] = r.render_host()
        assert stats[engine]["engine"] == ENGINES.index(engine) and stats[engine]["n_invalid"] == 0
    assert [stats["megakernel"][k] for k in KEYS] == [stats["wavefront"][k] for k in KEYS]
    assert frames["megakernel"].tobytes() == frames["wavefront"].tobytes()
    r.set_option("wavefront_paths", 1024)      # a quarter of the frame's samples: regeneration, many passes, wf_finish
    small, st = r.render_host()
    assert small.tobytes() == frames["wavefront"].tobytes() and [st[k] for k in KEYS] == [stats["wavefront"][k] for k in KEYS]
    r.set_medium(None)
    clear, _ = r.render_host()
    assert clear.tobytes() != small.tobytes()


# ------------------------------------------------------------------ 6. the estimators agree
def test_estimators_agree_on_the_box(renderer_factory):
    """per-pixel means of 64 samples from the three estimators, pairwise: the pixels' differences have mean zero (Student's t over
    the 1024 pixels, the harness's test at its alpha, three comparisons)"""
    lum = {}
    for k, integrator in enumerate(PATHS):
        r = renderer_factory(fog_box(integrator, spp=64))
        frame, st = r.render_host(spp_begin=64 * k)
        assert st["n_invalid"] == 0
        assert (frame[..., 3] == 64).all()
        lum[integrator] = sh.luminance((frame[..., :3] / frame[..., 3:]).reshape(-1, 3))
    for a, b in (("path_mats", "path_ems"), ("path_mats", "path_mis"), ("path_ems", "path_mis")):
        ok, info = sh.students_t_test(lum[a] - lum[b], 0.0, 0.01, 3)
        print(a, b, info)
        assert ok, (a, b, info)
    assert lum["path_mis"].mean() > 0.05


# ------------------------------------------------------------------ 7. unset is unset
@pytest.mark.parametrize("builder", [0, 2])
def test_unset_renders_the_bytes_of_a_context_that_never_had_one(renderer_factory, builder):
    sc = fog_box("path_mis", medium=False)
    med = fog_box().medium
    never = renderer_factory(sc, builder=builder)
    r = renderer_factory(sc, builder=builder)
    for engine in ENGINES:
        never.set_option("engine", engine); r.set_option("engine", engine)
        A, sa = never.render_host()
        r.set_medium(med)
        assert r.medium == Medium(float(F(med.sigma_t)), tuple(float(F(x)) for x in med.albedo), float(F(med.g)))
        B, sb = r.render_host()
        r.set_medium(None)
        assert r.medium is None
        C_, sc_ = r.render_host()
        assert A.tobytes() == C_.tobytes() and [sa[k] for k in KEYS] == [sc_[k] for k in KEYS], (engine, builder)
        assert B.tobytes() != A.tobytes() and sa["engine"] == sb["engine"] == ENGINES.index(engine)
    # an upload resets it, as it resets the lens
    r.set_medium(med)
    r.upload(sc, builder=builder)
    assert r.medium is None


def test_derived_renders_take_a_medium_and_leave_their_bytes_alone(renderer_factory):
    sc = fog_box("path_mis", medium=False)
    med = fog_box().medium
    never, r = renderer_factory(sc), renderer_factory(sc)

    def derived(x):
        f, m2, _ = x.render_moments_host()
        tf, tm2, _ = x.render_tiles_host([0, 3])
        af, am2, aerr, aspp, _, _ = x.render_adaptive_host(0.05, pass_spp=2, spp_count=4)
        feats, _ = x.render_features_host()
        return {"moments": f.tobytes() + m2.tobytes(), "tiles": tf.tobytes() + tm2.tobytes(), "adaptive": af.tobytes() + am2.tobytes() + aspp.tobytes(),
                "features": b"".join(feats[k].tobytes() for k in ("albedo", "normal", "depth"))}

    base = derived(never)
    r.set_medium(med)
    fog = derived(r)
    assert fog["features"] == base["features"]                         # the feature pass is unchanged: the first SURFACE
    assert all(fog[k] != base[k] for k in ("moments", "tiles", "adaptive"))
    r.set_medium(None)
    assert derived(r) == base


# ------------------------------------------------------------------ 8. errors
def test_errors(renderer_factory):
    from nori_amd.scene import Environment
    from tests import envmap_ref as er
    fresh = Renderer(0)
    try:
        with pytest.raises(NoriError, match="NOT_READY.*no scene uploaded"):
            fresh.set_medium(FOG)
    finally:
        fresh.close()
    r = renderer_factory(lit_floor_scene(medium=None))
    for call, word in ((lambda: r.medium_distance([0.5]), "medium_distance: no medium set"), (lambda: r.medium_transmittance([0.5]), "medium_transmittance: no medium set"),
                       (lambda: r.phase_eval(np.eye(3), np.eye(3)), "phase_eval: no medium set"), (lambda: r.phase_sample(np.eye(3), np.zeros((3, 2))), "phase_sample: no medium set")):
        with pytest.raises(NoriError, match="NOT_READY.*" + word):
            call()
    lib = r._lib
    bad = [((np.nan, (1, 1, 1), 0), "sigma_t"), ((np.inf, (1, 1, 1), 0), "sigma_t"), ((0.99e-4, (1, 1, 1), 0), "sigma_t"), ((1.01e4, (1, 1, 1), 0), "sigma_t"),
           ((-1.0, (1, 1, 1), 0), "sigma_t"), ((1.0, (1, -0.1, 1), 0), "albedo"), ((1.0, (1, 1, 1.001), 0), "albedo"), ((1.0, (np.nan, 1, 1), 0), "albedo"),
           ((1.0, (1, 1, 1), 0.995), "asymmetry g"), ((1.0, (1, 1, 1), -1.0), "asymmetry g"), ((1.0, (1, 1, 1), np.nan), "asymmetry g")]
    for state in (None, FOG):      # a failed call leaves the context as it was: without a medium, and with one
        r.set_medium(state)
        before, m0 = r.render_host()[0], r.medium
        for (sig, alb, g), word in bad:
            d = Medium(sig, alb, g).desc()
            rc = lib.nori_hip_set_medium(r._h, C.byref(d))
            msg = lib.nori_hip_last_error(r._h).decode()
            assert rc == -1 and word in msg, (sig, alb, g, rc, msg)
            assert r.medium == m0 and (m0 is None) == (state is None)
        after, _ = r.render_host()
        assert before.tobytes() == after.tobytes()
    # the edges of the ranges are inside
    for sig, g in ((1e-4, 0.99), (1e4, -0.99)):
        r.set_medium(Medium(sig, (0.0, 1.0, 0.5), g))
    # NORI_SEED_NORI_BLOCK
    r.set_medium(FOG)
    with pytest.raises(NoriError, match="UNSUPPORTED.*NORI_SEED_NORI_BLOCK"):
        r.render_host(seed_mode=_capi.SEED_NORI_BLOCK)
    # an environment and a medium exclude each other, whichever comes first
    env = Environment(er.make_map(7), (1.0, 1.0, 1.0), er.rotation())
    with pytest.raises(NoriError, match="UNSUPPORTED.*set_environment.*medium"):
        r.set_environment(env)
    assert r.environment_size == 0 and r.medium is not None
    r.set_medium(None)
    r.set_environment(env)
    with pytest.raises(NoriError, match="UNSUPPORTED.*set_medium.*environment"):
        r.set_medium(FOG)
    assert r.environment_size == 7 and r.medium is None
    # every other integrator
    for integrator in ("normals", "ao", "simple", "whitted"):
        sc = lit_floor_scene(integrator, medium=None)
        sc.integrator.position, sc.integrator.energy = (0.0, 3.0, 0.0), (50.0, 50.0, 50.0)
        q = renderer_factory(sc)
        A, _ = q.render_host()
        with pytest.raises(NoriError, match="UNSUPPORTED.*path_mats, path_ems and path_mis"):
            q.set_medium(FOG)
        assert q.medium is None
        B, _ = q.render_host()
        assert A.tobytes() == B.tobytes(), integrator


def test_the_group_sets_and_renders_a_medium(renderer_factory):
    sc = fog_box("path_mis")
    one, _ = renderer_factory(sc).render_host()
    g = DeviceGroup([0])
    try:
        g.upload(sc)
        frame, _, _ = g.render_host()
        assert frame.tobytes() == one.tobytes()
        g.set_medium(None)
        clear, _, _ = g.render_host()
        assert clear.tobytes() != one.tobytes()
        with pytest.raises(NoriError, match="sigma_t"):
            g.set_medium(Medium(0.0))
    finally:
        g.close()


def test_a_group_of_two_devices_renders_the_medium(renderer_factory):
    try:
        g = DeviceGroup([0, 1])
    except NoriError as e:
        if "device 1 not found" not in str(e):
            raise
        pytest.skip("needs two devices")
    sc = fog_box("path_mis")
    one, _ = renderer_factory(sc).render_host()
    try:
        g.upload(sc)
        frame, _, _ = g.render_host()
        np.testing.assert_allclose(frame, one, rtol=2e-5, atol=1e-6)
    finally:
        g.close()


# ------------------------------------------------------------------ 9. the command line
@pytest.mark.parametrize("engine", ENGINES)
def test_cli_renders_a_scene_with_a_medium(tmp_path, engine):
    from tests.test_medium_cpu import write_scene
    from nori_amd.render import develop_host
    path = write_scene(tmp_path, "fog.xml")
    env = dict(os.environ, NORI_HIP_ENGINE=engine)
    p = subprocess.run([os.path.join(_capi.LIB_DIR, "nori"), path], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = host.load_exr(str(tmp_path / "fog.exr"))
    assert out.shape == (17, 24, 3) and np.isfinite(out).all() and out.mean() > 0.01
    sc = host.HostRoot(path).scene()
    assert sc.medium is not None and F(sc.medium.g) == F(0.6)
    with Renderer(0) as r:
        r.upload(sc, builder=2)
        r.set_option("engine", engine)
        frame, st = r.render_host()
        assert st["n_invalid"] == 0 and st["engine"] == ENGINES.index(engine)
        assert np.allclose(develop_host(frame, r.border), out, rtol=1e-5, atol=1e-6)
        r.set_medium(None)
        clear, _ = r.render_host()
        assert clear.tobytes() != frame.tobytes()
