"""The environment-map emitter on the GPU (include/nori_hip.h, "Environment-map emitter") against the numpy restatement of
tests/envmap_ref.py: tables, lookup and sampling bit for bit, the sampler's distribution, a one-bounce scene restated as a whole,
both engines on a scene with every kind of surface, the estimators against each other, unsetting, errors, the command line."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from nori_amd import NoriError, _capi, host
from nori_amd.render import DeviceGroup
from nori_amd.scene import Bsdf, Camera, Environment, Integrator, Mesh, RFilter, Scene, Texture
from tests import envmap_ref as er, film_cases, lens_ref as lr, scenes, stat_harness as sh

pytestmark = pytest.mark.gpu

ENGINES = ("megakernel", "wavefront")
PATHS = ("path_mats", "path_ems", "path_mis")
KEYS = ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid")
W, H = 24, 17
ALBEDO = (0.7, 0.45, 0.2)
KINVPI = np.float32(0.31830988618379067154)


def floor_scene(integrator="path_mis", env=None, spp=1, size=6.0, width=W, height=H):
    """one diffuse quad facing up, seen from above at a slant: the pixels of the top rows look past it"""
    q = quad_mesh(size, ALBEDO)
    cam = Camera(width, height, 50.0, to_world=scenes.lookat((0.3, 2.0, 4.0), (0.0, 0.0, -1.5), (0.0, 1.0, 0.0)))
    return Scene([q], cam, RFilter("box"), Integrator(integrator), spp, environment=env)


def quad_mesh(size, albedo):
    s = float(size)
    v = np.array([(-s, 0, -s), (-s, 0, s), (s, 0, s), (s, 0, -s)], np.float32)
    return Mesh(v, np.array([(0, 1, 2), (0, 2, 3)], np.uint32), bsdf=Bsdf("diffuse", albedo), name="floor")


def environment(n, kind="random"):
    return Environment(er.make_map(n, kind), (0.5, 1.25, 2.0), er.rotation())


def ref_of(env: Environment):
    return er.EnvRef(env.texels, env.scale, env.to_world)


# ------------------------------------------------------------------ 1. tables, eval and sample, bit for bit
@pytest.mark.parametrize("n, kind", [(1, "random"), (2, "random"), (7, "zeros"), (7, "range"), (64, "random"), (64, "zeros")])
def test_tables_eval_and_sample_bit_for_bit(renderer_factory, n, kind):
    env = environment(n, kind)
    ref = ref_of(env)
    r = renderer_factory(floor_scene(env=env))
    assert r.environment_size == n
    rows, cols, weight = r.env_tables()
    assert weight.tobytes() == ref.weight.tobytes(), int((weight != ref.weight).sum())
    assert cols.tobytes() == ref.col_cdf.tobytes(), int((cols != ref.col_cdf).sum())
    assert rows.tobytes() == ref.row_cdf.tobytes(), int((rows != ref.row_cdf).sum())
    # directions: random, the six axes, the seams z = 0, x = 0, y = 0 of the map's own frame
    d = (er.directions().astype(np.float64) @ ref.m.astype(np.float64).T).astype(np.float32)
    d = np.concatenate([d, er.directions(500, seed=4)])
    le, pdf = r.env_eval(d)
    wle, wpdf, _ = ref.eval(d)
    assert le.tobytes() == wle.tobytes(), int((le != wle).any(axis=1).sum())
    assert pdf.tobytes() == wpdf.tobytes(), int((pdf != wpdf).sum())
    assert r.env_eval(d, pdf=False).tobytes() == wle.tobytes()
    # samples: random, 0, 1 - 2^-24, every CDF boundary value and its float neighbours
    xi = er.samples(ref)
    sd, sle, spdf = r.env_sample(xi)
    wd, wle, wpdf, _ = ref.sample(xi)
    assert sd.tobytes() == wd.tobytes(), int((sd != wd).any(axis=1).sum())
    assert sle.tobytes() == wle.tobytes() and spdf.tobytes() == wpdf.tobytes(), int((spdf != wpdf).sum())
    assert np.isfinite(sd).all() and np.isfinite(spdf).all() and np.abs(np.linalg.norm(sd.astype(np.float64), axis=1) - 1).max() < 1e-6
    # what env_sample returns for a direction is what env_eval says of it, byte for byte
    ele, epdf = r.env_eval(sd)
    assert ele.tobytes() == sle.tobytes() and epdf.tobytes() == spdf.tobytes()
    # the same map gives the same tables
    r.set_environment(env)
    again = r.env_tables()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (rows, cols, weight)))


# ------------------------------------------------------------------ 2. the sampler's distribution
def test_sampled_directions_follow_the_texel_probabilities(renderer_factory):
    n, count = 8, 100000
    env = Environment(er.make_map(n, "contrast"), (1.0, 1.0, 1.0), er.rotation(2))
    ref = ref_of(env)
    r = renderer_factory(floor_scene(env=env))
    xi = np.random.default_rng(12).random((count, 2), dtype=np.float32)
    d, _, _ = r.env_sample(xi)
    _, _, (i, j) = ref.eval(d)
    obs = np.bincount(j * n + i, minlength=n * n).astype(np.float64)
    p = (np.diff(ref.row_cdf.astype(np.float64))[:, None] * np.diff(ref.col_cdf.astype(np.float64), axis=1)).ravel()
    assert abs(p.sum() - 1) < 1e-5 and p.max() / p[p > 0].min() > 1000      # strong contrast
    ok, info = sh.chi2_test(obs, p * count, count, 5, 0.01, 1)
    assert ok, info


# ------------------------------------------------------------------ 3. a one-bounce scene, restated
def restated_li(r, sc, ref, integrator, rays, floats):
    """Li of the rays of floor_scene with the environment `ref`: the stated path (rt_path.h; include/nori_hip.h "In Li"), float32.
    floats[k]: the numbers path k draws, in order.  The second ray starts on the floor and points up: it always escapes."""
    n = rays.shape[0]
    its = r.intersect(rays)
    hit = its["mesh"] != _capi.NO_HIT
    L = np.zeros((n, 3), np.float32)
    le0, _, _ = ref.eval(rays["d"])
    L[~hit] = le0[~hit]                                   # a camera ray that leaves the scene: T = 1, wMat = 1
    a = np.asarray(sc.meshes[0].bsdf.albedo, np.float32)
    s, t, nn = its["sh_s"], its["sh_t"], its["sh_n"]
    dot = lambda u, v: u[:, 0] * v[:, 0] + (u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2])
    assert (dot(-rays["d"], nn)[hit] > 0).all()           # seen from above: wi.z > 0
    ems = integrator != "path_mats"
    Lh = np.zeros((n, 3), np.float32)
    if ems:                                               # four numbers: xiE, xiT (unused), xi
        assert ((floats[:, 0] * np.float32(1.0)).astype(np.uint32) == 0).all()      # one light: the environment
        dirs, le, pdfw, _ = ref.sample(floats[:, 2:4])
        woz = dot(dirs, nn)
        lit = hit & (pdfw > 0) & (woz > 0)
        pdf_em = pdfw * np.float32(1.0)                   # pdfPick = 1 / 1
        with np.errstate(divide="ignore", invalid="ignore"):
            ld = ((a * KINVPI)[None, :] * le) * (woz / pdf_em)[:, None]
            if integrator == "path_mis":
                pdf_bsdf = KINVPI * woz
                ld = ld * (pdf_em / (pdf_em + pdf_bsdf))[:, None]
        # st.Ld = T * Ld * w with T = 1 (and w = 1 for path_ems); the shadow ray leaves the scene: L = 0 + Ld
        Lh[lit] = ld[lit]
    xi_b = floats[:, 4:6] if ems else floats[:, 0:2]
    wo = r.warp("cosine_hemisphere", xi_b)
    cont = (s * wo[:, 0:1] + t * wo[:, 1:2]) + nn * wo[:, 2:3]
    le2, pdf2, _ = ref.eval(cont)
    if integrator == "path_mats":
        Lh = Lh + (a[None, :] * le2) * np.float32(1.0)
    elif integrator == "path_mis":
        pdf_mat = KINVPI * wo[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(pdf_mat + pdf2 > 0, pdf_mat / (pdf_mat + pdf2), np.float32(0)).astype(np.float32)
        Lh = np.where((w > 0)[:, None], Lh + (a[None, :] * le2) * w[:, None], Lh)
    L[hit] = Lh[hit]
    return L.astype(np.float32), hit


@pytest.mark.parametrize("integrator", PATHS)
def test_one_bounce_scene_bit_for_bit(renderer_factory, integrator):
    env = environment(7, "zeros")
    ref = ref_of(env)
    sc = floor_scene(integrator, env)
    r = renderer_factory(sc)
    for s in (0, 3):
        idx = np.arange(W * H, dtype=np.uint64)
        f = r.pcg32_floats(idx, np.full(idx.shape, s, np.uint64), 10)
        ps, _ = lr.camera_samples(W, H, s, r.pcg32_floats)
        rays = r.sample_rays(ps)
        want, hit = restated_li(r, sc, ref, integrator, rays, f[:, 4:])
        assert 0.5 < hit.mean() < 0.95 and (want[~hit] > 0).any() and (want[hit] > 0).any()
        # Li of the stated rays, its stream seeded like the render's and drawn from the start
        want_li, _ = restated_li(r, sc, ref, integrator, rays, f)
        got_li = r.li(rays, idx, np.full(idx.shape, s, np.uint64))
        assert got_li.tobytes() == want_li.tobytes(), (integrator, s, int((got_li != want_li).any(axis=1).sum()))
        for engine in ENGINES:
            r.set_option("engine", engine)
            frame, st = r.render_host(spp_count=1, spp_begin=s)
            assert st["engine"] == ENGINES.index(engine) and st["n_invalid"] == 0 and st["n_camera_samples"] == W * H
            assert frame.shape == (H, W, 4) and (frame[..., 3] == 1).all()
            got = frame[..., :3].reshape(-1, 3)
            assert got.tobytes() == want.tobytes(), (integrator, engine, s, int((got != want).any(axis=1).sum()))
            assert st["n_closest_rays"] == W * H + int(hit.sum())
            if engine == "wavefront":
                assert st["wf_record"] == "full"      # an environment: the one general variant, on the full record


def test_constant_map_under_path_mats_is_albedo_times_the_constant(renderer_factory):
    c = np.array([0.8, 1.5, 0.3], np.float32)
    env = Environment(np.broadcast_to(c, (7, 7, 3)).copy(), (1.0, 1.0, 1.0), er.rotation())
    r = renderer_factory(floor_scene("path_mats", env))
    ps, _ = lr.camera_samples(W, H, 0, r.pcg32_floats)
    hit = (r.intersect(r.sample_rays(ps))["mesh"] != _capi.NO_HIT).reshape(H, W)
    for engine in ENGINES:
        r.set_option("engine", engine)
        frame, _ = r.render_host(spp_count=1)
        assert np.array_equal(frame[hit][:, :3], np.broadcast_to(np.asarray(ALBEDO, np.float32) * c, (int(hit.sum()), 3)))
        assert np.array_equal(frame[~hit][:, :3], np.broadcast_to(c, (int((~hit).sum()), 3)))


# ------------------------------------------------------------------ 4. both engines, every kind of surface
def box_scene(integrator="path_mis", spp=4, env=True, size=32):
    """the Cornell box (open towards the camera, an area light under its ceiling) with a mirror and a glass sphere, an image
    texture on the back wall, and an environment that shines in through the opening"""
    sc = film_cases.cornell(size, size, spp, RFilter("box"), integrator=integrator)
    sc.textures = [Texture("image", np.random.default_rng(11).uniform(0.05, 0.95, (7, 9, 3)).astype(np.float32), "bilinear", "repeat", 4.0, 4.0)]
    {m.name: m for m in sc.meshes}["back"].albedo_texture = 0
    assert {m.bsdf.type for m in sc.meshes} >= {"diffuse", "mirror", "dielectric"} and any(m.radiance is not None for m in sc.meshes)
    if env:
        sc.environment = Environment(er.make_map(16, "contrast"), (2.0, 2.0, 2.5), er.rotation(7))
    return sc


@pytest.mark.parametrize("integrator", PATHS)
def test_both_engines_trace_the_same_bits(renderer_factory, integrator):
    r = renderer_factory(box_scene(integrator))
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
    # and the environment is in the picture: the frame without it is another frame, with fewer shadow rays under path_ems / path_mis
    r.set_environment(None)
    dark, sd = r.render_host()
    assert dark.tobytes() != small.tobytes() and dark[..., :3].sum() < small[..., :3].sum()


# ------------------------------------------------------------------ 5. the estimators agree
def test_estimators_agree_on_the_box(renderer_factory):
    """per-pixel means of 64 samples from the three estimators, pairwise: the pixels' differences have mean zero (Student's t over
    the 1024 pixels, the harness's test at its alpha, three comparisons)"""
    lum = {}
    for k, integrator in enumerate(PATHS):
        r = renderer_factory(box_scene(integrator, spp=64))
        frame, st = r.render_host(spp_begin=64 * k)
        assert st["n_invalid"] == 0
        assert (frame[..., 3] == 64).all()      # the box filter: a pixel's weight is its sample count
        lum[integrator] = sh.luminance((frame[..., :3] / frame[..., 3:]).reshape(-1, 3))
    for a, b in (("path_mats", "path_ems"), ("path_mats", "path_mis"), ("path_ems", "path_mis")):
        ok, info = sh.students_t_test(lum[a] - lum[b], 0.0, 0.01, 3)
        print(a, b, info)
        assert ok, (a, b, info)
    assert lum["path_mis"].mean() > 0.05


@pytest.mark.parametrize("integrator", PATHS)
def test_floor_under_a_constant_sky_has_albedo_times_the_sky(renderer_factory, integrator):
    c = np.array([0.8, 1.5, 0.3], np.float32)
    env = Environment(np.broadcast_to(c, (16, 16, 3)).copy(), (1.0, 1.0, 1.0), er.rotation())
    sc = floor_scene(integrator, env, spp=64, size=500.0, width=32, height=32)
    sc.camera.to_world = scenes.lookat((0.3, 3.0, 0.5), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0))      # straight down: floor in every pixel
    r = renderer_factory(sc)
    frame, st = r.render_host()
    assert st["n_invalid"] == 0 and st["n_closest_rays"] == 2 * st["n_camera_samples"]      # every camera ray hits, every second ray escapes
    want = float(sh.luminance((np.asarray(ALBEDO, np.float32) * c)[None, :])[0])
    assert (frame[..., 3] == 64).all()
    ok, info = sh.students_t_test(sh.luminance((frame[..., :3] / frame[..., 3:]).reshape(-1, 3)), want, 0.01, 3)
    print(integrator, info)
    assert ok, info
    assert abs(info["mean"] / want - 1) < 0.02


# ------------------------------------------------------------------ 6. unset is unset
@pytest.mark.parametrize("builder", [0, 2])
def test_unset_renders_the_bytes_of_a_context_that_never_had_one(renderer_factory, builder):
    sc = box_scene("path_mis", env=False)
    env = box_scene().environment
    never = renderer_factory(sc, builder=builder)
    r = renderer_factory(sc, builder=builder)
    for engine in ENGINES:
        never.set_option("engine", engine); r.set_option("engine", engine)
        A, sa = never.render_host()
        r.set_environment(env)
        assert r.environment_size == 16
        B, sb = r.render_host()
        r.set_environment(None)
        assert r.environment_size == 0
        C, sc_ = r.render_host()
        assert A.tobytes() == C.tobytes() and [sa[k] for k in KEYS] == [sc_[k] for k in KEYS], (engine, builder)
        assert B.tobytes() != A.tobytes() and sa["engine"] == sb["engine"] == ENGINES.index(engine)
    # an upload resets it, as it resets the lens
    r.set_environment(env)
    r.upload(sc, builder=builder)
    assert r.environment_size == 0


def test_derived_renders_take_an_environment_and_leave_their_bytes_alone(renderer_factory):
    sc = box_scene("path_mis", env=False)
    env = box_scene().environment
    never, r = renderer_factory(sc), renderer_factory(sc)

    def derived(x):
        f, m2, _ = x.render_moments_host()
        tf, tm2, _ = x.render_tiles_host([0, 3])
        feats, _ = x.render_features_host()
        den, wsum = x.denoise_host(f, m2, feats["albedo"], feats["normal"], feats["depth"])
        return {"moments": f.tobytes() + m2.tobytes(), "tiles": tf.tobytes() + tm2.tobytes(),
                "features": b"".join(feats[k].tobytes() for k in ("albedo", "normal", "depth")), "denoise": den.tobytes() + wsum.tobytes()}

    base = derived(never)
    r.set_environment(env)
    lit = derived(r)
    assert lit["features"] == base["features"]                         # the feature pass is unchanged: a miss is coverage 0
    assert all(lit[k] != base[k] for k in ("moments", "tiles", "denoise"))
    r.set_environment(None)
    assert derived(r) == base


# ------------------------------------------------------------------ 7. errors
def test_errors_and_the_group(renderer_factory):
    from nori_amd.render import Renderer
    good = environment(7)
    fresh = Renderer(0)
    try:
        with pytest.raises(NoriError, match="NOT_READY.*no scene uploaded"):
            fresh.set_environment(good)
    finally:
        fresh.close()
    r = renderer_factory(floor_scene())
    for call, word in ((lambda: r.env_eval(np.eye(3)), "env_eval: no environment set"), (lambda: r.env_sample(np.zeros((1, 2))), "env_sample: no environment set"),
                       (lambda: r.env_tables(), "no environment set")):
        with pytest.raises(NoriError, match="NOT_READY.*" + word):
            call()

    def bad(texels=None, scale=(1, 1, 1), to_world=np.eye(3), size=None):
        e = Environment(good.texels if texels is None else texels, scale, to_world)
        d = e.desc()
        if size is not None:
            d.size = size
        return e, d

    big = np.zeros((2, 2, 3), np.float32)
    cases = [(bad(size=0), "size must be 1 .. 4096"), (bad(size=4097), "size must be 1 .. 4096"),
             (bad(texels=np.where(np.arange(147).reshape(7, 7, 3) == 5, np.nan, 1).astype(np.float32)), "texel 1 is negative or not finite"),
             (bad(texels=np.where(np.arange(147).reshape(7, 7, 3) == 9, -1, 1).astype(np.float32)), "texel 3 is negative or not finite"),
             (bad(texels=np.where(np.arange(147).reshape(7, 7, 3) == 0, np.inf, 1).astype(np.float32)), "texel 0 is negative or not finite"),
             (bad(scale=(1, -1, 1)), "scale must be finite and not negative"), (bad(scale=(1, np.inf, 1)), "scale must be finite and not negative"),
             (bad(texels=big), "luminance is 0 everywhere"), (bad(scale=(0, 0, 0)), "luminance is 0 everywhere"),
             (bad(to_world=np.diag([1, 1, 1.001])), "not a rotation"), (bad(to_world=np.array([[1, 0.01, 0], [0, 1, 0], [0, 0, 1]])), "not a rotation")]
    lib = r._lib
    import ctypes as C
    for (e, d), word in cases:
        rc = lib.nori_hip_set_environment(r._h, C.byref(d))
        assert rc == -1 and word in lib.nori_hip_last_error(r._h).decode(), (word, rc, lib.nori_hip_last_error(r._h).decode())
    d = good.desc(); d.texels = None
    assert lib.nori_hip_set_environment(r._h, C.byref(d)) == -1 and "texels is NULL" in lib.nori_hip_last_error(r._h).decode()
    assert r.environment_size == 0                                  # a refused map leaves the context as it was
    r.set_environment(good)
    rc = lib.nori_hip_set_environment(r._h, C.byref(bad(size=0)[1]))
    assert rc == -1 and r.environment_size == 7
    with pytest.raises(NoriError, match="UNSUPPORTED.*NORI_SEED_NORI_BLOCK"):
        r.render_host(seed_mode=_capi.SEED_NORI_BLOCK)
    w = renderer_factory(floor_scene("whitted"))
    with pytest.raises(NoriError, match="UNSUPPORTED.*whitted"):
        w.set_environment(good)
    # integrators that ignore emitters ignore the environment
    for integrator in ("normals", "ao", "simple"):
        sc = floor_scene(integrator)
        sc.integrator.position, sc.integrator.energy = (0.0, 3.0, 0.0), (50.0, 50.0, 50.0)
        q = renderer_factory(sc)
        A, _ = q.render_host()
        q.set_environment(good)
        B, _ = q.render_host()
        assert A.tobytes() == B.tobytes(), integrator
    # the single-device group renders the context's frame
    sc = box_scene("path_mis")
    one, _ = renderer_factory(sc).render_host()
    g = DeviceGroup([0])
    try:
        g.upload(sc)
        frame, _, _ = g.render_host()
        assert frame.tobytes() == one.tobytes()
        g.set_environment(None)
        dark, _, _ = g.render_host()
        assert dark.tobytes() != one.tobytes()
    finally:
        g.close()


# ------------------------------------------------------------------ 8. the command line
def test_cli_renders_a_scene_with_an_environment(tmp_path):
    from tests.test_envmap_cpu import latlong_image, write_scene
    img, _ = latlong_image()
    host.save_images(str(tmp_path / "sky"), img)
    path = write_scene(tmp_path, "sky_floor.xml", "path_mis", '<integer name="resolution" value="32"/>')
    p = subprocess.run([os.path.join(_capi.LIB_DIR, "nori"), path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = host.load_exr(str(tmp_path / "sky_floor.exr"))
    assert out.shape == (17, 24, 3) and np.isfinite(out).all()
    # the top row looks at the sky just above the horizon, where the image is bluish: (0.2, 0.3, 0.5) and a little more
    top = out[0].mean(axis=0)
    assert top[2] > top[1] > top[0] > 0.15 and out[-1].mean() > 0.05
    # and the library renders the host's description of the scene -- its environment resampled by the host -- to the frame the
    # command line wrote (same library, same default engine and builder)
    from nori_amd.render import Renderer, develop_host
    sc = host.HostRoot(path).scene()
    assert sc.environment is not None and sc.environment.texels.shape == (32, 32, 3)
    with Renderer(0) as r:
        r.upload(sc, builder=2)
        frame, st = r.render_host()
        assert st["n_invalid"] == 0
        assert np.allclose(develop_host(frame, r.border), out, rtol=1e-5, atol=1e-6)
        r.set_environment(None)
        dark, _ = r.render_host()
        assert develop_host(dark, r.border).max() == 0      # nothing else lights this scene
