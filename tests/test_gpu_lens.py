"""The thin-lens camera on the GPU (include/nori_hip.h, "Thin-lens camera") against the numpy restatement of tests/lens_ref.py:
the ray twin bit for bit, the pinhole untouched, every consumer of the camera sample (megakernel, wavefront, feature pass) held
to the stated ray sample by sample, whole frames, the renders built on those kernels, the blur itself, errors, and the
arithmetic's domain.  Frames are 45 x 37 (3 x 3 tiles, neither side a multiple of 16) unless said otherwise."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import NoriError, _capi
from nori_amd.render import DeviceGroup
from nori_amd.scene import RFilter, Scene, Texture
from tests import features_ref as fr, film_cases, lens_cases as lc, lens_ref as lr, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 45, 37
R, F = 0.125, 4.0      # the Cornell box's camera stands 4.2 in front of the box's middle: the spheres are near focus, the walls are not
ENGINES = ("megakernel", "wavefront")


def box_scene(integrator="normals", rf="box", spp=1):
    """the Cornell box with a mirror and a glass (dielectric) sphere, an image texture on the floor and a checkerboard on the back wall"""
    sc = film_cases.cornell(W, H, spp, RFilter(rf), integrator=integrator)
    img = np.random.default_rng(11).uniform(0.05, 0.95, (7, 9, 3)).astype(np.float32)
    sc.textures = [Texture("image", img, "bilinear", "repeat", 4.0, 4.0), Texture("checkerboard", uscale=4.0, vscale=4.0, color0=(0.85, 0.3, 0.2), color1=(0.1, 0.5, 0.75))]
    by_name = {m.name: m for m in sc.meshes}
    by_name["floor"].albedo_texture = 0
    by_name["back"].albedo_texture = 1
    assert any(m.bsdf.type == "dielectric" for m in sc.meshes)
    return sc


_REF = {}


def ref_rays(r, s):
    """(pixelSample, nori_ray records) of camera sample s of every pixel of box_scene with the lens (R, F): the four floats of a pixel
    from the device's sampler twin (nori_hip_pcg32_floats(py * W + px, s, 4)), the rays from lens_ref.  Computed once, read-only."""
    if s not in _REF:
        ps, ap = lr.camera_samples(W, H, s, r.pcg32_floats)
        rays = lr.as_rays(lr.lens_rays(box_scene(), ps, ap, R, F))
        ps.setflags(write=False); rays.setflags(write=False)
        _REF[s] = (ps, rays)
    return _REF[s]


# ------------------------------------------------------------------ 1. the ray twin
def test_ray_twin_bit_for_bit(renderer_factory):
    sc = scenes.cornell_box(W, H, 1, "normals")
    sc.camera.to_world = scenes.lookat((0.7, 1.4, 4.0), (0.1, 0.9, 0.0), (0.1, 1.0, 0.05))      # rotated about all three axes, translated
    r = renderer_factory(sc)
    rng = np.random.default_rng(3)
    n = 50000
    ps = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1).astype(np.float32)
    ap = rng.random((n, 2), dtype=np.float32)
    ap[:6] = [(0, 0), (1, 1), (0, 1), (1, 0), (0, 0.5), (1, 0.25)]      # 0, 1 and the corners of the unit square
    r.set_lens(0.3125, 3.75)
    assert r.lens == (0.3125, 3.75)
    got = r.sample_rays_lens(ps, ap)
    want = lr.as_rays(lr.lens_rays(sc, ps, ap, 0.3125, 3.75))
    for k in ("o", "d", "mint", "maxt"):
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    assert got.tobytes() == want.tobytes()
    assert len(np.unique(got["o"], axis=0)) > n // 2      # the origins do move
    pin = r.sample_rays(ps)                               # the pinhole's twin does not look at the lens
    r.set_lens(0.0, 3.75)
    assert r.sample_rays_lens(ps, ap).tobytes() == pin.tobytes() == r.sample_rays(ps).tobytes()
    # the sampler twin gives the floats the reference samples are made of
    assert np.array_equal(np.concatenate(lr.camera_samples(W, H, 5, r.pcg32_floats), axis=1), np.concatenate(lr.camera_samples(W, H, 5), axis=1))


# ------------------------------------------------------------------ 2. the pinhole is untouched
@pytest.mark.parametrize("builder", [0, 2])
@pytest.mark.parametrize("name", ["pa4-cbox-path_mis", "pa4-cbox-whitted"])
def test_pinhole_frames_keep_their_bits(renderer_factory, name, builder):
    sc = Scene.load_npz(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    sc.camera.width, sc.camera.height, sc.sample_count = 64, 48, 4
    r = renderer_factory(sc, builder=builder)
    keys = ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid")
    for engine in ENGINES:
        r.set_option("engine", engine)
        r.upload(sc, builder=builder)      # (a fresh upload: no lens call has been made on this scene)
        A, sa = r.render_host()
        r.set_lens(0.0, 3.0)
        B, sb = r.render_host()
        r.set_lens(0.2, 3.0)
        C, sc_ = r.render_host()
        r.set_lens(0.0, 3.0)
        D, sd = r.render_host()
        assert sa["engine"] == ENGINES.index(engine)
        assert A.tobytes() == B.tobytes() == D.tobytes(), (name, engine)
        assert [sa[k] for k in keys] == [sb[k] for k in keys] == [sd[k] for k in keys]
        assert C.tobytes() != A.tobytes() and sc_["n_camera_samples"] == sa["n_camera_samples"]


# ------------------------------------------------------------------ 3. every consumer uses the stated ray
@pytest.mark.parametrize("engine", ENGINES)
def test_normals_frames_are_li_of_the_stated_rays(renderer_factory, engine):
    r = renderer_factory(box_scene("normals"))
    r.set_option("engine", engine)
    r.set_lens(R, F)
    for s in (0, 5):
        ps, rays = ref_rays(r, s)
        want = r.li(rays, np.zeros(len(rays), np.uint64), np.zeros(len(rays), np.uint64)).reshape(H, W, 3)
        frame, st = r.render_host(spp_count=1, spp_begin=s)
        assert st["engine"] == ENGINES.index(engine) and st["n_invalid"] == 0
        assert frame.shape == (H, W, 4) and (frame[..., 3] == 1).all()
        assert np.array_equal(frame[..., :3], want), (engine, s, int((frame[..., :3] != want).any(axis=-1).sum()))
    pin, _ = renderer_factory(box_scene("normals")).render_host(spp_count=1, spp_begin=5)
    assert (pin[..., :3] != want).any(axis=-1).mean() > 0.02      # and a lens ray is not the pinhole's


class _StatedRays:
    """what features_ref.sample_values asks of an oracle, answered with the lens rays and the device's intersection twin"""
    def __init__(self, renderer, rays):
        self.r, self.rays = renderer, rays

    def sample_rays(self, ps):
        return self.rays

    def intersect(self, rays):
        return self.r.intersect(rays)


def test_feature_frames_are_the_first_hits_of_the_stated_rays(renderer_factory):
    sc = box_scene("path_mis")
    r = renderer_factory(sc)
    r.set_lens(R, F)
    for s in (0, 5):
        ps, rays = ref_rays(r, s)
        its = r.intersect(rays)
        hit = its["mesh"] != _capi.NO_HIT
        vals = fr.sample_values(sc, ps, _StatedRays(r, rays))
        frames, st = r.render_features_host(spp_count=1, spp_begin=s)
        assert st["n_invalid"] == 0
        t = np.where(hit, its["t"], np.float32(0))
        depth = np.stack([t, (t * t).astype(np.float32), hit.astype(np.float32)], axis=1).reshape(H, W, 3)
        assert np.array_equal(frames["depth"][..., :3], depth), s
        for n in ("albedo", "normal"):
            assert (frames[n][..., 3] == 1).all()
            assert np.array_equal(frames[n][..., :3], vals[n].reshape(H, W, 3)), (n, s)
    assert len(np.unique(vals["albedo"].round(3), axis=0)) > 6      # the textures are in view


@pytest.mark.parametrize("integrator", ["path_mis", "path_mats"])
def test_both_engines_trace_the_same_paths(renderer_factory, integrator):
    r = renderer_factory(box_scene(integrator))
    r.set_lens(R, F)
    pin = None
    for s in (0, 5):
        out = {}
        for engine in ENGINES:
            r.set_option("engine", engine)
            out[engine] = r.render_host(spp_count=1, spp_begin=s)
            assert out[engine][1]["engine"] == ENGINES.index(engine)
        (A, sa), (B, sb) = out["megakernel"], out["wavefront"]
        assert np.array_equal(A, B), (integrator, s, int((A != B).any(axis=-1).sum()))
        for k in ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid"):
            assert sa[k] == sb[k], (k, sa[k], sb[k])
        assert sa["n_closest_rays"] > W * H
    r.set_lens(0.0, F)
    pin, _ = r.render_host(spp_count=1, spp_begin=5)
    assert not np.array_equal(pin, B)


# ------------------------------------------------------------------ 4. whole frames
def test_whole_frames_are_the_splat_of_the_stated_samples(renderer_factory):
    r = renderer_factory(box_scene("normals", "gaussian"))
    r.set_lens(R, F)
    zeros = np.zeros(W * H, np.uint64)
    ps = np.concatenate([ref_rays(r, s)[0] for s in range(16)])
    vals = np.concatenate([r.li(ref_rays(r, s)[1], zeros, zeros) for s in range(16)])
    want = r.splat(ps, vals)
    for engine in ENGINES:
        r.set_option("engine", engine)
        got, st = r.render_host(spp_count=16)
        assert st["engine"] == ENGINES.index(engine) and st["n_invalid"] == 0
        # the tolerances tests/test_gpu_parity.py allows the film's summation order
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5, err_msg=engine)


# ------------------------------------------------------------------ 5. derived renders
def test_derived_renders_inherit_the_lens(renderer_factory):
    r = renderer_factory(box_scene("path_mis", "gaussian"))
    r.set_lens(R, F)
    whole, sw = r.render_host(spp_count=8)
    pin, _ = renderer_factory(box_scene("path_mis", "gaussian")).render_host(spp_count=8)
    assert not np.array_equal(whole, pin)
    rgbw, m2, sm = r.render_moments_host(spp_count=8)
    assert rgbw.tobytes() == whole.tobytes() and m2.any()
    ty, tx = r.tile_grid()
    tiles, _, stt = r.render_tiles_host(np.arange(ty * tx), spp_count=8)
    assert tiles.tobytes() == whole.tobytes()
    assert sm["n_closest_rays"] == stt["n_closest_rays"] == sw["n_closest_rays"]
    shares = sum(r.render_host(spp_count=8, tile_mod=2, tile_rem=k)[0] for k in range(2))
    np.testing.assert_allclose(shares, whole, rtol=1e-4, atol=1e-5)
    full, _ = r.render_features_host(spp_count=8)
    parts = [r.render_features_host(spp_count=8, tile_mod=2, tile_rem=k)[0] for k in range(2)]
    pin_f, _ = renderer_factory(box_scene("path_mis", "gaussian")).render_features_host(spp_count=8)
    for n in fr.NAMES:
        np.testing.assert_allclose(parts[0][n] + parts[1][n], full[n], rtol=1e-4, atol=1e-5, err_msg=n)
        assert not np.array_equal(full[n], pin_f[n]), n


# ------------------------------------------------------------------ 6. depth of field is there
def _edge_counts_of_the_depth_frame(r):
    frames, st = r.render_features_host(features=("depth",), spp_count=lc.SPP)
    d = frames["depth"]
    assert d.shape == (lc.H, lc.W, 4) and st["n_invalid"] == 0
    cover = d[..., 2].sum(axis=0) / d[..., 3].sum(axis=0)            # hits / samples per pixel column (box filter: integers)
    half = lc.W // 2
    dist = [d[:, h, 0].sum() / d[:, h, 2].sum() for h in (slice(0, half), slice(half, lc.W))]      # mean distance of the hits of each half
    far_first = dist[0] > dist[1]
    assert 1.8 < max(dist) / min(dist) < 2.3
    zero = np.zeros(half)
    left, right = np.concatenate([cover[:half], zero]), np.concatenate([zero, cover[half:]])
    near, far = (right, left) if far_first else (left, right)
    assert near.max() == 1 and far.max() == 1
    return lc.edge_counts(near, far)


def test_depth_of_field_is_there(renderer_factory):
    r = renderer_factory(lc.scene())
    n_near, n_far = _edge_counts_of_the_depth_frame(r)
    print(f"pinhole: in-focus edge {n_near} partial columns, far edge {n_far}")
    lc.assert_blur(n_near, n_far, lens=False)
    r.set_lens(lc.R, lc.F)
    n_near, n_far = _edge_counts_of_the_depth_frame(r)
    print(f"lens: in-focus edge {n_near} partial columns, far edge {n_far} (c = {lc.COC_PIXELS:.2f} px)")
    lc.assert_blur(n_near, n_far, lens=True)


# ------------------------------------------------------------------ 7. errors
def test_errors_and_the_reset(renderer_factory):
    sc = box_scene("path_mis")
    from nori_amd.render import Renderer
    empty = Renderer(0)
    with pytest.raises(NoriError, match="NORI_ERR_NOT_READY"):
        empty.set_lens(0.1, 1.0)
    empty.close()
    r = renderer_factory(sc)
    assert r.lens == (0.0, 0.0)
    before, _ = r.render_host(spp_count=2)
    for bad in ((-0.1, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (0.1, 0.0), (0.1, -2.0), (0.1, float("nan")), (0.1, float("inf"))):
        with pytest.raises(NoriError, match="NORI_ERR_INVALID_ARGUMENT"):
            r.set_lens(*bad)
    assert r.lens == (0.0, 0.0)
    r.set_lens(0.0, -1.0)                     # no lens: the focus distance is not looked at
    r.set_lens(R, F)
    with pytest.raises(NoriError, match="NORI_ERR_UNSUPPORTED.*NORI_SEED_NORI_BLOCK"):
        r.render_host(spp_count=2, seed_mode=_capi.SEED_NORI_BLOCK)
    lens, _ = r.render_host(spp_count=2)      # the context is usable, and the lens still set
    assert not np.array_equal(lens, before) and r.lens == (R, F)
    r.set_lens(0.0, F)
    blk, _ = r.render_host(spp_count=2, seed_mode=_capi.SEED_NORI_BLOCK)      # the pinhole renders in that mode as before
    assert blk[..., 3].sum() > 0
    r.set_lens(R, F)
    r.upload(sc)
    assert r.lens == (0.0, 0.0)
    after, _ = r.render_host(spp_count=2)
    assert after.tobytes() == before.tobytes()
    # Scene.camera's lens is applied by the upload
    sc.camera.aperture_radius, sc.camera.focus_distance = R, F
    r.upload(sc)
    assert r.lens == (R, F) and r.render_host(spp_count=2)[0].tobytes() == lens.tobytes()


def test_a_single_device_group_renders_the_contexts_frame(renderer_factory):
    sc = box_scene("path_mis", "gaussian", spp=4)
    r = renderer_factory(sc)
    r.set_lens(R, F)
    want, _ = r.render_host()
    g = DeviceGroup([0]).upload(sc)
    pin, _, _ = g.render_host()
    g.set_lens(R, F)
    got, _, _ = g.render_host()
    with pytest.raises(NoriError, match="NORI_ERR_INVALID_ARGUMENT"):
        g.set_lens(-1.0, F)
    g.close()
    assert got.tobytes() == want.tobytes() and not np.array_equal(pin, got)


# ------------------------------------------------------------------ 8. the counting build
_COUNT = """
import json, sys
sys.path.insert(0, %r)
from tests.test_gpu_lens import box_scene, ENGINES, R, F
from nori_amd.render import Renderer
for integrator in ("path_mis", "normals"):
    r = Renderer(0).upload(box_scene(integrator, "gaussian"), builder=2)
    r.set_lens(R, F)
    r.excursions(reset=True)
    rays = 0
    for engine in ENGINES:
        r.set_option("engine", engine)
        st = r.render_host(spp_count=8)[1]
        rays += st["n_closest_rays"]
    rays += r.render_features_host(spp_count=8)[1]["n_closest_rays"]
    print(json.dumps({"integrator": integrator, "rays": int(rays), "excursions": list(r.excursions())}), flush=True)
    r.close()
"""


def test_lens_arithmetic_stays_inside_its_verified_domain():
    lib = os.path.join(ROOT, "nori_amd", "lib", "libnori_hip_count.so")
    assert os.path.exists(lib), "libnori_hip_count.so missing: __graft_entry__.build() makes it"
    p = subprocess.run([sys.executable, "-c", _COUNT % ROOT], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, NORI_HIP_LIBRARY=lib), timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    rows = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == 2
    for row in rows:
        print("[excursions]", row)
        assert row["rays"] >= 3 * W * H * 8 and row["excursions"] == [0, 0, 0, 0], row      # (two engines and the feature pass: a ray per camera sample at least)
