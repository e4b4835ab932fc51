"""The second-moment film, the per-pixel error map and the render to a target error (include/nori_hip.h:
nori_hip_render_moments, nori_hip_error_map, nori_hip_render_to_error) on the GPU, against the oracle's binary64 film and
the numpy restatements of tests/moments_ref.py (validated on the CPU by tests/test_moments_cpu.py)."""
from __future__ import annotations

import functools
import os
import re
import subprocess

import numpy as np
import pytest

from nori_amd import NoriError, _capi, host
from nori_amd.scene import RFilter
from tests import film_cases, moments_ref as mr
from tests.backends import Oracle
from tests.test_gpu_parity import assert_within_summation_bound

pytestmark = pytest.mark.gpu

W, H = 45, 37      # 3 x 3 tiles of 16 x 16, the right and bottom ones partial
ENGINES = ["megakernel", "wavefront"]
FILTERS = {"box": RFilter("box"), "tent": RFilter("tent"), "gaussian": RFilter("gaussian"),
           "gaussian5.2": RFilter("gaussian", radius=5.2, stddev=1.3), "mitchell4": RFilter("mitchell", radius=4.0)}
RAYS = ("n_camera_samples", "n_closest_rays", "n_shadow_rays")
C = (0.5, 1.25, 3.0)            # the wall's radiance
C2 = (0.25, 1.5625, 9.0)        # its square, exact in float32


def _renderer(renderer_factory, sc, engine=None, **options):
    r = renderer_factory(sc)
    if engine is not None:
        r.set_option("engine", engine)
    for k, v in options.items():
        r.set_option(k, v)
    return r


# ------------------------------------------------------------------ 1. the beauty frame is unchanged
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", list(FILTERS))
def test_beauty_frame_has_the_bits_of_a_plain_render(renderer_factory, engine, name):
    r = _renderer(renderer_factory, film_cases.cornell(W, H, 33, FILTERS[name]), engine)
    for spp in (1, 3, 33):
        plain, ps = r.render_host(spp_count=spp)
        rgbw, m2, ms = r.render_moments_host(spp_count=spp)
        assert np.array_equal(plain, rgbw), (name, engine, spp)
        assert all(ps[k] == ms[k] for k in RAYS + ("n_invalid", "engine")), (ps, ms)
        assert np.isfinite(m2).all() and (m2[..., 3] >= 0).all() and m2[..., 3].max() > 0
        again, _ = r.render_host(spp_count=spp)       # and a plain render after one with moments
        assert np.array_equal(plain, again)


# ------------------------------------------------------------------ 2. varying radiance, box filter
N_BOX = 24


def _radiance_per_sample(renderer_factory, width, height):
    """Under the box filter a sample lands in its own pixel with weight exactly 1 (border 0): a 1-spp frame of sample s IS the
    radiance L_s per pixel, whatever the filter of the render it is compared with (the pcg32 stream is per pixel and sample)."""
    r = _renderer(renderer_factory, film_cases.cornell(width, height, N_BOX, RFilter("box")), "megakernel")
    assert r.border == 0
    frames = [r.render_host(spp_count=1, spp_begin=s)[0] for s in range(N_BOX)]
    L = np.stack([f[..., :3] for f in frames])
    assert all((f[..., 3] == 1).all() for f in frames) and np.isfinite(L).all() and L.max() > 0
    return L


@pytest.mark.parametrize("size", [(W, H), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_box_filter_moments_are_the_sum_of_squares(renderer_factory, monkeypatch, size):
    """m2.rgb against the binary64 sum of float32(L_s L_s), N = 24 terms per pixel, within (N + 16) 2^-24 sum L_s^2 -- the bound
    of assert_within_summation_bound.  The device adds fma(float32(L L), 1, sum): the square's own rounding is in the TERM
    here (the reference sum is over the rounded squares), so a term is rounded once more at most -- inside the + 16.  m2.w is N
    exactly.  On both engines, and with the samples cut into several launches / batches (the wavefront engine's pending
    gather beside the next batch included)."""
    width, height = size
    L = _radiance_per_sample(renderer_factory, width, height)
    sq = (L * L).astype(np.float32).astype(np.float64).sum(0)
    total = np.concatenate([sq, np.full(sq.shape[:2] + (1,), float(N_BOX))], -1)
    terms = np.full(sq.shape[:2], N_BOX, np.uint32)
    r = _renderer(renderer_factory, film_cases.cornell(width, height, N_BOX, RFilter("box")))
    for engine, batch, env in (("megakernel", 0, {}), ("megakernel", 0, {"NORI_HIP_FILM_SAMPLES": "4096"}),      # (read per call)
                               ("wavefront", 0, {}), ("wavefront", 4096, {})):
        r.set_option("engine", engine)
        r.set_option("wavefront_samples", batch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rgbw, m2, st = r.render_moments_host()
        for k in env:
            monkeypatch.delenv(k)
        assert st["n_camera_samples"] == width * height * N_BOX and st["engine"] == ENGINES.index(engine)
        assert_within_summation_bound(m2, total, total, terms, f"box moments {size} {engine} batch {batch} {env}")
        assert (m2[..., 3] == N_BOX).all() and (rgbw[..., 3] == N_BOX).all()


def test_block_seed_keeps_moments(renderer_factory):
    """The third producer, the block-serial kernel of NORI_SEED_NORI_BLOCK (one pcg32 stream per 32 x 32 block: other samples than
    the per-sample seed's, so other references).  Box filter, one sample: the pixel holds that sample's L with weight exactly 1,
    so m2 is float32(L L) and 1, exactly.  Any sample count: the beauty frame and the ray counts of a plain render.  The
    wall under the gaussian: every sample carries C, and C[0] = 0.5, C2[0] = 0.25 are powers of two -- scaling by one commutes
    with every rounding of the sums (no underflow here), and the four channels of a pixel are added in the same order, so the
    red channels are 0.5 W and 0.25 W exactly: the moments saw the positions and weights the frame saw."""
    block = _capi.SEED_NORI_BLOCK
    r = _renderer(renderer_factory, film_cases.cornell(W, H, 5, RFilter("box")))
    plain, ps = r.render_host(spp_count=1, seed_mode=block)
    rgbw, m2, ms = r.render_moments_host(spp_count=1, seed_mode=block)
    assert np.array_equal(plain, rgbw) and all(ps[k] == ms[k] for k in RAYS + ("n_invalid", "engine")), (ps, ms)
    assert (rgbw[..., 3] == 1).all() and rgbw[..., :3].max() > 0
    assert np.array_equal(m2[..., :3], (rgbw[..., :3] * rgbw[..., :3]).astype(np.float32)) and (m2[..., 3] == 1).all()
    plain, ps = r.render_host(seed_mode=block)
    rgbw, m2, ms = r.render_moments_host(seed_mode=block)
    assert np.array_equal(plain, rgbw) and all(ps[k] == ms[k] for k in RAYS + ("n_invalid", "engine")), (ps, ms)
    assert (m2[..., 3] == 5).all() and np.isfinite(m2).all()

    r = _renderer(renderer_factory, mr.emitter_wall(W, H, N_WALL, RFilter("gaussian"), C))
    plain, ps = r.render_host(seed_mode=block)
    rgbw, m2, ms = r.render_moments_host(seed_mode=block)
    assert np.array_equal(plain, rgbw) and all(ps[k] == ms[k] for k in RAYS + ("n_invalid", "engine")), (ps, ms)
    weight = rgbw[..., 3]
    assert weight.max() > 1 and np.array_equal(rgbw[..., 0], np.float32(0.5) * weight)
    assert np.array_equal(m2[..., 0], np.float32(0.25) * weight)
    assert np.isfinite(m2).all() and (m2[..., 3] >= 0).all() and m2[..., 3].max() > 0


# ------------------------------------------------------------------ 3. constant radiance, wide filters
N_WALL = 6


@functools.lru_cache(maxsize=None)
def _wall_reference(name):
    """(total, abs_total, terms) of the wall with radiance C2: the positions and weights of the render with radiance C.  First the
    premise, on the integrator the renders use (path_mats): every 1-spp box frame of the wall IS its radiance, exactly."""
    for c in (C, C2):
        o = Oracle(mr.emitter_wall(W, H, 1, RFilter("box"), c), use_bvh=True)
        for s in range(N_WALL):
            f, _ = o.render_host(spp_count=1, spp_begin=s)
            assert (f[..., :3] == np.array(c, np.float32)).all() and (f[..., 3] == 1).all()
        o.close()
    o = Oracle(mr.emitter_wall(W, H, N_WALL, FILTERS[name], C2), use_bvh=True)
    total, abs_total, terms, _ = o.render_f64(threads=1)
    o.close()
    for a in (total, abs_total, terms):
        a.setflags(write=False)
    return total, abs_total, terms


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ["tent", "gaussian", "gaussian5.2"])
def test_wide_filter_moments_against_the_squared_scene(renderer_factory, monkeypatch, engine, name):
    total, abs_total, terms = _wall_reference(name)
    sc = mr.emitter_wall(W, H, N_WALL, FILTERS[name], C)

    def check(rgbw, m2, what):
        assert_within_summation_bound(np.concatenate([m2[..., :3], rgbw[..., 3:]], -1), total, abs_total, terms, f"{name} {engine} {what}")

    r = _renderer(renderer_factory, sc, engine)
    check(*r.render_moments_host()[:2], "one call")
    shares = [r.render_moments_host(tile_mod=3, tile_rem=k)[:2] for k in range(3)]
    check((shares[0][0] + shares[1][0]) + shares[2][0], (shares[0][1] + shares[1][1]) + shares[2][1], "tile_mod 3 shares summed")
    if engine == "wavefront":
        r = _renderer(renderer_factory, sc, engine, wavefront_samples=4096)      # 9 tiles x 256 = 2304 samples per spp: a batch per sample index
        check(*r.render_moments_host()[:2], "wavefront_samples 4096")
    else:
        monkeypatch.setenv("NORI_HIP_FILM_SAMPLES", "4096")                      # read per call: one launch per sample index
        check(*r.render_moments_host()[:2], "NORI_HIP_FILM_SAMPLES 4096")


# ------------------------------------------------------------------ 4. sum of w^2
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ["gaussian", "tent"])
def test_sum_of_squared_weights(renderer_factory, engine, name):
    width, height, n = 31, 29, 8
    sc = mr.emitter_wall(width, height, n, FILTERS[name], C)
    o = Oracle(sc)
    table = o.filter_table()
    y, x, s = np.meshgrid(np.arange(height), np.arange(width), np.arange(n), indexing="ij")
    f = Oracle.pcg32_floats((y * width + x).reshape(-1), s.reshape(-1), 2)
    pos = np.stack([x.reshape(-1).astype(np.float32) + f[:, 0], y.reshape(-1).astype(np.float32) + f[:, 1]], -1)
    total, terms = mr.sum_w2(pos, width, height, mr.filter_radius(FILTERS[name]), table)
    o.close()
    r = _renderer(renderer_factory, sc, engine)
    rgbw, m2, _ = r.render_moments_host()
    four = lambda a: np.repeat(np.asarray(a)[..., None], 4, -1)
    assert_within_summation_bound(four(m2[..., 3]), four(total), four(total), terms, f"sum w^2 {name} {engine}")


# ------------------------------------------------------------------ 5. error map
def _check_error_map(r, rgbw, m2, threshold):
    want, empty = mr.error_map(rgbw, m2, r.border)
    err, s = r.error_map(rgbw, m2, threshold=threshold)
    assert err.dtype == np.float32 and np.array_equal(err, want)
    ref = mr.summary(want, empty, threshold)
    assert (s["n_pixels"], s["n_empty"], s["n_above"]) == (ref["n_pixels"], ref["n_empty"], ref["n_above"])
    assert s["max_err"] == ref["max_err"] and s["threshold"] == np.float32(threshold)
    # any order of adding n non-negative binary64 numbers is within n 2^-52 of any other, relative to the sum
    assert abs(s["sum_err"] - ref["sum_err"]) <= ref["n_pixels"] * 2.0 ** -52 * ref["sum_err"]
    err2, s2 = r.error_map(rgbw, m2, threshold=threshold)
    assert s2 == s and err2.tobytes() == err.tobytes()
    return err, s


def test_error_map_of_a_rendered_pair(renderer_factory):
    r = _renderer(renderer_factory, film_cases.cornell(W, H, 16, RFilter("gaussian")))
    rgbw, m2, _ = r.render_moments_host()
    err, s = _check_error_map(r, rgbw, m2, 0.05)
    assert s["n_empty"] == 0 and 0 < s["n_above"] < W * H and 0 < s["sum_err"] / s["n_pixels"] < 1


def test_error_map_of_a_hand_made_pair(renderer_factory):
    r = _renderer(renderer_factory, mr.emitter_wall(11, 9, 1, RFilter("gaussian"), C))
    rgbw, m2 = mr.hand_made_pair(border=r.border)
    assert rgbw.shape == tuple(r.frame_shape())
    err, s = _check_error_map(r, rgbw, m2, 0.1)
    assert s["n_empty"] == 3
    # every pixel special: all empty (99 pixels: one workgroup, 157 of its threads past the last pixel)
    err, s = _check_error_map(r, np.zeros_like(rgbw), m2, 0.0)
    assert s["n_empty"] == s["n_pixels"] == 99 and s["sum_err"] == 0 and s["n_above"] == 0
    # a negative threshold: every frame pixel is above it, the threads past the last pixel are not pixels
    err, s = _check_error_map(r, rgbw, m2, -1.0)
    assert s["n_above"] == s["n_pixels"] == 99


def test_error_map_summary_of_more_than_256_workgroups(renderer_factory):
    """320 x 208 pixels are 260 workgroups of 256: lanes 0 to 3 of the workgroup that adds the partials take two each (the
    strided loop a frame of 1024 x 1024 runs 16 times per lane), and the last map workgroup is full.  A made-up pair of
    frames (the map needs no render), against the numpy restatement like the small ones."""
    width, height = 320, 208
    r = _renderer(renderer_factory, mr.emitter_wall(width, height, 1, RFilter("gaussian"), C))
    rng = np.random.default_rng(11)
    shape = tuple(r.frame_shape())
    n = rng.uniform(3.0, 40.0, shape[:2]).astype(np.float32)
    mean = rng.uniform(0.0, 3.0, shape[:2] + (3,)).astype(np.float32)
    spread = rng.uniform(1.5, 6.0, shape[:2] + (3,)).astype(np.float32)
    rgbw = np.concatenate([mean * n[..., None], n[..., None]], -1).astype(np.float32)
    m2 = np.concatenate([mean * mean * spread * n[..., None], (n * np.float32(0.4))[..., None]], -1).astype(np.float32)
    rgbw[r.border + 5, r.border + 7] = 0          # one empty pixel
    assert rgbw.shape == shape and width * height == 260 * 256
    err, s = _check_error_map(r, rgbw, m2, 0.3)
    assert s["n_pixels"] == width * height and s["n_empty"] == 1 and 0 < s["n_above"] < s["n_pixels"]


# ------------------------------------------------------------------ 6. unsupported
def test_reference_order_keeps_no_moments(renderer_factory):
    r = _renderer(renderer_factory, film_cases.cornell(W, H, 2, RFilter("gaussian")), film_order="reference")
    with pytest.raises(NoriError, match=r"NORI_ERR_UNSUPPORTED: \S+"):
        r.render_moments_host()
    frame, st = r.render_host()
    assert st["n_camera_samples"] == W * H * 2 and np.isfinite(frame).all() and frame[..., 3].max() > 0


# ------------------------------------------------------------------ 7. render to a target error
def test_render_to_error_is_the_explicit_loop(renderer_factory):
    import torch
    r = _renderer(renderer_factory, film_cases.cornell(48, 48, 64, RFilter("gaussian")))
    zeros = lambda: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    rgbw, m2 = zeros(), zeros()
    stats, at16, means = [], None, []
    for k in range(16):
        stats.append(r.render_moments_into(rgbw, m2, spp_count=4, spp_begin=4 * k))
        s = r.error_map(rgbw, m2)[1]
        means.append(s["sum_err"] / s["n_pixels"])
        if k == 3:
            at16 = (rgbw.clone(), m2.clone())
    print("[render to error] mean error after 4, 8, ... spp:", " ".join(f"{m:.4f}" for m in means))

    a, b = zeros(), zeros()
    done, last, st = r.render_to_error(a, b, 0.0, pass_spp=4, spp_count=64)
    assert done == 64 and torch.equal(a, rgbw) and torch.equal(b, m2)
    assert all(st[k] == sum(x[k] for x in stats) for k in RAYS)
    assert last["sum_err"] / last["n_pixels"] == means[-1] and last["n_pixels"] == 48 * 48

    target = np.float32(means[3])
    if float(target) < means[3]:
        target = np.nextafter(target, np.float32(np.inf))      # the smallest float32 target the mean after 16 spp meets
    assert all(m > float(target) for m in means[1:3])          # (the first pass is not evaluated)
    a, b = zeros(), zeros()
    done, last, st = r.render_to_error(a, b, float(target), pass_spp=4, spp_count=64)
    assert done == 16 and torch.equal(a, at16[0]) and torch.equal(b, at16[1])
    assert all(st[k] == sum(x[k] for x in stats[:4]) for k in RAYS)
    assert last["sum_err"] / last["n_pixels"] == means[3]
    # a last pass shorter than the others; and one pass only: nothing to stop early, the summary still describes the frame
    done, last, _ = r.render_to_error(zeros(), zeros(), 0.0, pass_spp=5, spp_count=13)
    assert done == 13
    done, last, _ = r.render_to_error(zeros(), zeros(), 1e9, pass_spp=8, spp_count=8)
    assert done == 8 and last["n_pixels"] == 48 * 48 and last["sum_err"] > 0
    with pytest.raises(NoriError, match="INVALID_ARGUMENT"):
        r.render_to_error(zeros(), zeros(), 0.1, pass_spp=0)


# ------------------------------------------------------------------ 8. command line
def test_cli_target_error(renderer_factory, tmp_path):
    import torch
    (tmp_path / "floor.obj").write_text("v -3 0 -3\nv -3 0 3\nv 3 0 3\nv 3 0 -3\nf 1 2 3 4\n")
    (tmp_path / "light.obj").write_text("v -0.5 2 -0.5\nv 0.5 2 -0.5\nv 0.5 2 0.5\nv -0.5 2 0.5\nf 1 2 3 4\n")
    (tmp_path / "s.xml").write_text("""<scene><integrator type="path_mis"/>
      <sampler type="independent"><integer name="sampleCount" value="40"/></sampler>
      <camera type="perspective"><integer name="width" value="40"/><integer name="height" value="24"/><float name="fov" value="50"/>
        <transform name="toWorld"><lookat target="0, 0.5, 0" origin="0, 1, 4" up="0, 1, 0"/></transform></camera>
      <mesh type="obj"><string name="filename" value="floor.obj"/><bsdf type="diffuse"><color name="albedo" value="0.6,0.5,0.4"/></bsdf></mesh>
      <mesh type="obj"><string name="filename" value="light.obj"/><emitter type="area"><color name="radiance" value="8,8,8"/></emitter></mesh>
    </scene>""")
    sc = host.load_xml(str(tmp_path / "s.xml"))
    r = renderer_factory(sc, builder=2)
    zeros = lambda: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    # a target the loop meets part way: the mean error after 16 of the 40 samples
    a, b = zeros(), zeros()
    r.render_moments_into(a, b, spp_count=16)
    s = r.error_map(a, b)[1]
    target = float(np.float32(1.02 * s["sum_err"] / s["n_pixels"]))
    a, b = zeros(), zeros()
    done, last, _ = r.render_to_error(a, b, target, pass_spp=8, spp_count=40)
    assert 16 <= done < 40
    want = r.error_map(a, b)[0].cpu().numpy()

    exe = os.path.join(_capi.LIB_DIR, "nori")
    p = subprocess.run([exe, str(tmp_path / "s.xml"), "--target-error", repr(target), "--pass-spp", "8"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"Stopped at (\d+) samples per pixel: mean error ([0-9.eE+-]+)", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) == done
    assert abs(float(m.group(2)) - last["sum_err"] / last["n_pixels"]) <= 1e-5 * float(m.group(2))
    assert os.path.exists(tmp_path / "s.exr") and os.path.exists(tmp_path / "s.error.exr")
    got = host.load_exr(str(tmp_path / "s.error.exr"))
    assert got.shape == (24, 40, 3) and got.dtype == np.float32
    for c in range(3):      # 32-bit float channels hold the map exactly
        assert np.array_equal(got[..., c], want)
    from nori_amd.render import develop_host
    assert np.array_equal(host.load_exr(str(tmp_path / "s.exr")), develop_host(a.cpu().numpy(), r.border))
