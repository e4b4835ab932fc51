"""First-hit feature frames on the GPU (include/nori_hip.h: nori_hip_render_features) against the restatement of
tests/features_ref.py: per sample bit for bit, filtered frames within the film's derived summation bound, one set of weights
with the beauty frame, independence of the mask, launches / shares / ranges, stats, errors and the command line.  Frames are
45 x 37 (3 x 3 tiles, the right column 13 px wide, the bottom row 5 px high) unless said otherwise."""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

from nori_amd import NoriError, _capi, host
from nori_amd.render import develop_features_host
from nori_amd.scene import Bsdf, RFilter, Texture
from tests import features_ref as fr, film_cases, moments_ref as mr, scenes
from tests.backends import Oracle
from tests.exr_reader import read_exr_rgb
from tests.test_gpu_parity import assert_within_summation_bound
from tests.test_gpu_textures import _textured_and_split

pytestmark = pytest.mark.gpu

W, H = 45, 37
NAMES = fr.NAMES
FILTERS = {"box": RFilter("box"), "gaussian": RFilter("gaussian"), "tent": RFilter("tent"), "gaussian5": RFilter("gaussian", radius=5.2, stddev=1.3)}


def scene_a(rf="gaussian", integrator="path_mis"):
    """the Cornell box with a mirror and a glass sphere; a bilinear repeat image at uv scale 4 on the floor, a checkerboard on the back
    wall (no texcoords: uv is the barycentric pair), the last mesh microfacet"""
    sc = film_cases.cornell(W, H, 1, FILTERS[rf], integrator=integrator)
    img = np.random.default_rng(11).uniform(0.05, 0.95, (7, 9, 3)).astype(np.float32)
    sc.textures = [Texture("image", img, "bilinear", "repeat", 4.0, 4.0), Texture("checkerboard", uscale=4.0, vscale=4.0, color0=(0.85, 0.3, 0.2), color1=(0.1, 0.5, 0.75))]
    by_name = {m.name: m for m in sc.meshes}
    by_name["floor"].albedo_texture = 0
    by_name["back"].albedo_texture = 1
    sc.meshes[-1].bsdf = Bsdf("microfacet", (0.2, 0.4, 0.6))
    return sc


def scene_b(rf="box"):
    sc = scenes.soup_scene(500, 1, W, H)
    sc.rfilter = FILTERS[rf]
    return sc


SCENES = {"A": scene_a, "B": scene_b}


@functools.lru_cache(maxsize=None)
def ref_samples(scene, begin, count):
    """(ps, values) of samples [begin, begin + count) of every pixel: computed once, shared, read-only"""
    ps, vals = fr.job_samples(SCENES[scene]("box"), begin, count)
    ps.setflags(write=False)
    for v in vals.values():
        v.setflags(write=False)
    return ps, vals


@functools.lru_cache(maxsize=None)
def ref_film(scene, rf, begin, count):
    """{name: (total, abs_total, terms)} of the job's binary64 film under filter rf"""
    sc = SCENES[scene](rf)
    o = Oracle(sc, use_bvh=True)
    table = o.filter_table()
    o.close()
    ps, vals = ref_samples(scene, begin, count)
    films = fr.film_f64(ps, [vals[n] for n in NAMES], W, H, mr.filter_radius(sc.rfilter), table)
    return dict(zip(NAMES, films))


def check_films(frames, scene, rf, begin, count, what):
    films = ref_film(scene, rf, begin, count)
    for n in NAMES:
        assert_within_summation_bound(frames[n], *films[n], what=f"{what} {n}")


def test_scene_a_has_hits_and_misses():
    _, vals = ref_samples("A", 0, 1)
    assert 0.05 <= 1.0 - vals["hit"].mean() <= 0.60
    _, vals = ref_samples("B", 0, 1)
    assert 0.05 <= 1.0 - vals["hit"].mean() <= 0.60


# ------------------------------------------------------------------ 1. per sample, bit for bit
def _per_sample(r, scene):
    for s in (0, 1, 5):
        frames, st = r.render_features_host(spp_begin=s, spp_count=1)
        _, vals = ref_samples(scene, s, 1)
        assert st["n_invalid"] == 0
        for n in NAMES:
            f = frames[n]
            assert f.shape == (H, W, 4) and (f[..., 3] == 1).all(), (scene, s, n)
            want = vals[n].reshape(H, W, 3)
            assert np.array_equal(f[..., :3], want), (scene, s, n, int((f[..., :3] != want).any(axis=-1).sum()))


@pytest.mark.parametrize("builder", [0, 2])
@pytest.mark.parametrize("scene", ["A", "B"])
def test_every_sample_bit_for_bit(renderer_factory, scene, builder):
    _per_sample(renderer_factory(SCENES[scene]("box"), builder=builder), scene)


def test_every_sample_bit_for_bit_on_wide_nodes(renderer_factory):
    r = renderer_factory(scene_a("box"), build=False)
    r.set_option("accel_layout", "bvh4q")
    r.build_accel(0)
    assert r.accel_info()["node_children"] == 4
    _per_sample(r, "A")


TOP = 2 ** 32 - 1      # the last sample index: spp_begin + spp_count is 2^32 there, one past uint32


def test_the_top_of_the_sample_range(renderer_factory):
    """The pass counts a chunk's samples relative to spp_begin, as render_kernel does: the sample 2^32 - 1 is rendered (an end formed
    in uint32 wraps to 0 and the pass renders nothing, with success), alone bit for bit and as the last of three in one call."""
    r = renderer_factory(scene_a("box"))
    frames, st = r.render_features_host(spp_begin=TOP, spp_count=1)
    _, vals = ref_samples("A", TOP, 1)
    assert st["n_invalid"] == 0
    print("sample 2^32 - 1: camera samples", st["n_camera_samples"], "of", W * H)
    for n in NAMES:
        f, want = frames[n], vals[n].reshape(H, W, 3)
        print("sample 2^32 - 1", n, int((f[..., :3] != want).any(axis=-1).sum()), "pixels differ, weight", float(f[..., 3].sum()))
    assert st["n_camera_samples"] == st["n_closest_rays"] == W * H
    for n in NAMES:
        f, want = frames[n], vals[n].reshape(H, W, 3)
        assert f.shape == (H, W, 4) and (f[..., 3] == 1).all(), n
        assert np.array_equal(f[..., :3], want), (n, int((f[..., :3] != want).any(axis=-1).sum()))
    # [2^32 - 3, 2^32) in one call: the binary64 film of the three samples, and the three single-sample frames combined
    singles = []
    for s in (TOP - 2, TOP - 1, TOP):
        one, s1 = r.render_features_host(spp_begin=s, spp_count=1)
        _, v1 = ref_samples("A", s, 1)
        assert s1["n_camera_samples"] == W * H and all(np.array_equal(one[n][..., :3], v1[n].reshape(H, W, 3)) for n in NAMES), s
        singles.append(one)
    three, st = r.render_features_host(spp_begin=TOP - 2, spp_count=3)
    print("samples 2^32 - 3 .. 2^32 - 1: camera samples", st["n_camera_samples"], "of", 3 * W * H)
    assert st["n_camera_samples"] == st["n_closest_rays"] == 3 * W * H and st["n_invalid"] == 0
    check_films(three, "A", "box", TOP - 2, 3, "[2^32 - 3, 2^32)")
    for n in NAMES:
        total = sum(one[n].astype(np.float64) for one in singles)      # (the values are not negative: the sum of magnitudes is the sum)
        assert (three[n][..., 3] == 3).all(), n
        assert_within_summation_bound(three[n], total, total, np.full((H, W), 3, np.uint32), what=f"three single frames combined, {n}")


# ------------------------------------------------------------------ 2. filtered frames
@pytest.mark.parametrize("rf", ["gaussian", "tent", "gaussian5"])
def test_filtered_frames_within_the_summation_bound(renderer_factory, rf):
    r = renderer_factory(scene_a(rf))
    frames, st = r.render_features_host(spp_count=33)
    assert st["n_invalid"] == 0
    check_films(frames, "A", rf, 0, 33, f"{rf} 33 spp")


# ------------------------------------------------------------------ 3. one set of weights
def test_weights_are_the_beauty_frames(renderer_factory):
    r = renderer_factory(scene_a("gaussian"))
    r.set_option("engine", "megakernel")
    beauty, sb = r.render_host(spp_count=33)
    frames, sf = r.render_features_host(spp_count=33)
    assert sb["engine"] == 0 and sb["n_invalid"] == 0 and sf["n_invalid"] == 0      # the premise: no sample was dropped on either side
    for n in NAMES:
        assert np.array_equal(frames[n][..., 3], frames["albedo"][..., 3]), n
        assert np.array_equal(frames[n][..., 3], beauty[..., 3]), n


# ------------------------------------------------------------------ 4. independence and determinism
def test_mask_independence_determinism_and_an_untouched_render(renderer_factory):
    r = renderer_factory(scene_a("gaussian"))
    before, _ = r.render_host(spp_count=8)
    all3, _ = r.render_features_host(spp_count=33)
    for n in NAMES:
        one, st = r.render_features_host(features=(n,), spp_count=33)
        assert list(one) == [n] and np.array_equal(one[n], all3[n]), n
    again, _ = r.render_features_host(spp_count=33)
    for n in NAMES:
        assert again[n].tobytes() == all3[n].tobytes(), n
    after, _ = r.render_host(spp_count=8)
    assert after.tobytes() == before.tobytes()


# ------------------------------------------------------------------ 5. several launches, shares, ranges
def test_several_launches(renderer_factory, monkeypatch):
    r = renderer_factory(scene_a("gaussian"))
    monkeypatch.setenv("NORI_HIP_FILM_SAMPLES", str(9 * 256 * 7))
    frames, st = r.render_features_host(spp_count=40, time_kernels=True)
    monkeypatch.delenv("NORI_HIP_FILM_SAMPLES")
    assert st["n_trace_launches"] == 6 and st["n_camera_samples"] == W * H * 40
    check_films(frames, "A", "gaussian", 0, 40, "six launches")


def test_tile_shares_and_sample_ranges(renderer_factory):
    import torch
    r = renderer_factory(scene_a("gaussian"))
    zeros = lambda: {n: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0") for n in NAMES}
    t = zeros()
    n_cam = 0
    for rem in range(3):
        n_cam += r.render_features_into(spp_count=12, tile_mod=3, tile_rem=rem, **t)["n_camera_samples"]
    assert n_cam == W * H * 12
    check_films({n: t[n].cpu().numpy() for n in NAMES}, "A", "gaussian", 0, 12, "three tile shares")
    t = zeros()
    r.render_features_into(spp_begin=0, spp_count=5, **t)
    r.render_features_into(spp_begin=5, spp_count=7, want_stats=False, **t)
    torch.cuda.synchronize()
    check_films({n: t[n].cpu().numpy() for n in NAMES}, "A", "gaussian", 0, 12, "[0, 5) then [5, 12)")


# ------------------------------------------------------------------ 6. textured = split
def test_textured_scene_gives_the_split_scenes_frames(renderer_factory):
    tx, sp = _textured_and_split("path_mis", W, H, 4)
    (A, sa), (B, sb) = (renderer_factory(s, builder=2).render_features_host() for s in (tx, sp))
    assert sa["n_closest_rays"] == sb["n_closest_rays"] == W * H * 4
    for n in NAMES:
        assert np.array_equal(A[n], B[n]), (n, int((A[n] != B[n]).sum()))
    assert len(np.unique(develop_features_host(A, 2)["albedo"].reshape(-1, 3).round(3), axis=0)) > 4      # the textures show


# ------------------------------------------------------------------ 7. stats
def test_stats(renderer_factory):
    r = renderer_factory(scene_a("gaussian"))
    _, st = r.render_features_host(spp_count=6, spp_begin=2, time_kernels=True)
    _, sn = renderer_factory(scene_a("gaussian", integrator="normals")).render_host(spp_count=6, spp_begin=2)
    assert st["n_camera_samples"] == W * H * 6
    assert st["n_closest_rays"] == sn["n_closest_rays"] == W * H * 6
    assert st["n_shadow_rays"] == 0 and st["engine"] == 3 and st["n_invalid"] == 0
    assert st["n_node_tests"] == 0 and st["n_tri_tests"] == 0
    assert st["n_trace_launches"] == 1 and st["trace_ms"] > 0 and st["film_ms"] > 0 and st["kernel_ms"] > 0
    assert st["lds_bytes"] in (16 * 1024, 24 * 1024, 32 * 1024, 64 * 1024)


# ------------------------------------------------------------------ 8. errors
def test_errors_leave_the_context_usable(renderer_factory):
    import torch
    r = renderer_factory(scene_a("gaussian"))
    before, _ = r.render_host(spp_count=4)
    t = torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    with pytest.raises(NoriError, match="NORI_ERR_INVALID_ARGUMENT"):
        r.render_features_into(albedo=t, spp_count=1, features=0)
    with pytest.raises(NoriError, match="NORI_ERR_INVALID_ARGUMENT"):
        r.render_features_into(albedo=t, spp_count=1, features=8 | 1)
    with pytest.raises(NoriError, match="NORI_ERR_INVALID_ARGUMENT"):
        r.render_features_into(albedo=t, spp_count=1, features=7)          # normal and depth asked for, no frames
    with pytest.raises(NoriError, match="NORI_ERR_UNSUPPORTED.*NORI_SEED_PER_SAMPLE"):
        r.render_features_into(albedo=t, spp_count=1, seed_mode=_capi.SEED_NORI_BLOCK)
    assert not t.any()
    after, _ = r.render_host(spp_count=4)
    assert after.tobytes() == before.tobytes()
    frames, _ = r.render_features_host(features=("depth",), spp_count=1)
    assert frames["depth"][..., 3].sum() > 0
    unbuilt = renderer_factory(scene_a("gaussian"), build=False)
    with pytest.raises(NoriError, match="NORI_ERR_NOT_READY"):
        unbuilt.render_features_host(spp_count=1)


# ------------------------------------------------------------------ 9. the command line
def test_cli_features(renderer_factory, tmp_path):
    (tmp_path / "floor.obj").write_text("v -3 0 -3\nv -3 0 3\nv 3 0 3\nv 3 0 -3\nf 1 2 3 4\n")
    (tmp_path / "light.obj").write_text("v -0.5 2 -0.5\nv 0.5 2 -0.5\nv 0.5 2 0.5\nv -0.5 2 0.5\nf 1 2 3 4\n")
    (tmp_path / "s.xml").write_text("""<scene><integrator type="path_mis"/>
      <sampler type="independent"><integer name="sampleCount" value="6"/></sampler>
      <camera type="perspective"><integer name="width" value="40"/><integer name="height" value="24"/><float name="fov" value="50"/>
        <transform name="toWorld"><lookat target="0, 0.5, 0" origin="0, 1, 4" up="0, 1, 0"/></transform></camera>
      <mesh type="obj"><string name="filename" value="floor.obj"/><bsdf type="diffuse"><color name="albedo" value="0.6,0.5,0.4"/></bsdf></mesh>
      <mesh type="obj"><string name="filename" value="light.obj"/><emitter type="area"><color name="radiance" value="8,8,8"/></emitter></mesh>
    </scene>""")
    r = renderer_factory(host.load_xml(str(tmp_path / "s.xml")), builder=2)
    frames, _ = r.render_features_host(spp_count=4)
    want = develop_features_host(frames, r.border)
    exe = os.path.join(_capi.LIB_DIR, "nori")
    p = subprocess.run([exe, str(tmp_path / "s.xml"), "--features", "--feature-spp", "4"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Feature frames (albedo, normal, depth) of 4 samples per pixel" in p.stdout, p.stdout
    for n in NAMES:
        path = tmp_path / f"s.{n}.exr"
        assert path.exists(), n
        got = read_exr_rgb(str(path))[1]
        assert got.shape == (24, 40, 3) and np.array_equal(got, want[n]), n
    cov = want["depth"][..., 1]
    assert (cov < 1).any() and (cov > 0).any()      # the frame sees past the floor: hits and misses are in it
