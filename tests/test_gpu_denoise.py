"""The denoiser on the GPU (include/nori_hip.h: nori_hip_denoise) against the restatement of tests/denoise_ref.py, bit for bit on
the same rendered or hand-made frames: guide records, the filter over its parameters and feature terms, partial and small
frames, determinism and isolation, what it does to the error of a 16-spp render, errors and the command line.  Frames are
45 x 37 (3 x 3 tiles, the right column 13 px wide, the bottom row 5 px high) unless said otherwise."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nori_amd import NoriError, _capi, host
from nori_amd.render import Renderer, develop_host
from nori_amd.scene import RFilter
from tests import denoise_ref as dr, film_cases, moments_ref as mr
from tests.exr_reader import read_exr_rgb
from tests.test_gpu_features import FILTERS, scene_a, scene_b

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 45, 37
NAMES = ("albedo", "normal", "depth")
_cache = {}


def rendered(renderer_factory, scene, rf, spp=16, tile_mod=1, tile_rem=0):
    """(renderer, rgbw, m2, {name: frame}) of `spp` samples: rendered once per module, shared, read-only"""
    key = (scene, rf, spp, tile_mod, tile_rem)
    if key not in _cache:
        sc = {"A": scene_a, "B": scene_b, "plain": lambda f: film_cases.cornell(W, H, 1, FILTERS[f])}[scene](rf)
        r = renderer_factory(sc)
        rgbw, m2, _ = r.render_moments_host(spp_count=spp, tile_mod=tile_mod, tile_rem=tile_rem)
        feats, _ = r.render_features_host(spp_count=spp, tile_mod=tile_mod, tile_rem=tile_rem)
        for a in (rgbw, m2, *feats.values()):
            a.setflags(write=False)
        _cache[key] = (r, rgbw, m2, feats)
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()


def check(r, rgbw, m2, feats, what, **params):
    """denoise_host against the restatement, bit for bit; returns the pair"""
    rgb, wsum = r.denoise_host(rgbw, m2, **feats, **params)
    want, want_w = dr.denoise_frames(rgbw, m2, feats.get("albedo"), feats.get("normal"), feats.get("depth"), border=r.border, **params)
    bad = (rgb != want).any(-1) | (wsum != want_w)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert rgb.tobytes() == want.tobytes() and wsum.tobytes() == want_w.tobytes(), what
    return rgb, wsum


# ------------------------------------------------------------------ 1. guides
def test_guides_bit_for_bit(renderer_factory):
    r, rgbw, m2, feats = rendered(renderer_factory, "A", "gaussian")
    g = r.denoise_guides_host(rgbw, m2, **feats)
    want = dr.guides(rgbw, m2, feats["albedo"], feats["normal"], feats["depth"], border=r.border)
    assert g.shape == (H, W, 16) and g.tobytes() == want.tobytes()
    assert (g[..., 14] == 1).all() and (g[..., 3:6] > 0).any() and 0 < (g[..., 13] < 1).sum()
    none = r.denoise_guides_host(rgbw, m2)
    assert none.tobytes() == dr.guides(rgbw, m2, border=r.border).tobytes() and (none[..., 6:14] == 0).all()
    only = r.denoise_guides_host(rgbw, m2, depth=feats["depth"])
    assert only.tobytes() == dr.guides(rgbw, m2, depth=feats["depth"], border=r.border).tobytes()


# ------------------------------------------------------------------ 2. the filter
@pytest.mark.parametrize("terms,params", [
    (NAMES, {}),
    (NAMES, dict(radius=1, patch=0)),
    (NAMES, dict(radius=8, patch=2)),
    (NAMES, dict(radius=6, patch=0)),
    (NAMES, dict(radius=5, patch=2)),
    (("albedo",), {}), (("normal",), {}), (("depth",), {}), ((), {}),
    (NAMES, dict(alpha=0.0)),
    (NAMES, dict(k_c=0.45, alpha=0.5, tau_albedo=0.3, tau_normal=0.7, k_depth=0.6, tau_cov=0.2)),
], ids=lambda v: "-".join(v) if isinstance(v, tuple) else ",".join(f"{k}={x}" for k, x in v.items()) or "defaults")
def test_filter_bit_for_bit(renderer_factory, terms, params):
    r, rgbw, m2, feats = rendered(renderer_factory, "A", "gaussian")
    rgb, wsum = check(r, rgbw, m2, {n: feats[n] for n in terms}, (terms, params), **params)
    assert np.isfinite(rgb).all() and (wsum >= 1).all()
    if not params and terms == NAMES:
        assert (wsum > 1.5).mean() > 0.5      # the window is used: most pixels find neighbours


@pytest.mark.parametrize("scene,rf", [("A", "gaussian5"), ("B", "box"), ("A", "box")])
def test_filter_bit_for_bit_on_other_frames(renderer_factory, scene, rf):
    r, rgbw, m2, feats = rendered(renderer_factory, scene, rf)
    assert r.border == {"gaussian5": 5, "box": 0}[rf]
    check(r, rgbw, m2, feats, (scene, rf))
    if scene == "B":
        cov = dr.guides(rgbw, m2, feats["albedo"], feats["normal"], feats["depth"], border=r.border)[..., 13]
        assert ((cov > 0) & (cov < 1)).any() and (cov == 0).any()      # the soup has misses and partly covered pixels


# ------------------------------------------------------------------ 3. partial frames
def test_a_tile_share_leaves_empty_tiles(renderer_factory):
    r, rgbw, m2, feats = rendered(renderer_factory, "A", "box", tile_mod=2, tile_rem=1)
    rgb, wsum = check(r, rgbw, m2, feats, "tiles 1, 3, 5, 7")
    empty = ~(rgbw[..., 3] > 0)
    assert empty[:16, :16].all() and not empty[:16, 16:32].any()      # tile 0 is not of the share, tile 1 is
    assert (rgb[empty] == 0).all() and (wsum[empty] == 0).all() and (wsum[~empty] >= 1).all()


# ------------------------------------------------------------------ 4. small frames
@pytest.mark.parametrize("w,h", [(5, 3), (17, 16)])
def test_small_frames_under_the_largest_window(renderer_factory, w, h):
    r = renderer_factory(film_cases.cornell(w, h, 1, RFilter("gaussian")))
    rgbw, m2, _ = r.render_moments_host(spp_count=16)
    feats, _ = r.render_features_host(spp_count=16)
    for patch in (1, 2):
        rgb, wsum = check(r, rgbw, m2, feats, (w, h, patch), radius=8, patch=patch)
    assert rgb.shape == (h, w, 3) and (wsum >= 1).all()


# ------------------------------------------------------------------ 5. hand-made frames
def test_the_hand_made_pair(renderer_factory):
    r = renderer_factory(mr.emitter_wall(11, 9, 1, RFilter("gaussian"), (1.0, 1.0, 1.0)))
    rgbw, m2 = mr.hand_made_pair(border=r.border)
    assert rgbw.shape == tuple(r.frame_shape())
    rgb, wsum = check(r, rgbw, m2, {}, "hand-made pair")
    g = r.denoise_guides_host(rgbw, m2)
    assert g.tobytes() == dr.guides(rgbw, m2, border=r.border).tobytes()
    assert (g[..., 14] == 0).sum() == 3 and (wsum[g[..., 14] == 0] == 0).all()
    check(r, rgbw, m2, {}, "hand-made pair, R 8 F 2", radius=8, patch=2)


def wide_range_frames(shape, seed):
    """finite frames whose means span 1e-6 .. 1e4, E[L^2] / mean^2 in 0.5 .. 10 (below 1: the variance clamps), a few empty pixels"""
    rng = np.random.default_rng(seed)
    h, w = shape[:2]
    n = rng.uniform(3.0, 40.0, (h, w)).astype(F)
    mean = (10.0 ** rng.uniform(-6, 4, (h, w, 3))).astype(F)
    spread = (10.0 ** rng.uniform(np.log10(0.5), 1.0, (h, w, 3))).astype(F)
    rgbw = np.concatenate([mean * n[..., None], n[..., None]], -1).astype(F)
    m2 = np.concatenate([mean * mean * spread * n[..., None], (n * F(0.4))[..., None]], -1).astype(F)
    feats = {}
    for name in NAMES:
        f = rng.uniform(0.0, 1.0, (h, w, 4)).astype(F) * n[..., None]
        f[..., 3] = n
        feats[name] = f.astype(F)
    feats["depth"][..., 0] *= (10.0 ** rng.uniform(-3, 3, (h, w))).astype(F)
    hole = rng.uniform(size=(h, w)) < 0.03
    rgbw[hole] = 0
    feats["depth"][rng.uniform(size=(h, w)) < 0.1] = 0      # misses: z = cov = 0
    assert all(np.isfinite(a).all() for a in (rgbw, m2, *feats.values()))
    return rgbw, m2, feats


@pytest.mark.parametrize("seed", [1, 2])
def test_random_frames_of_large_dynamic_range(renderer_factory, seed):
    r = rendered(renderer_factory, "A", "gaussian")[0]
    rgbw, m2, feats = wide_range_frames(r.frame_shape(), seed)
    check(r, rgbw, m2, feats, "wide range")
    check(r, rgbw, m2, {}, "wide range, colour alone", radius=3, patch=2, k_c=0.7)
    g = r.denoise_guides_host(rgbw, m2, **feats)
    assert g.tobytes() == dr.guides(rgbw, m2, feats["albedo"], feats["normal"], feats["depth"], border=r.border).tobytes()


# ------------------------------------------------------------------ 6. determinism and isolation
def test_determinism_and_an_untouched_render(renderer_factory):
    r, rgbw, m2, feats = rendered(renderer_factory, "A", "gaussian")
    before, _ = r.render_host(spp_count=8)
    a = r.denoise_host(rgbw, m2, **feats)
    b = r.denoise_host(rgbw, m2, **feats)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    after, _ = r.render_host(spp_count=8)
    assert after.tobytes() == before.tobytes()


def test_two_streams_at_once(renderer_factory):
    import torch
    r, rgbw, m2, feats = rendered(renderer_factory, "A", "gaussian")
    rgbw2, m22, feats2 = wide_range_frames(r.frame_shape(), 7)
    jobs = [(rgbw, m2, feats, dict(radius=8, patch=2)), (rgbw2, m22, feats2, dict())]
    want = [r.denoise_host(a, b, **f, **p) for a, b, f, p in jobs]
    dev = lambda a: torch.from_numpy(np.array(a, F)).to("cuda:0")
    ins = [(dev(a), dev(b), {n: dev(f[n]) for n in NAMES}) for a, b, f, _ in jobs]
    outs = [(torch.full((H, W, 3), -1.0, device="cuda:0"), torch.full((H, W), -1.0, device="cuda:0")) for _ in jobs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for rep in range(3):
        for k in (0, 1):
            r.denoise_into(outs[k][0], ins[k][0], ins[k][1], wsum=outs[k][1], stream=streams[k], **ins[k][2], **jobs[k][3])
    torch.cuda.synchronize()
    for k in (0, 1):
        assert outs[k][0].cpu().numpy().tobytes() == want[k][0].tobytes() and outs[k][1].cpu().numpy().tobytes() == want[k][1].tobytes(), k
    # the tensor form of step A, and a NULL wsum
    g = torch.zeros((H, W, 16), device="cuda:0")
    r.denoise_guides_into(g, ins[0][0], ins[0][1], **ins[0][2])
    r.denoise_into(outs[0][0], ins[0][0], ins[0][1], **ins[0][2])
    torch.cuda.synchronize()
    assert g.cpu().numpy().tobytes() == r.denoise_guides_host(rgbw, m2, **feats).tobytes()
    assert outs[0][0].cpu().numpy().tobytes() == r.denoise_host(rgbw, m2, **feats)[0].tobytes()


# ------------------------------------------------------------------ 7. quality on GPU frames
def _ratio(renderer_factory, scene, rf):
    r, rgbw, m2, feats = rendered(renderer_factory, scene, rf)
    key = ("ref", scene, rf)
    if key not in _cache:
        _cache[key] = develop_host(r.render_host(spp_count=8192, spp_begin=100000)[0], r.border)
    ref = _cache[key]
    rgb, wsum = r.denoise_host(rgbw, m2, **feats)
    e_noisy, e_den = dr.trimmed_error(develop_host(rgbw, r.border), ref), dr.trimmed_error(rgb, ref)
    print(f"{scene} {rf}: noisy {e_noisy:.5f} denoised {e_den:.5f} ratio {e_den / e_noisy:.3f}")
    assert np.isfinite(rgb).all() and (wsum >= 1).all()
    return e_den / e_noisy


@pytest.mark.parametrize("scene", ["plain", "A"])
def test_error_at_16_spp_is_halved_under_the_box_filter(renderer_factory, scene):
    """trimmed ratio <= 0.5 against 8192 spp of a disjoint range: a float32 prototype of the operation gave 0.31 / 0.30"""
    assert _ratio(renderer_factory, scene, "box") <= 0.5


def test_error_at_16_spp_goes_down_under_the_gaussian_filter(renderer_factory):
    """neighbouring pixels share samples under a wide filter, so their differences understate the noise: only < 1 is asked"""
    assert _ratio(renderer_factory, "A", "gaussian") < 1.0


# ------------------------------------------------------------------ 8. errors
def test_errors_leave_the_context_usable(renderer_factory):
    r, rgbw, m2, feats = rendered(renderer_factory, "A", "gaussian")
    want = r.denoise_host(rgbw, m2, **feats)
    for bad, word in ((dict(radius=0), "radius"), (dict(radius=9), "radius"), (dict(patch=3), "patch"), (dict(k_c=0.0), "k_c"),
                      (dict(k_c=float("nan")), "k_c"), (dict(alpha=-0.5), "alpha"), (dict(tau_albedo=0.0), "tau"), (dict(tau_normal=-1.0), "tau"),
                      (dict(tau_cov=0.0), "tau"), (dict(k_depth=0.0), "k_depth")):
        with pytest.raises(NoriError, match=f"NORI_ERR_INVALID_ARGUMENT.*{word}"):
            r.denoise_host(rgbw, m2, **feats, **bad)
    lib, out, ws = r._lib, np.zeros((H, W, 3), F), np.zeros((H, W), F)
    p = _capi.DenoiseParams()
    ptr = _capi.ptr
    assert lib.nori_hip_denoise_host(r._h, C.byref(p), None, ptr(m2), None, None, None, ptr(out), ptr(ws)) == -1
    assert lib.nori_hip_denoise_host(r._h, C.byref(p), ptr(rgbw), None, None, None, None, ptr(out), ptr(ws)) == -1
    assert lib.nori_hip_denoise_host(r._h, C.byref(p), ptr(rgbw), ptr(m2), None, None, None, None, ptr(ws)) == -1
    assert lib.nori_hip_denoise_guides_host(r._h, ptr(rgbw), ptr(m2), None, None, None, None) == -1
    assert lib.nori_hip_denoise(r._h, None, None, None, None, None, None, None, None, None) == -1
    assert not out.any() and not ws.any()
    # params == NULL: the defaults; wsum == NULL
    assert lib.nori_hip_denoise_host(r._h, None, ptr(rgbw), ptr(m2), ptr(feats["albedo"]), ptr(feats["normal"]), ptr(feats["depth"]), ptr(out), None) == 0
    assert out.tobytes() == want[0].tobytes()
    again = r.denoise_host(rgbw, m2, **feats)
    assert again[0].tobytes() == want[0].tobytes() and again[1].tobytes() == want[1].tobytes()
    empty = Renderer(0)
    try:
        assert lib.nori_hip_denoise_host(empty._h, None, ptr(rgbw), ptr(m2), None, None, None, ptr(out), None) == -4      # NORI_ERR_NOT_READY
        assert lib.nori_hip_denoise_guides(empty._h, None, None, None, None, None, None, None) == -4
    finally:
        empty.close()


# ------------------------------------------------------------------ 9. the command line
def test_cli_denoise(renderer_factory, tmp_path):
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
    rgbw, m2, _ = r.render_moments_host()
    exe = os.path.join(_capi.LIB_DIR, "nori")
    for args, fspp, params in ((["--denoise"], 6, {}), (["--denoise", "--denoise-radius", "3", "--denoise-patch", "2", "--feature-spp", "4"], 4, dict(radius=3, patch=2))):
        feats, _ = r.render_features_host(spp_count=fspp)
        want, _ = r.denoise_host(rgbw, m2, **feats, **params)
        p = subprocess.run([exe, str(tmp_path / "s.xml")] + args, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "Denoised" in p.stdout and f"features of {fspp} samples per pixel" in p.stdout, p.stdout
        got = read_exr_rgb(str(tmp_path / "s.denoised.exr"))[1]
        assert got.shape == (24, 40, 3) and np.array_equal(got, want), args
        beauty = read_exr_rgb(str(tmp_path / "s.exr"))[1]
        assert np.array_equal(beauty, develop_host(rgbw, r.border))      # the usual output beside it
        os.remove(tmp_path / "s.denoised.exr")
