"""The denoiser's output variance, the error of a denoised frame and the adaptive loop that stops on it, on the GPU (include/nori_hip.h:
nori_hip_denoise_var, nori_hip_denoised_error_map, nori_hip_denoised_tile_errors, nori_hip_render_adaptive_denoised) against the
restatement of tests/denoise_error_ref.py (validated by tests/test_denoise_error_cpu.py), bit for bit, and a replay of the loop from
outside.  Frames are 45 x 37 (3 x 3 tiles, the right column 13 px wide, the bottom row 5 px high), 72 x 40 and 5 x 3."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nori_amd import NoriError, _capi, host
from nori_amd.scene import RFilter
from tests import adaptive_ref as ar, denoise_error_ref as de, film_cases, moments_ref as mr
from tests.exr_reader import read_exr_rgb
from tests.test_gpu_adaptive import wall_and_cornell
from tests.test_gpu_denoise import wide_range_frames
from tests.test_gpu_features import scene_a

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 45, 37
NAMES = ("albedo", "normal", "depth")
ENGINES = ["megakernel", "wavefront"]
LISTS = [(0, 4, 8), (5,), (2, 3, 7, 8), tuple(range(9))]
SENTINEL = -7.25
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()


def rendered(renderer_factory):
    """(renderer, rgbw, m2, feats) of 16 samples of the textured scene under the gaussian filter: rendered once, shared, read-only"""
    if "A" not in _cache:
        r = renderer_factory(scene_a("gaussian"))
        rgbw, m2, _ = r.render_moments_host(spp_count=16)
        feats, _ = r.render_features_host(spp_count=16)
        for a in (rgbw, m2, *feats.values()):
            a.setflags(write=False)
        _cache["A"] = (r, rgbw, m2, feats)
    return _cache["A"]


def made_up(r, seed=3):
    """random frames of a large dynamic range with empty pixels (tests/test_gpu_denoise.py), shared, read-only"""
    key = ("made up", seed)
    if key not in _cache:
        rgbw, m2, feats = wide_range_frames(r.frame_shape(), seed)
        for a in (rgbw, m2, *feats.values()):
            a.setflags(write=False)
        _cache[key] = (rgbw, m2, feats)
    return _cache[key]


def check(r, rgbw, m2, feats, what, **params):
    """denoise_var_host: rgb and wsum are nori_hip_denoise's bytes, var the restatement's; returns the triple"""
    rgb, var, wsum = r.denoise_var_host(rgbw, m2, **feats, **params)
    rgb0, wsum0 = r.denoise_host(rgbw, m2, **feats, **params)
    assert np.array_equal(rgb, rgb0) and np.array_equal(wsum, wsum0), what
    assert rgb.tobytes() == rgb0.tobytes() and wsum.tobytes() == wsum0.tobytes(), what
    _, want, _ = de.denoise_var_frames(rgbw, m2, feats.get("albedo"), feats.get("normal"), feats.get("depth"), border=r.border, **params)
    bad = (var != want).any(-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert var.tobytes() == want.tobytes(), what
    return rgb, var, wsum


# ------------------------------------------------------------------ 1. the filter with its variance
@pytest.mark.parametrize("terms", [NAMES, ("normal",), ()], ids=lambda t: "-".join(t) or "none")
@pytest.mark.parametrize("R,Fp", [(5, 1), (8, 2), (1, 0), (6, 1)])
def test_variance_bit_for_bit(renderer_factory, R, Fp, terms):
    r, rgbw, m2, feats = rendered(renderer_factory)
    rgb, var, wsum = check(r, rgbw, m2, {n: feats[n] for n in terms}, ("rendered", R, Fp, terms), radius=R, patch=Fp)
    assert np.isfinite(var).all() and (var >= 0).all() and (var > 0).any() and (wsum >= 1).all()
    rgbw2, m22, feats2 = made_up(r)
    rgb, var, wsum = check(r, rgbw2, m22, {n: feats2[n] for n in terms}, ("made up", R, Fp, terms), radius=R, patch=Fp)
    empty = ~(rgbw2[r.border:r.border + H, r.border:r.border + W, 3] > 0)
    assert empty.any() and not var[empty].any() and not wsum[empty].any() and (var[~empty] >= 0).all()


@pytest.mark.parametrize("w,h", [(72, 40), (5, 3)])
def test_variance_on_other_frame_sizes(renderer_factory, w, h):
    r = renderer_factory(film_cases.cornell(w, h, 1, RFilter("box")))
    rgbw, m2, _ = r.render_moments_host(spp_count=16)
    feats, _ = r.render_features_host(spp_count=16)
    for params in (dict(), dict(radius=8, patch=2)):
        rgb, var, wsum = check(r, rgbw, m2, feats, (w, h, params), **params)
    assert var.shape == (h, w, 3) and (wsum >= 1).all()


# ------------------------------------------------------------------ 2. tile lists
def test_a_tile_list_writes_its_tiles_and_nothing_else(renderer_factory):
    import torch
    r, rgbw, m2, feats = rendered(renderer_factory)
    dev = lambda a: torch.from_numpy(np.array(a, F)).to("cuda:0")
    ins = (dev(rgbw), dev(m2))
    fd = {n: dev(feats[n]) for n in NAMES}
    ys, xs = np.mgrid[0:H, 0:W]
    tile_of = (ys // 16) * 3 + xs // 16
    for params in (dict(), dict(radius=8, patch=2)):
        whole = r.denoise_var_host(rgbw, m2, **feats, **params)
        for tiles in LISTS:
            listed = np.isin(tile_of, tiles)
            out = [torch.full(s, SENTINEL, device="cuda:0") for s in ((H, W, 3), (H, W, 3), (H, W))]
            r.denoise_var_into(out[0], out[1], *ins, wsum=out[2], tiles=tiles, **fd, **params)
            torch.cuda.synchronize()
            host_out = tuple(np.full(s, SENTINEL, F) for s in ((H, W, 3), (H, W, 3), (H, W)))
            r.denoise_var_host(rgbw, m2, **feats, tiles=tiles, out=host_out, **params)
            for got, twin, want in zip(out, host_out, whole):
                got = got.cpu().numpy()
                assert got[listed].tobytes() == want[listed].tobytes(), (tiles, params)
                assert (got[~listed] == F(SENTINEL)).all(), (tiles, params)
                assert twin.tobytes() == got.tobytes(), (tiles, params)
    # the empty list touches nothing; bad lists are refused as for render_tiles
    out = [torch.full(s, SENTINEL, device="cuda:0") for s in ((H, W, 3), (H, W, 3), (H, W))]
    r.denoise_var_into(out[0], out[1], *ins, wsum=out[2], tiles=[], **fd)
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in out)
    for tiles, word in (([0, 9], "out of range"), ([4, 0xffffffff], "out of range"), ([3, 2], "ascending"), ([1, 5, 5, 6], "ascending")):
        with pytest.raises(NoriError, match=rf"NORI_ERR_INVALID_ARGUMENT: .*{word}"):
            r.denoise_var_into(out[0], out[1], *ins, wsum=out[2], tiles=tiles, **fd)
        with pytest.raises(NoriError, match=rf"NORI_ERR_INVALID_ARGUMENT: .*{word}"):
            r.denoise_var_host(rgbw, m2, **feats, tiles=tiles)
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in out)
    # a NULL wsum, a NULL variance, bad parameters
    r.denoise_var_into(out[0], out[1], *ins, **fd)
    torch.cuda.synchronize()
    whole = r.denoise_var_host(rgbw, m2, **feats)
    assert out[0].cpu().numpy().tobytes() == whole[0].tobytes() and out[1].cpu().numpy().tobytes() == whole[1].tobytes() and (out[2] == SENTINEL).all()
    p = _capi.DenoiseParams()
    raw = lambda t: C.c_void_p(t.data_ptr())
    assert r._lib.nori_hip_denoise_var(r._h, C.byref(p), raw(ins[0]), raw(ins[1]), None, None, None, None, 0, raw(out[0]), None, None, None) == -1
    assert r._lib.nori_hip_denoise_var(r._h, C.byref(p), None, raw(ins[1]), None, None, None, None, 0, raw(out[0]), raw(out[1]), None, None) == -1
    with pytest.raises(NoriError, match="NORI_ERR_INVALID_ARGUMENT.*radius"):
        r.denoise_var_host(rgbw, m2, radius=9)
    again = r.denoise_var_host(rgbw, m2, **feats)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, whole))


# ------------------------------------------------------------------ 3. error map, summary, tile errors
def made_up_outputs(h, w, seed):
    """(rgb, var, wsum) as a filter might have written them: variances over six decades, empty pixels, a tile of nothing but empty ones"""
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(0.0, 2.0, (h, w, 3)).astype(F)
    rgb[rng.uniform(size=(h, w)) < 0.02] = 0                      # black pixels: den = 0.03 alone
    var = (10.0 ** rng.uniform(-7, -1, (h, w, 3))).astype(F)
    var[rng.uniform(size=(h, w)) < 0.02] = 0
    wsum = rng.uniform(1.0, 120.0, (h, w)).astype(F)
    wsum[rng.uniform(size=(h, w)) < 0.03] = 0
    if h > 32 and w > 32:
        wsum[16:32, 16:32] = 0
    scale = rng.uniform(0.2, 5.0, ar.tile_grid(w, h)).astype(F)      # errors that differ from tile to tile
    var *= np.repeat(np.repeat(scale, 16, 0), 16, 1)[:h, :w, None]
    return rgb, var.astype(F), wsum


def check_errors(r, rgb, var, wsum, threshold, what):
    import torch
    want, empty = de.pixel_error(rgb, var, wsum)
    want_s = de.summary(want, empty, threshold)
    err, s = r.denoised_error_map(rgb, var, wsum, threshold=threshold)
    assert err.tobytes() == want.tobytes(), what
    assert {k: s[k] for k in want_s} == want_s, (what, s, want_s)
    assert s["threshold"] == float(F(threshold))
    assert np.float64(s["sum_err"]).tobytes() == np.float64(want_s["sum_err"]).tobytes(), what
    err2, s2 = r.denoised_error_map(rgb, var, wsum, threshold=threshold)
    assert err2.tobytes() == err.tobytes() and s2 == s
    none, s3 = r.denoised_error_map(rgb, var, wsum, threshold=threshold, want_map=False)
    assert none is None and s3 == s
    te = r.denoised_tile_errors(rgb, var, wsum)
    want_te = de.tile_errors(rgb, var, wsum)
    assert te.dtype == F and te.shape == want_te.shape and te.tobytes() == want_te.tobytes(), what
    assert r.denoised_tile_errors(rgb, var, wsum).tobytes() == te.tobytes()
    d = [torch.from_numpy(a).cuda() for a in (rgb, var, wsum)]
    derr, ds = r.denoised_error_map(*d, threshold=threshold)
    assert derr.cpu().numpy().tobytes() == err.tobytes() and ds == s
    assert r.denoised_tile_errors(*d).cpu().numpy().tobytes() == te.tobytes()
    return err, s, te


def test_error_map_summary_and_tile_errors_bit_for_bit(renderer_factory):
    r, rgbw, m2, feats = rendered(renderer_factory)
    rgb, var, wsum = r.denoise_var_host(rgbw, m2, **feats)
    err, s, te = check_errors(r, rgb, var, wsum, float(np.median(de.pixel_error(rgb, var, wsum)[0])), "rendered")
    assert s["n_empty"] == 0 and 0 < s["n_above"] < W * H and (te > 0).all()
    rgb, var, wsum = made_up_outputs(H, W, 5)
    err, s, te = check_errors(r, rgb, var, wsum, float(np.median(de.pixel_error(rgb, var, wsum)[0])), "made up")
    assert s["n_empty"] == int((~(wsum > 0)).sum()) > 256 and te[1, 1] == 0 and np.count_nonzero(te) == 8
    lib, ptr = r._lib, _capi.ptr
    assert lib.nori_hip_denoised_error_map_host(r._h, ptr(rgb), ptr(var), ptr(wsum), None, 0.0, None) == -1
    assert lib.nori_hip_denoised_error_map_host(r._h, ptr(rgb), None, ptr(wsum), ptr(err), 0.0, None) == -1
    assert lib.nori_hip_denoised_tile_errors_host(r._h, ptr(rgb), ptr(var), None, ptr(te)) == -1
    assert lib.nori_hip_denoised_tile_errors_host(r._h, ptr(rgb), ptr(var), ptr(wsum), None) == -1


def test_errors_of_a_frame_of_several_hundred_tiles(renderer_factory):
    """520 x 520 is 33 x 33 = 1089 tiles, the last column and row 8 pixels wide, and 1057 workgroups of the map: lanes of the
    summary's second stage own several partials.  Made-up buffers, no render."""
    r = renderer_factory(mr.emitter_wall(520, 520, 1, RFilter("box"), (0.5, 1.25, 3.0)))
    rgb, var, wsum = made_up_outputs(520, 520, 9)
    err, s, te = check_errors(r, rgb, var, wsum, 0.05, "520 x 520")
    assert te.shape == (33, 33) and te[1, 1] == 0 and s["n_pixels"] == 520 * 520 and 0 < s["n_above"] < s["n_pixels"]


# ------------------------------------------------------------------ 4. the loop, by replay
# The target is an input chosen BEFOREHAND from the CPU restatement (tests/denoise_error_ref.replay_loop) on oracle frames of this
# scene -- 48 one-sample oracle renders under the box filter, the restated feature samples of 16 spp -- so that tiles retire in
# several passes and some never do.  Denoised tile errors of the oracle frames (tiles 3, 4, 8, 9, 13, 14 see only the wall):
#     after pass 2 (16 spp)  0: .0324  1: .0557  2: .0142  5: .0419  6: .0838  7: .0170  10: .0450  11: .1505  12: .0264, wall 0
#                            -> stay 1, 6, 10, 11
#     after pass 3 (24 spp)  1: .0535  6: .0715  10: .0363  11: .1357     -> 10 retires
#     after pass 4 (32 spp)  1: .0471  6: .0697  11: .1270                -> all stay
#     after pass 5 (40 spp)  1: .0431  6: .0687  11: .1227                -> 1 retires
#     after pass 6 (48 spp)  6: .0645  11: .1151                          -> the budget: two tiles still active
# oracle tile_spp = 16 40 16 16 16 / 16 48 16 16 16 / 24 48 16 16 16.  The nearest errors on either side of E = 0.044 are .0431 and
# .0450: a gap of 2 % on each side, where the GPU's frames differ from the oracle's by the order of float32 sums.
LOOP_E, LOOP_K, LOOP_N, LOOP_FEATURE_SPP = 0.044, 8, 48, 16


@pytest.mark.parametrize("engine", ENGINES)
def test_the_loop_is_its_replay(renderer_factory, engine):
    """Conditions of the test (asserted at the end): tile_spp takes at least two distinct values below the budget, and not every
    tile ends at the budget while at least one does."""
    import torch
    width, height = 72, 40
    K, N, E = LOOP_K, LOOP_N, LOOP_E
    r = renderer_factory(wall_and_cornell(width, height, N, RFilter("box")))
    r.set_option("engine", engine)
    zeros = lambda: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    fd = {n: zeros() for n in NAMES}
    r.render_features_into(**fd, spp_count=LOOP_FEATURE_SPP)
    a, b = zeros(), zeros()
    rgb, var, wsum, tile_spp_t, summary, stats = r.render_adaptive_denoised(a, b, E, **fd, pass_spp=K, spp_count=N)
    tile_spp = tile_spp_t.cpu().numpy().astype(np.int64).reshape(-1)
    n = tile_spp.size
    assert n == 15 and summary["n_tiles"] == n
    print(f"[denoised loop] {engine}: tile_spp {tile_spp.tolist()} summary {summary}")

    def filtered(x, y):
        out = (torch.empty((height, width, 3), device="cuda:0"), torch.empty((height, width, 3), device="cuda:0"), torch.empty((height, width), device="cuda:0"))
        r.denoise_var_into(out[0], out[1], x, y, wsum=out[2], **fd)
        return out

    ra, rb = zeros(), zeros()
    replay_stats, passes, active_at_end = [], 0, None
    for k in range((N + K - 1) // K):
        active = np.flatnonzero(tile_spp > k * K).astype(np.uint32)
        if active.size == 0:
            break
        count = min(K, N - k * K)
        replay_stats.append(r.render_tiles_into(active, ra, rb, spp_count=count, spp_begin=k * K))
        passes += 1
        nxt = np.flatnonzero(tile_spp > (k + 1) * K).astype(np.uint32)
        if k == 0:
            assert nxt.tolist() == active.tolist()      # the first pass is not evaluated: nothing retires
            continue
        # (b) what retires after pass k + 1: denoise_var of the whole frame as replayed so far, its tile errors, the rule
        te = r.denoised_tile_errors(*filtered(ra, rb)).cpu().numpy().reshape(-1)
        print(f"[denoised loop] {engine}: after pass {k + 1} tile errors {' '.join(f'{v:.4f}' for v in te)}")
        stay = ar.select(te, E, active)
        if k * K + count < N:
            assert nxt.tolist() == stay.tolist(), (k, te.tolist())
        active_at_end = stay
    # (a) the frames are the sum of the replayed passes
    assert torch.equal(a, ra) and torch.equal(b, rb)
    # (c) the outputs are denoise_var of the final frames
    want = filtered(a, b)
    assert torch.equal(rgb, want[0]) and torch.equal(var, want[1]) and torch.equal(wsum, want[2])
    # (d) the summary
    assert summary["passes"] == passes
    pixels = ar.tile_pixels(width, height).reshape(-1)
    assert stats["n_camera_samples"] == int((tile_spp * pixels).sum())
    assert all(stats[key] == sum(s[key] for s in replay_stats) for key in ("n_camera_samples", "n_closest_rays", "n_shadow_rays"))
    assert (summary["spp_min"], summary["spp_max"]) == (int(tile_spp.min()), int(tile_spp.max()))
    assert summary["n_unconverged"] == active_at_end.size
    h_rgb, h_var, h_wsum = (t.cpu().numpy() for t in (rgb, var, wsum))
    err, empty = de.pixel_error(h_rgb, h_var, h_wsum)
    want_s = de.summary(err, empty, E)
    assert {key: summary["frame"][key] for key in want_s} == want_s and summary["frame"]["threshold"] == float(F(E))
    derr, dsum = r.denoised_error_map(rgb, var, wsum, threshold=E)
    assert dsum == summary["frame"] and derr.cpu().numpy().tobytes() == err.tobytes()
    # the conditions: tiles retired in at least two different passes, at least one was still active at the budget, not all were
    retired_at = set(tile_spp[tile_spp < N].tolist())
    assert len(retired_at) >= 2, tile_spp.tolist()
    assert 2 * K in retired_at                              # the wall's tiles: retired at the first evaluation
    assert summary["n_unconverged"] >= 1 and (tile_spp == N).any() and not (tile_spp == N).all()
    # the host twin returns the same frames, outputs, map and counts
    hf = {name: t.cpu().numpy() for name, t in fd.items()}
    tw = r.render_adaptive_denoised_host(E, **hf, pass_spp=K, spp_count=N)
    assert np.array_equal(tw["rgbw"], a.cpu().numpy()) and np.array_equal(tw["m2"], b.cpu().numpy())
    assert tw["rgb"].tobytes() == h_rgb.tobytes() and tw["var"].tobytes() == h_var.tobytes() and tw["wsum"].tobytes() == h_wsum.tobytes()
    assert tw["err"].tobytes() == err.tobytes() and tw["tile_spp"].reshape(-1).tolist() == tile_spp.tolist() and tw["summary"] == summary


# ------------------------------------------------------------------ 5. limits of the loop
@pytest.mark.parametrize("engine", ENGINES)
def test_limits_of_the_loop(renderer_factory, engine):
    import torch
    K, N = 3, 11
    r = renderer_factory(film_cases.cornell(W, H, N, RFilter("gaussian")))
    r.set_option("engine", engine)
    zeros = lambda: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    fd = {n: zeros() for n in NAMES}
    r.render_features_into(**fd, spp_count=N)

    def final(x, y, **params):
        out = (torch.empty((H, W, 3), device="cuda:0"), torch.empty((H, W, 3), device="cuda:0"), torch.empty((H, W), device="cuda:0"))
        r.denoise_var_into(out[0], out[1], x, y, wsum=out[2], **fd, **params)
        return out

    def same(got, want):
        return all(torch.equal(g, w) for g, w in zip(got, want))

    # target 0 never retires a tile with an error: the budget everywhere, the frames of the raw loop at target 0
    a, b = zeros(), zeros()
    rgb, var, wsum, tile_spp, summary, st = r.render_adaptive_denoised(a, b, 0.0, **fd, pass_spp=K, spp_count=N)
    c, d = zeros(), zeros()
    _, _, ust = r.render_adaptive(c, d, 0.0, pass_spp=K, spp_count=N)
    assert torch.equal(a, c) and torch.equal(b, d) and (tile_spp == N).all()
    assert summary["passes"] == 4 and summary["n_unconverged"] == 9 and st["n_camera_samples"] == ust["n_camera_samples"] == W * H * N
    assert same((rgb, var, wsum), final(a, b))
    # a target above every tile error: two passes, then every tile retires
    a, b = zeros(), zeros()
    rgb, var, wsum, tile_spp, summary, st = r.render_adaptive_denoised(a, b, 1e9, **fd, pass_spp=K, spp_count=N, radius=3, patch=2)
    assert (tile_spp == 2 * K).all() and summary["passes"] == 2 and summary["n_unconverged"] == 0 and summary["frame"]["n_above"] == 0
    assert (summary["spp_min"], summary["spp_max"]) == (2 * K, 2 * K) and st["n_camera_samples"] == W * H * 2 * K
    e, f = zeros(), zeros()
    r.render_moments_into(e, f, spp_count=K)
    r.render_moments_into(e, f, spp_count=K, spp_begin=K)
    assert torch.equal(a, e) and torch.equal(b, f) and same((rgb, var, wsum), final(a, b, radius=3, patch=2))
    # a budget of one pass: no evaluation, the outputs are still the final denoise and the summary describes them
    a, b = zeros(), zeros()
    rgb, var, wsum, tile_spp, summary, st = r.render_adaptive_denoised(a, b, 0.01, **fd, pass_spp=8, spp_count=5)
    assert (tile_spp == 5).all() and summary["passes"] == 1 and summary["frame"]["n_pixels"] == W * H
    assert same((rgb, var, wsum), final(a, b))
    te = r.denoised_tile_errors(rgb, var, wsum).cpu().numpy().reshape(-1)
    with np.errstate(invalid="ignore"):
        assert summary["n_unconverged"] == int((~(te <= F(0.01))).sum()) > 0
    # without feature frames
    a, b = zeros(), zeros()
    rgb, var, wsum, tile_spp, summary, st = r.render_adaptive_denoised(a, b, 1e9, pass_spp=K, spp_count=N)
    out = (torch.empty((H, W, 3), device="cuda:0"), torch.empty((H, W, 3), device="cuda:0"), torch.empty((H, W), device="cuda:0"))
    r.denoise_var_into(out[0], out[1], a, b, wsum=out[2])
    assert same((rgb, var, wsum), out) and summary["passes"] == 2
    # refusals, with the codes of the existing loop
    for bad in (dict(pass_spp=0), dict(pass_spp=2, target=-0.5), dict(pass_spp=2, target=float("nan")), dict(pass_spp=2, tile_mod=2), dict(pass_spp=2, radius=9)):
        with pytest.raises(NoriError, match="INVALID_ARGUMENT"):
            r.render_adaptive_denoised(zeros(), zeros(), bad.get("target", 0.1), spp_count=4, **{k: v for k, v in bad.items() if k != "target"})
    with pytest.raises(NoriError, match=r"NORI_ERR_UNSUPPORTED: \S+"):
        r.render_adaptive_denoised(zeros(), zeros(), 0.1, pass_spp=2, spp_count=4, seed_mode=_capi.SEED_NORI_BLOCK)
    r.set_option("film_order", "reference")
    with pytest.raises(NoriError, match=r"NORI_ERR_UNSUPPORTED: \S+"):
        r.render_adaptive_denoised(zeros(), zeros(), 0.1, pass_spp=2, spp_count=4)
    r.set_option("film_order", "fast")
    a, b = zeros(), zeros()
    assert r.render_adaptive_denoised(a, b, 1e9, **fd, pass_spp=K, spp_count=N)[4]["passes"] == 2      # the context still renders


# ------------------------------------------------------------------ 6. isolation
def test_other_calls_give_the_same_bytes_before_and_after(renderer_factory):
    r, rgbw, m2, feats = rendered(renderer_factory)

    def others():
        plain, _ = r.render_host(spp_count=8)
        den = r.denoise_host(rgbw, m2, **feats)
        ad = r.render_adaptive_host(0.2, pass_spp=4, spp_count=12)
        return [plain, den[0], den[1], ad[0], ad[1], ad[2], ad[3]], ad[4]

    before, s_before = others()
    tw = r.render_adaptive_denoised_host(0.03, **feats, pass_spp=4, spp_count=12)
    assert tw["summary"]["passes"] >= 2
    after, s_after = others()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after)) and s_before == s_after
    again = r.render_adaptive_denoised_host(0.03, **feats, pass_spp=4, spp_count=12)
    assert all(again[k].tobytes() == tw[k].tobytes() for k in ("rgbw", "m2", "rgb", "var", "wsum", "err", "tile_spp")) and again["summary"] == tw["summary"]


# ------------------------------------------------------------------ 7. the command line
def test_cli_target_denoised_error(renderer_factory, tmp_path):
    (tmp_path / "floor.obj").write_text("v -3 0 -3\nv -3 0 3\nv 3 0 3\nv 3 0 -3\nf 1 2 3 4\n")
    (tmp_path / "light.obj").write_text("v -0.5 2 -0.5\nv 0.5 2 -0.5\nv 0.5 2 0.5\nv -0.5 2 0.5\nf 1 2 3 4\n")
    (tmp_path / "s.xml").write_text("""<scene><integrator type="path_mis"/>
      <sampler type="independent"><integer name="sampleCount" value="12"/></sampler>
      <camera type="perspective"><integer name="width" value="40"/><integer name="height" value="24"/><float name="fov" value="50"/>
        <transform name="toWorld"><lookat target="0, 0.5, 0" origin="0, 1, 4" up="0, 1, 0"/></transform></camera>
      <mesh type="obj"><string name="filename" value="floor.obj"/><bsdf type="diffuse"><color name="albedo" value="0.6,0.5,0.4"/></bsdf></mesh>
      <mesh type="obj"><string name="filename" value="light.obj"/><emitter type="area"><color name="radiance" value="8,8,8"/></emitter></mesh>
    </scene>""")
    r = renderer_factory(host.load_xml(str(tmp_path / "s.xml")), builder=2)
    feats, _ = r.render_features_host(spp_count=5)
    E = 0.05
    want = r.render_adaptive_denoised_host(E, **feats, pass_spp=4, radius=3, patch=2)
    exe = os.path.join(_capi.LIB_DIR, "nori")
    p = subprocess.run([exe, str(tmp_path / "s.xml"), "--target-denoised-error", str(E), "--pass-spp", "4", "--feature-spp", "5", "--denoise-radius", "3",
                        "--denoise-patch", "2"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    s = want["summary"]
    assert f"stopped after {s['passes']} passes" in p.stdout and f"{s['n_unconverged']} of {s['n_tiles']} tiles above the target" in p.stdout, p.stdout
    assert "features of 5 samples per pixel" in p.stdout, p.stdout
    got = {name: read_exr_rgb(str(tmp_path / f"s.{name}.exr"))[1] for name in ("denoised", "error", "spp")}
    assert all(g.shape == (24, 40, 3) for g in got.values())
    assert np.array_equal(got["denoised"], want["rgb"])
    assert np.array_equal(got["error"][..., 0], want["err"])
    assert np.array_equal(got["spp"][..., 0], np.repeat(np.repeat(want["tile_spp"], 16, 0), 16, 1)[:24, :40].astype(F))
    from nori_amd.render import develop_host
    assert np.array_equal(read_exr_rgb(str(tmp_path / "s.exr"))[1], develop_host(want["rgbw"], r.border))      # the usual output: the raw frame
