"""The denoiser's output variance and the error of a denoised frame without a GPU: the restatement (tests/denoise_error_ref.py)
against a per-pixel loop and closed forms, its calibration on oracle renders, the resources of denoise_error.hip's kernels, the
bindings and the command line.

Calibration measured here (float32 restatement, 45 x 37, box filter, 16 spp against 2048 oracle spp of a disjoint range; mean
squared error / mean predicted variance, beside the same ratio of the raw frame and its plug-in variance):
    plain Cornell box   denoised 0.935   raw 0.823   median per-pixel ratio 0.841   predicted tile errors 0.059 .. 0.176
    textured scene_a    denoised 0.852   raw 0.835   median per-pixel ratio 0.944   predicted tile errors 0.058 .. 0.173"""
from __future__ import annotations

import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi
from nori_amd.scene import RFilter
from tests import denoise_error_ref as de, denoise_ref as dr, film_cases
from tests.backends import Oracle
from tests.test_denoise_cpu import filter_lds, oracle_frames, oracle_reference, random_guides
from tests.test_gpu_features import scene_a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ------------------------------------------------------------------ the restatement against a per-pixel loop
def loop_denoise_var(g, with_albedo, with_normal, with_depth, **params):
    """step B with the variance pixel by pixel, tap by tap in Python scalars of float32: (rgb, var, wsum)"""
    p = {**dr.DEFAULTS, **params}
    R, Fp = p["radius"], p["patch"]
    alpha, kc2, kd2 = F(p["alpha"]), F(p["k_c"]) * F(p["k_c"]), F(p["k_depth"]) * F(p["k_depth"])
    h, w = g.shape[:2]
    inside = lambda x, y: 0 <= x < w and 0 <= y < h and g[y, x, 14] != 0
    taps = []      # (y, x, qy, qx, e)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if not inside(x, y):
                    continue
                for dy in range(-R, R + 1):
                    for dx in range(-R, R + 1):
                        qx, qy = x + dx, y + dy
                        if not inside(qx, qy):
                            continue
                        acc, cnt = F(0), 0
                        for oy in range(-Fp, Fp + 1):
                            for ox in range(-Fp, Fp + 1):
                                if not (inside(x + ox, y + oy) and inside(qx + ox, qy + oy)):
                                    continue
                                a, b = g[y + oy, x + ox], g[qy + oy, qx + ox]
                                delta = F(0)
                                for c in range(3):
                                    t = F(a[c] - b[c])
                                    nume = F(F(t * t) - F(alpha * F(a[3 + c] + min(b[3 + c], a[3 + c]))))
                                    deno = F(F(1e-10) + F(kc2 * F(a[3 + c] + b[3 + c])))
                                    delta = F(delta + F(nume / deno))
                                acc = F(acc + delta)
                                cnt += 1
                        d = F(acc / F(F(3) * F(cnt)))
                        e = d if d > 0 else F(0)
                        a, b = g[y, x], g[qy, qx]
                        if with_albedo:
                            s = F(0)
                            for c in range(6, 9):
                                t = F(a[c] - b[c]); s = F(s + F(t * t))
                            e = F(e + F(s / F(p["tau_albedo"])))
                        if with_normal:
                            s = F(0)
                            for c in range(9, 12):
                                t = F(a[c] - b[c]); s = F(s + F(t * t))
                            e = F(e + F(s / F(p["tau_normal"])))
                        if with_depth:
                            t = F(a[12] - b[12])
                            gg = F(F(kd2 * F(F(a[12] * a[12]) + F(b[12] * b[12]))) + F(1e-12))
                            e = F(e + F(F(t * t) / gg))
                            u = F(a[13] - b[13])
                            e = F(e + F(F(u * u) / F(p["tau_cov"])))
                        taps.append((y, x, qy, qx, e))
    e = np.asarray([t[4] for t in taps], F)
    wgt = np.zeros(len(taps), F)
    keep = e <= F(87)
    wgt[keep] = Oracle.libm("exp", -e[keep])
    num, vnum, wsum = np.zeros((h, w, 3), F), np.zeros((h, w, 3), F), np.zeros((h, w), F)
    for (y, x, qy, qx, _), wt in zip(taps, wgt):
        for c in range(3):
            num[y, x, c] = F(num[y, x, c] + F(wt * g[qy, qx, c]))
        wsum[y, x] = F(wsum[y, x] + wt)
        ww = F(wt * wt)
        for c in range(3):
            vnum[y, x, c] = F(vnum[y, x, c] + F(ww * g[qy, qx, 3 + c]))
    valid = g[..., 14] != 0
    with np.errstate(all="ignore"):
        rgb = np.where(valid[..., None], num / wsum[..., None], F(0)).astype(F)
        var = np.where(valid[..., None], ((vnum / wsum[..., None]).astype(F) / wsum[..., None]).astype(F), F(0)).astype(F)
    return rgb, var, wsum


@pytest.mark.parametrize("h,w,params", [(3, 5, dict(radius=8, patch=2)), (6, 7, dict()), (6, 7, dict(radius=2, patch=0, alpha=0.0))])
def test_shifted_arrays_equal_the_pixel_loop(h, w, params):
    g, _ = random_guides(h, w, 3, empty=[(1, 2)])
    for terms in ((True, True, True), (False, False, False), (True, False, False), (False, False, True)):
        rgb, var, wsum = de.denoise_var(g, *terms, **params)
        lrgb, lvar, lwsum = loop_denoise_var(g, *terms, **params)
        assert np.array_equal(rgb, lrgb) and np.array_equal(var, lvar) and np.array_equal(wsum, lwsum), (terms, params)
        want, want_w = dr.denoise(g, *terms, **params)      # the three accumulators change nothing of the filter's own outputs
        assert rgb.tobytes() == want.tobytes() and wsum.tobytes() == want_w.tobytes()
        assert (var[1, 2] == 0).all() and (rgb[1, 2] == 0).all() and wsum[1, 2] == 0
        live = g[..., 14] != 0
        assert (var[live] > 0).all() and np.isfinite(var).all()
        assert (var[live] <= g[..., 3:6].max()).all()      # a convex combination of squares of weights: never above the largest input


# ------------------------------------------------------------------ hand cases with exact answers
def hand_guides(h, w, mean, var):
    g = np.zeros((h, w, 16), F)
    g[..., 0:3] = np.asarray(mean, F)
    g[..., 3:6] = np.asarray(var, F)
    g[..., 14] = 1
    return g


def test_a_lone_valid_pixel_keeps_its_variance():
    g = hand_guides(5, 6, (0.3, 0.7, 1.1), (0.013, 0.37, 2.9))
    g[..., 14] = 0
    g[2, 3, 14] = 1
    for params in (dict(), dict(radius=8, patch=2), dict(radius=1, patch=0)):
        rgb, var, wsum = de.denoise_var(g, False, False, False, **params)
        assert var[2, 3].tobytes() == g[2, 3, 3:6].tobytes() and wsum[2, 3] == 1 and rgb[2, 3].tobytes() == g[2, 3, 0:3].tobytes()
        others = np.ones((5, 6), bool); others[2, 3] = False
        assert not var[others].any() and not rgb[others].any() and not wsum[others].any()


def test_constant_frame_divides_the_variance_by_the_clipped_window():
    """alpha = 0 and equal means: every delta is 0 and every weight exp(-0) = 1, so wsum = N, vnum = N var exactly (var a power of
    two, N <= 289) and var_out = (N var / N) / N = var / N, one rounded division"""
    var = np.asarray((2.0 ** -3, 2.0 ** -10, 2.0 ** 4), F)
    g = hand_guides(7, 20, (0.375, 0.375, 0.375), var)
    y, x = np.arange(7), np.arange(20)
    for R in (1, 5, 8):
        rgb, vout, wsum = de.denoise_var(g, False, False, False, radius=R, alpha=0.0)
        ny = np.minimum(y + R, 6) - np.maximum(y - R, 0) + 1
        nx = np.minimum(x + R, 19) - np.maximum(x - R, 0) + 1
        n = (ny[:, None] * nx[None, :]).astype(F)
        assert np.array_equal(wsum, n), R
        assert np.array_equal(vout, (var[None, None, :] / n[..., None]).astype(F)), R
        assert np.array_equal(rgb, g[..., :3]), R


def test_an_invalid_pixel_gives_zeros_and_counts_as_empty():
    g = hand_guides(6, 6, (0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
    g[2, 3, 14] = 0
    g[2, 3, :6] = 0
    rgb, var, wsum = de.denoise_var(g, False, False, False, radius=8, alpha=0.0)
    assert not rgb[2, 3].any() and not var[2, 3].any() and wsum[2, 3] == 0
    err, empty = de.pixel_error(rgb, var, wsum)
    assert err[2, 3] == 0 and empty[2, 3] and empty.sum() == 1
    live = ~empty
    assert (wsum[live] == 35).all() and np.array_equal(var[live], np.full((35, 3), F(0.25) / F(35), F))
    # the error of the others: 3 sqrt(var / 35) / (1.5 + 0.03) in the stated float32 order
    s = np.sqrt(F(0.25) / F(35)).astype(F)
    want = F(F(F(s + s) + s) / F(F(1.5) + F(0.03)))
    assert (err[live] == want).all()
    summ = de.summary(err, empty, float(want))
    assert summ["n_empty"] == 1 and summ["n_above"] == 0 and summ["n_pixels"] == 36 and summ["max_err"] == float(want)
    assert de.summary(err, empty, 0.0)["n_above"] == 35
    assert np.isclose(summ["sum_err"], 35 * float(want), rtol=1e-12)


def test_pixel_error_has_the_form_of_the_raw_error():
    """a pixel filtered with itself alone (wsum = 1, rgb = mu, var = the variance of the mean) has the raw pixel's error, bit for bit"""
    from tests import moments_ref as mr
    rgbw, m2 = mr.hand_made_pair(border=0)
    g = dr.guides(rgbw, m2)
    err, empty = de.pixel_error(g[..., 0:3], g[..., 3:6], g[..., 14])
    want, want_empty = mr.error_map(rgbw, m2, 0)
    assert err.tobytes() == want.tobytes() and np.array_equal(empty, want_empty) and empty.sum() == 3


def test_tile_errors_and_summary_follow_the_fixed_orders():
    rng = np.random.default_rng(11)
    h, w = 37, 45
    rgb = rng.uniform(0.0, 2.0, (h, w, 3)).astype(F)
    var = (10.0 ** rng.uniform(-6, 0, (h, w, 3))).astype(F)
    wsum = rng.uniform(1.0, 100.0, (h, w)).astype(F)
    wsum[rng.uniform(size=(h, w)) < 0.05] = 0
    wsum[16:32, 16:32] = 0      # a whole tile of empty pixels
    err, empty = de.pixel_error(rgb, var, wsum)
    te = de.tile_errors(rgb, var, wsum)
    assert te.shape == (3, 3) and te.dtype == F and te[1, 1] == 0 and np.count_nonzero(te) == 8
    # tile (2, 2) is 13 x 5 pixels: the mean over the pixels inside the frame, within the rounding of 65 binary64 additions and one float32 rounding
    assert np.isclose(te[2, 2], err[32:, 32:].astype(np.float64).mean(), rtol=2.0 ** -23)
    s = de.summary(err, empty, 0.1)
    assert np.isclose(s["sum_err"], err.astype(np.float64).sum(), rtol=1e-13) and s["n_empty"] == int(empty.sum())
    assert s["n_above"] == int((err > F(0.1)).sum()) and s["max_err"] == float(err.max()) and s["n_pixels"] == h * w
    # more than 256 workgroups: lanes own several partials
    big = rng.uniform(0.0, 1.0, (300, 300)).astype(F)
    sb = de.summary(big, np.zeros(big.shape, bool), 0.5)
    assert np.isclose(sb["sum_err"], big.astype(np.float64).sum(), rtol=1e-13) and sb["n_pixels"] == 90000


# ------------------------------------------------------------------ calibration on oracle frames
@pytest.mark.parametrize("name", ["plain", "textured"])
def test_the_predicted_variance_is_no_worse_calibrated_than_the_raw_one(name):
    """16 spp under the box filter against 2048 oracle spp of a disjoint range: mean squared error / mean predicted variance of the
    denoised frame lies inside [0.5 r, 2 r], r being the same ratio of the raw frame and its plug-in variance, the estimate the
    existing loop trusts.  The factor 2 is the room for a 1 665-pixel frame; a float64 prototype gave 0.93 against r = 0.82 on the
    plain box.  Measured with this float32 restatement: plain 0.935 (r = 0.823), textured 0.852 (r = 0.835)."""
    sc = film_cases.cornell(45, 37, 1, RFilter("box"), integrator="path_mis") if name == "plain" else scene_a("box")
    rgbw, m2, feats = oracle_frames(sc)
    ref = oracle_reference(sc).astype(np.float64)
    g = dr.guides(rgbw, m2, feats["albedo"], feats["normal"], feats["depth"], border=0)
    rgb, var, wsum = de.denoise_var(g)
    assert np.isfinite(var).all() and (var >= 0).all() and (wsum >= 1).all()
    raw = g[..., 0:3].astype(np.float64)
    r = ((raw - ref) ** 2).mean() / g[..., 3:6].astype(np.float64).mean()
    ratio = ((rgb.astype(np.float64) - ref) ** 2).mean() / var.astype(np.float64).mean()
    per_pixel = ((rgb.astype(np.float64) - ref) ** 2).sum(-1) / np.maximum(var.astype(np.float64).sum(-1), 1e-30)
    te = de.tile_errors(rgb, var, wsum)
    print(f"{name}: denoised mse / predicted variance {ratio:.3f}; raw mse / plug-in variance {r:.3f}; median per-pixel ratio {np.median(per_pixel):.3f}; "
          f"predicted tile errors {te.min():.3f} .. {te.max():.3f}")
    assert 0.5 * r <= ratio <= 2.0 * r, (ratio, r)


# ------------------------------------------------------------------ the loop's target, from oracle frames
def test_the_loop_target_splits_the_tiles_on_oracle_frames():
    """Where tests/test_gpu_denoise_error.py::test_the_loop_is_its_replay has its target from: the loop replayed in numpy
    (denoise_error_ref.replay_loop) on 48 one-sample oracle renders of its scene under the box filter and the restated feature
    samples.  The target must split the tiles -- several retirement passes, some tiles at the budget -- with room on either side."""
    from tests import adaptive_ref as ar, features_ref as fr
    from tests.test_gpu_adaptive import wall_and_cornell
    from tests.test_gpu_denoise_error import LOOP_E, LOOP_FEATURE_SPP, LOOP_K, LOOP_N
    w, h = 72, 40
    sc = wall_and_cornell(w, h, LOOP_N, RFilter("box"))
    o = Oracle(sc, use_bvh=True)
    L = np.stack([o.render_host(spp_count=1, spp_begin=s)[0] for s in range(LOOP_N)])
    _, vals = fr.job_samples(sc, 0, LOOP_FEATURE_SPP, o)
    o.close()
    feats = {}
    for n in fr.NAMES:
        frame = np.zeros((h, w, 4), F)
        for v in vals[n].reshape(LOOP_FEATURE_SPP, h, w, 3):
            frame[..., :3] += v
        frame[..., 3] = F(LOOP_FEATURE_SPP)
        feats[n] = frame
    ys, xs = np.mgrid[0:h, 0:w]
    tile_of = (ys // 16) * ar.tile_grid(w, h)[1] + xs // 16
    rgbw, m2 = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)

    def render_pass(k, active, count):
        m = np.isin(tile_of, active)
        for s in range(k * LOOP_K, k * LOOP_K + count):
            f = L[s] * m[..., None]
            rgbw[...] += f
            m2[..., :3] += (f[..., :3] * f[..., :3]).astype(F)
            m2[..., 3] += m.astype(F)

    filtered = lambda: de.denoise_var_frames(rgbw, m2, feats["albedo"], feats["normal"], feats["depth"], border=0)
    tile_spp, active, passes, log = de.replay_loop(render_pass, 15, filtered, LOOP_E, LOOP_K, LOOP_N)
    for k, te, stay in log:
        print(f"after pass {k + 1}: {' '.join(f'{v:.4f}' for v in te)} -> stay {stay.tolist()}")
    assert tile_spp.tolist() == [16, 40, 16, 16, 16, 16, 48, 16, 16, 16, 24, 48, 16, 16, 16] and passes == 6 and active.tolist() == [6, 11]
    # no error that decided anything lies within 1.5 % of the target: the GPU's frames differ from these by the order of float32 sums
    decided = np.concatenate([te[before] for (_, te, _), before in zip(log, [np.arange(15)] + [stay for _, _, stay in log[:-1]])])
    assert (np.abs(decided - F(LOOP_E)) > 0.015 * LOOP_E).all(), np.sort(np.abs(decided - F(LOOP_E)))[:3]


# ------------------------------------------------------------------ the new device source
@pytest.fixture(scope="module")
def error_kernels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as ge
    from kernel_resources import kernels
    assert "denoise_error.hip" in ge.HIP_SOURCES
    res = {}
    for tag, extra in (("product", []), ("count", ["-DNORI_COUNT_EXCURSIONS=1"])):
        out = tmp_path_factory.mktemp("asm") / f"denoise_error_{tag}.s"
        flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")] + extra
        p = subprocess.run([ge.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(ge.DEV, "denoise_error.hip"), "-o", str(out)],
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        res[tag] = {r["demangled"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: r for r in kernels(str(out))}
    return res


def test_error_kernels_fit_their_budget(error_kernels):
    want = {f"denoise_filter_var_kernel<{f}, {r}>": filter_lds(f, r) for f in (0, 1, 2) for r in (5, 8)}
    # the map and its reduction: 256 x (double + float + 2 x uint64); the tile means: 256 doubles
    want.update({"denoise_error_map_kernel": 256 * 28, "denoise_error_reduce_kernel": 256 * 28, "denoise_tile_errors_kernel": 256 * 8})
    for tag, ks in error_kernels.items():
        assert set(ks) == set(want), (tag, sorted(ks))
        for name, k in ks.items():
            assert k["scratch"] == 0 and k["vgpr"] <= 128, (tag, name, k)
            assert k["lds"] == want[name] <= 65536, (tag, name, k)
        assert ks["denoise_filter_var_kernel<1, 5>"]["lds"] == 33472 and ks["denoise_filter_var_kernel<2, 8>"]["lds"] == 49088


# ------------------------------------------------------------------ bindings, command line
NEW = ("nori_hip_denoise_var", "nori_hip_denoise_var_host", "nori_hip_denoised_error_map", "nori_hip_denoised_error_map_host",
       "nori_hip_denoised_tile_errors", "nori_hip_denoised_tile_errors_host", "nori_hip_render_adaptive_denoised", "nori_hip_render_adaptive_denoised_host")


def test_capi_declares_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "nori_hip.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*|nori_hip_ctx \*)\s*(nori_hip_\w+)\(", header, re.M))
    lib = _capi.load_hip()
    for name in NEW:
        assert name in declared and name in _capi.HIP_PROTOTYPES and hasattr(lib, name), name
    assert declared <= set(_capi.HIP_PROTOTYPES)
    for name in declared:
        assert hasattr(lib, name), name
    assert _capi.HIP_ABI_VERSION == 8 and "#define NORI_HIP_ABI_VERSION 8 " in header
    # the prototypes have the arity of the declarations
    for name in NEW:
        decl = re.search(r"^int " + name + r"\((.*?)\);", header, re.M | re.S).group(1)
        n_args = len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(","))
        assert n_args == len(_capi.HIP_PROTOTYPES[name][1]), (name, n_args)
    from nori_amd.render import Renderer
    for name in ("denoise_var_into", "denoise_var_host", "denoised_error_map", "denoised_tile_errors", "render_adaptive_denoised", "render_adaptive_denoised_host"):
        assert callable(getattr(Renderer, name)), name


def test_cli_rejects_the_new_flag_with_other_loops_and_bad_values(tmp_path):
    """before anything is loaded or a device is asked for: the scene file does not even exist"""
    exe = os.path.join(_capi.LIB_DIR, "nori")
    scene = str(tmp_path / "missing.xml")
    flag = "--target-denoised-error"
    for args, words in (([flag, "0.02", "--denoise"], (flag, "--denoise")),
                        ([flag, "0.02", "--target-error", "0.05"], (flag, "--target-error")),
                        (["--target-error", "0.05", "--adaptive", flag, "0.02"], (flag,)),
                        ([flag, "0.02", "--adaptive"], (flag, "--adaptive")),
                        ([flag, "0.02", "--gpus", "2"], (flag, "one device")),
                        (["--gpus", "3", flag, "0.02"], (flag, "one device")),
                        ([flag, "-0.5"], (flag, ">= 0")), ([flag, "nan"], (flag, ">= 0")), ([flag, "inf"], (flag, ">= 0")),
                        ([flag, "abc"], (flag, ">= 0")), ([flag, "0.1x"], (flag, ">= 0")), ([flag], (flag, ">= 0")),
                        ([flag, "0.02", "--denoise-radius", "9"], ("1 .. 8",)),
                        ([flag, "0.02", "--denoise-patch", "3"], ("0 .. 2",)),
                        ([flag, "0.02", "--pass-spp", "0"], ("--pass-spp",)),
                        # every existing rejection keeps its text
                        (["--pass-spp", "4"], ("\"--pass-spp\" goes with --target-error E.",)),
                        (["--adaptive"], ("\"--adaptive\" goes with --target-error E.",)),
                        (["--feature-spp", "4"], ("\"--feature-spp\" goes with --features (or --denoise).",)),
                        (["--denoise-radius", "3"], ("\"--denoise-radius\" goes with --denoise.",)),
                        (["--denoise", "--target-error", "0.05"], ("\"--denoise\" renders the scene's sample count and does not go with --target-error.",))):
        p = subprocess.run([exe, scene] + args, capture_output=True, text=True, timeout=120)
        out = p.stdout + p.stderr
        assert p.returncode != 0 and "Usage" in out and "missing.xml" not in out, (args, out)
        for word in words:
            assert word in out, (args, out)
    # the flag with its companions is accepted: the scene is then opened, and is missing
    p = subprocess.run([exe, scene, flag, "0.02", "--pass-spp", "4", "--feature-spp", "3", "--denoise-radius", "3", "--denoise-patch", "2"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "Usage" not in p.stdout + p.stderr and "missing.xml" in p.stdout + p.stderr
