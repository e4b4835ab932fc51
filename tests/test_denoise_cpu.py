"""The denoiser without a GPU: what the stated operation (tests/denoise_ref.py) does to oracle renders, hand cases against closed
forms and against a per-pixel loop, the resources of denoise.hip's kernels, the bindings and the command line.

Known limit, stated rather than tested: at 4-8 samples per pixel the variance estimates are too noisy (a float32 prototype of
this operation gave a trimmed error ratio of 0.69 at 8 spp and above 1 at 4 spp); fireflies pass through unchanged."""
from __future__ import annotations

import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi
from nori_amd.scene import RFilter
from tests import denoise_ref as dr, features_ref as fr, film_cases
from tests.backends import Oracle
from tests.test_gpu_features import scene_a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
W, H = 45, 37
SPP = 16


# ------------------------------------------------------------------ quality of the stated operation
def oracle_frames(sc, spp=SPP):
    """(rgbw, m2, {albedo, normal, depth}) of `spp` one-sample oracle renders under the box filter (W = 1 per sample) and of the
    restated feature samples averaged per pixel; float32 sums in sample order"""
    h, w = sc.camera.height, sc.camera.width
    o = Oracle(sc, use_bvh=True)
    rgbw, m2 = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    for s in range(spp):
        f, _ = o.render_host(spp_count=1, spp_begin=s)
        assert f.shape == (h, w, 4) and (f[..., 3] == 1).all()
        rgbw += f
        m2[..., :3] += (f[..., :3] * f[..., :3]).astype(F)
        m2[..., 3] += F(1)
    _, vals = fr.job_samples(sc, 0, spp, o)
    o.close()
    feats = {}
    for n in fr.NAMES:
        v = vals[n].reshape(spp, h, w, 3)
        frame = np.zeros((h, w, 4), F)
        for s in range(spp):
            frame[..., :3] += v[s]
        frame[..., 3] = F(spp)
        feats[n] = frame
    return rgbw, m2, feats


def oracle_reference(sc, spp=2048, begin=100000):
    o = Oracle(sc, use_bvh=True)
    f, _ = o.render_host(spp_count=spp, spp_begin=begin)
    o.close()
    return (f[..., :3] / f[..., 3:4]).astype(F)


@pytest.mark.parametrize("name", ["plain", "textured"])
def test_the_stated_operation_halves_the_error_at_16_spp(name):
    """denoised / noisy <= 0.5 in the trimmed relative squared error against 2048 spp of a disjoint sample range.  A float32
    prototype of this operation gave 0.31 (plain box) and 0.30 (textured box) against 8192 spp; 0.5 leaves room for the
    reference's own noise (about 0.01 of the ratio) and for the bits of exp."""
    sc = film_cases.cornell(W, H, 1, RFilter("box"), integrator="path_mis") if name == "plain" else scene_a("box")
    rgbw, m2, feats = oracle_frames(sc)
    ref = oracle_reference(sc)
    rgb, wsum = dr.denoise_frames(rgbw, m2, feats["albedo"], feats["normal"], feats["depth"], border=0)
    noisy = (rgbw[..., :3] / rgbw[..., 3:4]).astype(F)
    e_noisy, e_den = dr.trimmed_error(noisy, ref), dr.trimmed_error(rgb, ref)
    print(f"{name}: noisy {e_noisy:.5f} denoised {e_den:.5f} ratio {e_den / e_noisy:.3f}")
    assert np.isfinite(rgb).all() and np.isfinite(wsum).all()
    assert (wsum >= 1).all()
    assert e_den / e_noisy <= 0.5, (e_noisy, e_den)


# ------------------------------------------------------------------ hand cases
def frames_of(mean, var_scale, n=16.0):
    """(rgbw, m2) whose pixels have mean `mean` (h, w, 3) and E[L^2] = mean^2 (1 + var_scale); W = n, sum w^2 = n"""
    mean = np.asarray(mean, F)
    h, w = mean.shape[:2]
    rgbw = np.concatenate([mean * F(n), np.full((h, w, 1), n, F)], -1).astype(F)
    m2 = np.concatenate([mean * mean * F(1 + var_scale) * F(n), np.full((h, w, 1), n, F)], -1).astype(F)
    return rgbw, m2


def loop_denoise(g, with_albedo, with_normal, with_depth, **params):
    """step B pixel by pixel, tap by tap, offset by offset in Python scalars of float32: what denoise_ref's shifted arrays must equal"""
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
    num, wsum = np.zeros((h, w, 3), F), np.zeros((h, w), F)
    for (y, x, qy, qx, _), wt in zip(taps, wgt):
        for c in range(3):
            num[y, x, c] = F(num[y, x, c] + F(wt * g[qy, qx, c]))
        wsum[y, x] = F(wsum[y, x] + wt)
    valid = g[..., 14] != 0
    with np.errstate(all="ignore"):
        return np.where(valid[..., None], num / wsum[..., None], F(0)).astype(F), wsum


def random_guides(h, w, seed, empty=()):
    rng = np.random.default_rng(seed)
    mean = rng.uniform(0.05, 2.0, (h, w, 3)).astype(F)
    rgbw, m2 = frames_of(mean, 0.5)
    feats = []
    for k in range(3):
        f = rng.uniform(0.0, 1.0, (h, w, 4)).astype(F)
        f[..., 3] = F(16)
        f[..., :3] *= F(16)
        feats.append(f)
    feats[2][..., 2] = np.minimum(feats[2][..., 2], F(16))
    for (y, x) in empty:
        rgbw[y, x] = 0
    return dr.guides(rgbw, m2, *feats), (rgbw, m2, feats)


@pytest.mark.parametrize("h,w,params", [(3, 5, dict(radius=8, patch=2)), (6, 7, dict()), (6, 7, dict(radius=2, patch=0, alpha=0.0))])
def test_shifted_arrays_equal_the_pixel_loop(h, w, params):
    g, _ = random_guides(h, w, 3, empty=[(1, 2)])
    for terms in ((True, True, True), (False, False, False), (True, False, False), (False, False, True)):
        a, wa = dr.denoise(g, *terms, **params)
        b, wb = loop_denoise(g, *terms, **params)
        assert np.array_equal(a, b) and np.array_equal(wa, wb), (terms, params)
        assert (a[1, 2] == 0).all() and wa[1, 2] == 0


def test_two_flat_halves_keep_their_bits():
    """var = 0 and colours of few mantissa bits: inside a half every weight is 1 and the sums are exact, across the edge
    t^2 / 1e-10 is far above the cut-off and the weight 0"""
    mean = np.zeros((9, 14, 3), F)
    mean[:, :7] = (0.25, 0.5, 0.75)
    mean[:, 7:] = (2.0, 1.0, 3.0)
    rgbw, m2 = frames_of(mean, 0.0)
    g = dr.guides(rgbw, m2)
    assert (g[..., 3:6] == 0).all() and (g[..., 14] == 1).all()
    rgb, wsum = dr.denoise(g, False, False, False)
    assert np.array_equal(rgb, mean) and (wsum >= 1).all()
    # without a patch (F = 0) a pixel's weights are exactly the pixels of its own half inside the window; with one, the pixels
    # next to the edge lose the taps whose patch straddles it
    rgb, wsum = dr.denoise(g, False, False, False, patch=0)
    assert np.array_equal(rgb, mean)
    x = np.arange(14)
    in_half = np.where(x < 7, np.minimum(x + 5, 6) - np.maximum(x - 5, 0) + 1, np.minimum(x + 5, 13) - np.maximum(x - 5, 7) + 1)
    y = np.arange(9)
    rows = np.minimum(y + 5, 8) - np.maximum(y - 5, 0) + 1
    assert np.array_equal(wsum, (rows[:, None] * in_half[None, :]).astype(F))


def test_constant_frame_counts_the_clipped_window():
    mean = np.full((7, 20, 3), 0.375, F)
    rgbw, m2 = frames_of(mean, 0.8)
    g = dr.guides(rgbw, m2)
    assert (g[..., 3:6] > 0).all()
    for R in (1, 5, 8):
        rgb, wsum = dr.denoise(g, False, False, False, radius=R, alpha=0.0)
        y, x = np.arange(7), np.arange(20)
        ny = np.minimum(y + R, 6) - np.maximum(y - R, 0) + 1
        nx = np.minimum(x + R, 19) - np.maximum(x - R, 0) + 1
        assert np.array_equal(wsum, (ny[:, None] * nx[None, :]).astype(F)), R
        assert np.array_equal(rgb, g[..., :3]), R


def test_empty_pixels_give_zero_and_are_skipped_as_taps():
    mean = np.full((6, 6, 3), 0.5, F)
    rgbw, m2 = frames_of(mean, 0.8)
    rgbw[2, 3] = 0
    rgbw[0, 0, 3] = F(-1)
    g = dr.guides(rgbw, m2)
    assert g[2, 3, 14] == 0 and g[0, 0, 14] == 0 and (g[2, 3, :6] == 0).all() and (g[0, 0, :6] == 0).all()
    rgb, wsum = dr.denoise(g, False, False, False, radius=8, alpha=0.0)
    assert (rgb[2, 3] == 0).all() and wsum[2, 3] == 0 and (rgb[0, 0] == 0).all() and wsum[0, 0] == 0
    live = g[..., 14] != 0
    assert (wsum[live] == 34).all() and np.array_equal(rgb[live], g[..., :3][live])      # the 36 pixels but the two empty ones


def test_guides_follow_the_decode():
    g, (rgbw, m2, feats) = random_guides(4, 5, 9)
    dec = fr.decode(dict(zip(fr.NAMES, feats)), 0)
    assert np.array_equal(g[..., 6:9], dec["albedo"]) and np.array_equal(g[..., 9:12], dec["normal"])
    assert np.array_equal(g[..., 12], dec["depth"][..., 0]) and np.array_equal(g[..., 13], dec["depth"][..., 1])
    none = dr.guides(rgbw, m2)
    assert (none[..., 6:14] == 0).all() and np.array_equal(none[..., :6], g[..., :6]) and (g[..., 15] == 0).all()


# ------------------------------------------------------------------ the new device source
@pytest.fixture(scope="module")
def denoise_kernels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as ge
    from kernel_resources import kernels
    assert "denoise.hip" in ge.HIP_SOURCES
    res = {}
    for tag, extra in (("product", []), ("count", ["-DNORI_COUNT_EXCURSIONS=1"])):
        out = tmp_path_factory.mktemp("asm") / f"denoise_{tag}.s"
        flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")] + extra
        p = subprocess.run([ge.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(ge.DEV, "denoise.hip"), "-o", str(out)],
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        res[tag] = {r["demangled"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: r for r in kernels(str(out))}
    return res


def filter_lds(patch, rmax):
    """7 staged planes of the tile and a halo of rmax + patch, two delta planes of 40 float2 per row"""
    side = 16 + 2 * (rmax + patch)
    return 7 * side * side * 4 + 2 * 40 * (16 + 2 * patch) * 8


def test_denoise_kernels_fit_their_budget(denoise_kernels):
    want = {f"denoise_filter_kernel<{f}, {r}>": filter_lds(f, r) for f in (0, 1, 2) for r in (5, 8)}
    want["denoise_guides_kernel"] = 0
    for tag, ks in denoise_kernels.items():
        assert set(ks) == set(want), (tag, sorted(ks))
        for name, k in ks.items():
            assert k["scratch"] == 0 and k["vgpr"] <= 128, (tag, name, k)
            assert k["lds"] == want[name] <= 65536, (tag, name, k)
        assert ks["denoise_filter_kernel<1, 5>"]["lds"] == 33472      # the default R = 5, F = 1


# ------------------------------------------------------------------ bindings, command line
def test_capi_declares_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "nori_hip.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*|nori_hip_ctx \*)\s*(nori_hip_\w+)\(", header, re.M))
    lib = _capi.load_hip()
    for name in ("nori_hip_denoise_guides", "nori_hip_denoise", "nori_hip_denoise_guides_host", "nori_hip_denoise_host"):
        assert name in declared and name in _capi.HIP_PROTOTYPES and hasattr(lib, name), name
    assert declared <= set(_capi.HIP_PROTOTYPES)
    assert _capi.HIP_ABI_VERSION == 8 and "#define NORI_HIP_ABI_VERSION 8 " in header
    m = re.search(r"#define NORI_DENOISE_PARAMS_DEFAULT \{([^}]*)\}", header)
    values = [float(v.strip().rstrip("uf")) for v in m.group(1).split(",")]
    p = _capi.DenoiseParams()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct nori_denoise_params \{(.*?)\}", header, re.S).group(1), flags=re.S)
    assert [k for k, _ in p._fields_] == re.findall(r"(\w+)\s*[;,]", body)      # the struct's fields in the struct's order
    assert values == [pytest.approx(v) for v in p.as_dict().values()]
    assert p.as_dict() == pytest.approx(dr.DEFAULTS) and _capi.GUIDE_FLOATS == 16
    with pytest.raises(TypeError):
        _capi.DenoiseParams(raduis=3)


def test_cli_rejects_denoise_on_several_devices_and_stray_options(tmp_path):
    """before anything is loaded or a device is asked for: the scene file does not even exist"""
    exe = os.path.join(_capi.LIB_DIR, "nori")
    scene = str(tmp_path / "missing.xml")
    for args, words in ((["--denoise", "--gpus", "2"], ("one device",)),
                        (["--denoise-radius", "3"], ("--denoise-radius", "goes with --denoise")),
                        (["--denoise-patch", "1"], ("--denoise-patch", "goes with --denoise")),
                        (["--denoise", "--denoise-radius", "9"], ("1 .. 8",)),
                        (["--denoise", "--denoise-patch", "3"], ("0 .. 2",)),
                        (["--denoise", "--target-error", "0.05"], ("--target-error",))):
        p = subprocess.run([exe, scene] + args, capture_output=True, text=True, timeout=120)
        out = p.stdout + p.stderr
        assert p.returncode != 0 and "Usage" in out and "missing.xml" not in out, (args, out)
        for word in words:
            assert word in out, (args, out)
