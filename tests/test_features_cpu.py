"""First-hit feature frames without a GPU: the premise of the restatement (tests/features_ref.py) against the CPU oracle, the
resources of features.hip's kernels, the bindings and the command line."""
from __future__ import annotations

import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi
from nori_amd.scene import RFilter
from tests import features_ref as fr, film_cases, moments_ref as mr, scenes
from tests.backends import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
W, H = 45, 37      # 3 x 3 tiles, the right column 13 px wide, the bottom row 5 px high
SAMPLES = (0, 1, 5)


# ------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def cornell_samples():
    """per sample index of SAMPLES: (ps, values) of the Cornell box with a mirror and a glass sphere, and the oracle's 1-spp box frame"""
    sc = film_cases.cornell(W, H, 1, RFilter("box"), integrator="normals")
    o = Oracle(sc, use_bvh=True)
    out = {}
    for s in SAMPLES:
        ps = fr.camera_samples(W, H, s)
        out[s] = (ps, fr.sample_values(sc, ps, o), o.render_host(spp_count=1, spp_begin=s, threads=1)[0])
    o.close()
    return sc, out


def test_restated_samples_are_the_normals_integrators(cornell_samples):
    """|sh_n| of the restated samples is the oracle's `normals` frame of the same sample index under the box filter, bit for bit,
    W = 1 everywhere: the restated camera samples and hits are the ones a render draws and finds."""
    sc, per = cornell_samples
    meshes = set()
    for s, (ps, v, frame) in per.items():
        assert frame.shape == (H, W, 4) and (frame[..., 3] == 1).all()
        o = Oracle(sc, use_bvh=True)
        its = o.intersect(o.sample_rays(ps))
        o.close()
        want = np.where(v["hit"][:, None], np.abs(its["sh_n"]), F(0)).reshape(H, W, 3)
        assert np.array_equal(frame[..., :3], want), s
        assert np.array_equal(v["hit"], its["mesh"] != fr.NO_HIT)
        meshes |= set(int(m) for m in its["mesh"][v["hit"]])
    assert meshes == set(range(len(sc.meshes))), meshes         # all eight meshes, the mirror and the dielectric sphere included


def test_hits_and_misses_are_both_there(cornell_samples):
    sc, per = cornell_samples
    hit = np.concatenate([v["hit"] for _, v, _ in per.values()])
    assert 0.05 <= 1.0 - hit.mean() <= 0.60, hit.mean()
    normals = np.concatenate([v["normal"][v["hit"]] for _, v, _ in per.values()])
    assert (normals < F(0.5)).mean() > 0.05                     # negative components: what the encoding is for
    assert normals.min() >= 0 and normals.max() <= 1
    soup = scenes.soup_scene(500, 1, W, H)
    o = Oracle(soup, use_bvh=True)
    miss = 1.0 - np.concatenate([fr.sample_values(soup, fr.camera_samples(W, H, s), o)["hit"] for s in SAMPLES]).mean()
    o.close()
    assert 0.05 <= miss <= 0.60, miss


def test_values_follow_the_rules(cornell_samples):
    sc, per = cornell_samples
    ps, v, _ = per[0]
    o = Oracle(sc, use_bvh=True)
    its = o.intersect(o.sample_rays(ps))
    o.close()
    miss = ~v["hit"]
    assert (v["albedo"][miss] == 0).all() and (v["normal"][miss] == F(0.5)).all() and (v["depth"][miss] == 0).all()
    for mi, m in enumerate(sc.meshes):
        sel = its["mesh"] == mi
        want = (1, 1, 1) if m.bsdf.type in ("mirror", "dielectric") else m.bsdf.albedo
        assert (v["albedo"][sel] == np.asarray(want, F)).all(), m.name
    light = [i for i, m in enumerate(sc.meshes) if m.radiance is not None][0]
    assert (its["mesh"] == light).any() and (v["albedo"][its["mesh"] == light] == 0).all()      # the emitter's BSDF, not its radiance
    t = its["t"][v["hit"]]
    assert np.array_equal(v["depth"][v["hit"]], np.stack([t, (t * t).astype(F), np.ones_like(t)], axis=1))


def test_encode_decode_returns_the_normal(cornell_samples):
    """0.5 n is exact; one rounding in the add (<= 2^-24 below 1) and one in 2 e - 1 (<= 2^-24): within 2^-23 absolute"""
    sc, per = cornell_samples
    for s, (ps, v, _) in per.items():
        o = Oracle(sc, use_bvh=True)
        n = o.intersect(o.sample_rays(ps))["sh_n"][v["hit"]]
        o.close()
        e = v["normal"][v["hit"]]
        back = F(2) * e - F(1)
        assert np.abs(back.astype(np.float64) - n.astype(np.float64)).max() <= 2.0 ** -23
    # and through the film's decode: a one-sample box frame holds the sample itself
    frame = np.zeros((H, W, 4), F)
    frame[..., :3] = per[0][1]["normal"].reshape(H, W, 3); frame[..., 3] = 1
    dec = fr.decode({"normal": frame}, 0)["normal"]
    from nori_amd.render import develop_features_host
    assert np.array_equal(dec, develop_features_host({"normal": frame}, 0)["normal"])
    assert np.array_equal(dec, (F(2) * per[0][1]["normal"] - F(1)).reshape(H, W, 3))


@pytest.mark.parametrize("rf", [RFilter("box"), RFilter("tent"), RFilter("gaussian"), RFilter("gaussian", radius=5.2, stddev=1.3)], ids=lambda r: f"{r.type}-{r.radius}")
def test_film_of_a_constant_is_the_constant_times_the_weights(rf):
    sc = film_cases.cornell(W, H, 1, rf, integrator="normals")
    o = Oracle(sc, use_bvh=True)
    table, radius = o.filter_table(), mr.filter_radius(rf)
    o.close()
    ps = np.concatenate([fr.camera_samples(W, H, s) for s in (0, 1)])[::3]
    const = np.broadcast_to(np.asarray([0.25, 0.5, 0.75], F), (ps.shape[0], 3))
    total, abs_total, terms = fr.film_f64(ps, const, W, H, radius, table)
    assert np.array_equal(total, abs_total) and terms.max() > 0
    wsum = total[..., 3]
    for c, k in enumerate((0.25, 0.5, 0.75)):
        assert np.allclose(total[..., c], k * wsum, rtol=1e-14, atol=0)
    b = mr.border_of(radius)
    assert total.shape == (H + 2 * b, W + 2 * b, 4) and (wsum[terms == 0] == 0).all()
    # decode of such a frame gives the constant back wherever a weight arrived
    dec = fr.decode({"albedo": total.astype(F)}, b)["albedo"]
    inside = total[b:b + H, b:b + W, 3] > 0
    assert inside.any() and np.allclose(dec[inside], [0.25, 0.5, 0.75], rtol=1e-6)


def test_decode_of_depth_and_empty_pixels():
    frame = np.zeros((3, 3, 4), F)
    frame[0, 0] = (6.0, 20.0, 2.0, 4.0)       # two of four samples hit, at distances 2 and 4: R = 6, G = 4 + 16, B = 2, W = 4
    frame[0, 1] = (0.0, 0.0, 0.0, 4.0)        # all miss
    from nori_amd.render import develop_features_host
    for dec in (fr.decode({"depth": frame}, 0)["depth"], develop_features_host({"depth": frame}, 0)["depth"]):
        assert dec[0, 0].tolist() == [3.0, 0.5, 10.0] and dec[0, 1].tolist() == [0.0, 0.0, 0.0] and dec[2, 2].tolist() == [0.0, 0.0, 0.0]
    for name in ("albedo", "normal"):
        for dec in (fr.decode({name: frame}, 0)[name], develop_features_host({name: frame}, 0)[name]):
            assert dec[2, 2].tolist() == [0.0, 0.0, 0.0]      # W = 0: 0, not -1 and not NaN


# ------------------------------------------------------------------ the new device source
@pytest.fixture(scope="module")
def feature_kernels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as ge
    from kernel_resources import kernels
    assert "features.hip" in ge.HIP_SOURCES
    res = {}
    for tag, extra in (("product", []), ("count", ["-DNORI_COUNT_EXCURSIONS=1"])):
        out = tmp_path_factory.mktemp("asm") / f"features_{tag}.s"
        flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")] + extra
        p = subprocess.run([ge.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(ge.DEV, "features.hip"), "-o", str(out)],
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        res[tag] = {r["demangled"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: r for r in kernels(str(out))}
    return res


def test_feature_kernels_fit_their_budget(feature_kernels):
    want = {f"feature_pass_kernel<{s}>": s for s in (16, 24, 32, 64)}
    for tag, ks in feature_kernels.items():
        assert set(ks) == set(want), (tag, sorted(ks))
        for name, k in ks.items():
            assert k["scratch"] == 0 and k["vgpr"] <= 128, (tag, name, k)
            assert k["lds"] == want[name] * 256 * 4, (tag, name, k)      # the traversal stacks, nothing else


# ------------------------------------------------------------------ bindings, command line
def test_capi_declares_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "nori_hip.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*|nori_hip_ctx \*)\s*(nori_hip_\w+)\(", header, re.M))
    for name in ("nori_hip_render_features", "nori_hip_render_features_host"):
        assert name in declared and name in _capi.HIP_PROTOTYPES, name
    assert declared <= set(_capi.HIP_PROTOTYPES)
    assert "NORI_FEATURE_ALBEDO = 1, NORI_FEATURE_NORMAL = 2, NORI_FEATURE_DEPTH = 4" in header
    assert _capi.FEATURE_BITS == {"albedo": 1, "normal": 2, "depth": 4}
    assert _capi.HIP_ABI_VERSION == 8 and "#define NORI_HIP_ABI_VERSION 8 " in header
    lib = _capi.load_hip()
    assert hasattr(lib, "nori_hip_render_features") and hasattr(lib, "nori_hip_render_features_host")


def test_cli_rejects_features_on_several_devices_and_a_stray_feature_spp(tmp_path):
    """before anything is loaded or a device is asked for: the scene file does not even exist"""
    exe = os.path.join(_capi.LIB_DIR, "nori")
    p = subprocess.run([exe, str(tmp_path / "missing.xml"), "--features", "--gpus", "2"], capture_output=True, text=True, timeout=120)
    out = p.stdout + p.stderr
    assert p.returncode != 0 and "Usage" in out and "one device" in out and "missing.xml" not in out, out
    p = subprocess.run([exe, str(tmp_path / "missing.xml"), "--feature-spp", "4"], capture_output=True, text=True, timeout=120)
    out = p.stdout + p.stderr
    assert p.returncode != 0 and "Usage" in out and "--features" in out and "missing.xml" not in out, out
