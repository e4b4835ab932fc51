"""The thin-lens camera without a GPU (include/nori_hip.h, "Thin-lens camera"): properties of the numpy restatement
(tests/lens_ref.py) in binary64, its float32 evaluation against the binary64 one, the circle of confusion it gives on the scene of
tests/lens_cases.py, the bindings, the command line, the host's XML reader and the set of compiled wavefront kernels."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

from nori_amd import _capi, host
from nori_amd.scene import Scene
from tests import lens_cases as lc, lens_ref as lr
from tests.test_build_guards import wavefront_kernels      # noqa: F401  (the fixture: one compile of wavefront.hip to assembly)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shipped():
    return Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz"))


def _camera_space(sc, p):
    """world points -> camera space, binary64 (the shipped camera's transform is rigid up to float32 rounding)"""
    m = np.asarray(sc.camera.to_world, np.float64).reshape(4, 4)
    return (np.linalg.inv(m) @ np.concatenate([p, np.ones((p.shape[0], 1))], axis=1).T).T[:, :3]


# ------------------------------------------------------------------ 1. properties in binary64
def test_rays_of_a_film_point_meet_on_the_focal_plane():
    sc = _shipped()
    assert not np.allclose(sc.camera.to_world, np.eye(4))
    c = sc.camera
    rng = np.random.default_rng(5)
    n_film, n_ap, R, F = 1000, 64, 0.3125, 3.75      # (both are float32 numbers: the plane the test cuts with is the lens's)
    film = np.stack([rng.uniform(0, c.width, n_film), rng.uniform(0, c.height, n_film)], axis=1).astype(np.float32)
    ps = np.repeat(film, n_ap, axis=0)
    ap = rng.random((n_film * n_ap, 2), dtype=np.float32)
    r = lr.lens_rays(sc, ps, ap, R, F, dtype=np.float64)
    assert r["o"].dtype == np.float64
    # where each ray crosses the plane at camera-space depth F
    o, e = _camera_space(sc, r["o"]), _camera_space(sc, r["o"] + r["d"])
    d = e - o
    t = (F - o[:, 2]) / d[:, 2]
    p = (o + t[:, None] * d).reshape(n_film, n_ap, 3)
    spread = np.abs(p - p[:, :1]).max(axis=(1, 2))
    scale = np.abs(p).max(axis=(1, 2))
    # 1e-9 relative: binary64 evaluation of the formulas (~1e-15) through a float32 matrix inverted in binary64 (~1e-13)
    assert (spread <= 1e-9 * scale).all(), float((spread / scale).max())
    # origins: in the lens plane z = 0 of camera space, within R of the camera position
    assert np.abs(o[:, 2]).max() <= 1e-9 * F
    cam_pos = np.asarray(c.to_world, np.float64).reshape(4, 4)[:3, 3]
    dist = np.linalg.norm(r["o"] - cam_pos, axis=1)
    assert dist.max() <= R * (1 + 1e-6) and dist.max() > 0.9 * R      # (1e-6: the disk points are float32) ... and the disk is used
    # mint / maxt are the clip planes measured along the ray: the same camera-space depth for every ray
    assert np.allclose(r["mint"] * r["dl"][:, 2], c.near_clip, rtol=1e-12) and np.allclose(r["maxt"] * r["dl"][:, 2], c.far_clip, rtol=1e-12)


# ------------------------------------------------------------------ 2. float32 against binary64
def test_float32_evaluation_is_within_its_rounding_bound():
    sc = _shipped()
    c = sc.camera
    rng = np.random.default_rng(6)
    n, R, F = 20000, 0.3125, 3.75
    ps = np.stack([rng.uniform(0, c.width, n), rng.uniform(0, c.height, n)], axis=1).astype(np.float32)
    ap = rng.random((n, 2), dtype=np.float32)
    a, b = lr.lens_rays(sc, ps, ap, R, F), lr.lens_rays(sc, ps, ap, R, F, dtype=np.float64)
    assert a["d"].dtype == np.float32
    # Both start from the same float32 inputs (d, disk).  Every rounding on the way to a component of the direction perturbs
    # it by at most 2^-24 relative to the largest magnitude in play: the intermediate vectors are bounded by
    # |pf| + R <= F / cos(half the diagonal field of view) + R, the result by 1.  lens_ref counts the roundings of the longest
    # chain; the bound is that count, times 2^-24, times the growth |pf - l| / dl.z can give an error before normalisation (<= 2 here).
    half_diag = np.arctan(np.tan(np.radians(c.fov) / 2) * np.hypot(1.0, c.height / c.width))
    growth = 1.0 / np.cos(half_diag) + R / F
    assert growth < 2
    bound = lr.DIRECTION_ROUNDINGS * 2.0 ** -24 * 2
    err = np.abs(a["d"].astype(np.float64) - b["d"]).max()
    print(f"direction error {err:.3e}, bound {bound:.3e} ({lr.DIRECTION_ROUNDINGS} roundings)")
    assert err <= bound
    assert np.abs(np.linalg.norm(a["d"].astype(np.float64), axis=1) - 1).max() <= bound


def test_radius_zero_is_the_pinhole():
    sc = _shipped()
    ps = np.array([[3.25, 7.5], [100.0, 40.0]], np.float32)
    r = lr.lens_rays(sc, ps, np.array([[0.3, 0.9], [0.5, 0.5]], np.float32), 0.0, 3.0)
    from tests.backends import Oracle
    want = Oracle(sc).sample_rays(ps)
    for k in ("o", "d", "mint", "maxt"):
        assert np.array_equal(r[k], want[k])


# ------------------------------------------------------------------ 3. circle of confusion
def reference_covers(radius):
    """(W,) coverage per pixel column of the near and of the far quad: SPP camera samples per pixel, rays from lens_ref (float32),
    ray-plane hits, box filter (a sample counts for the pixel it was drawn in)."""
    sc = lc.scene()
    near, far = np.zeros(lc.W), np.zeros(lc.W)
    for s in range(lc.SPP):
        ps, ap = lr.camera_samples(lc.W, lc.H, s)
        r = lr.lens_rays(sc, ps, ap, radius, lc.F)
        hn, hf = lc.analytic_hits(r["o"], r["d"])
        near += hn.reshape(lc.H, lc.W).sum(axis=0)
        far += hf.reshape(lc.H, lc.W).sum(axis=0)
    return near / (lc.SPP * lc.H), far / (lc.SPP * lc.H)


def test_circle_of_confusion_of_the_reference():
    assert 11.5 <= lc.COC_PIXELS <= 12.5
    near, far = reference_covers(lc.R)
    n_near, n_far = lc.edge_counts(near, far)
    print(f"lens: in-focus edge {n_near} partial columns, far edge {n_far} (c = {lc.COC_PIXELS:.2f} px)")
    lc.assert_blur(n_near, n_far, lens=True)
    assert near.max() == 1 and far.max() == 1 and (near + far).min() == 0      # each quad fills columns, and the gap between them is empty
    near, far = reference_covers(0.0)
    n_near, n_far = lc.edge_counts(near, far)
    print(f"pinhole: {n_near}, {n_far}")
    lc.assert_blur(n_near, n_far, lens=False)


# ------------------------------------------------------------------ 4. bindings
NEW = {"nori_hip_set_lens": 3, "nori_hip_get_lens": 3, "nori_hip_sample_rays_lens": 5, "nori_hip_group_set_lens": 3}


def test_capi_declares_the_lens_entry_points():
    header = open(os.path.join(ROOT, "include", "nori_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _capi.load_hip()
    for name, arity in NEW.items():
        m = re.search(r"^int\s+" + name + r"\(([^)]*)\);", flat, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(_capi.HIP_PROTOTYPES[name][1]), name
        assert hasattr(lib, name), name
    assert _capi.HIP_ABI_VERSION == 8 and "#define NORI_HIP_ABI_VERSION 8 " in header and lib.nori_hip_abi_version() == 8
    declared = set(re.findall(r"^(?:int|void|const char \*|nori_hip_ctx \*)\s*(nori_hip_\w+)\(", header, re.M))
    assert declared <= set(_capi.HIP_PROTOTYPES)


def test_pinhole_fixtures_serialise_and_hash_as_before(tmp_path):
    import json
    sc = _shipped()
    assert sc.camera.aperture_radius == 0.0 and sc.camera.focus_distance == 1.0
    # the digest a fixture is keyed by: the value of the commit before there was a lens
    assert sc.geometry_digest() == scenes_digest_before()
    sc.save_npz(str(tmp_path / "a.npz"))
    meta = json.loads(bytes(np.load(tmp_path / "a.npz")["meta"]).decode())
    assert set(meta["camera"]) == {"width", "height", "fov", "near_clip", "far_clip"}
    sc.camera.aperture_radius, sc.camera.focus_distance = 0.25, 3.5
    assert sc.geometry_digest() == scenes_digest_before()
    sc.save_npz(str(tmp_path / "b.npz"))
    back = Scene.load_npz(str(tmp_path / "b.npz"))
    assert (back.camera.aperture_radius, back.camera.focus_distance) == (0.25, 3.5)


def scenes_digest_before():
    return "30e6d6f42582a5a114640851a56786f4de14019b1e65133c3fee2c2bf68d583e"      # tests/golden/pa4-cbox-path_mis.npz


# ------------------------------------------------------------------ 5. command line
@pytest.mark.parametrize("args, word", [
    (["--aperture"], "--aperture"), (["--aperture", "-0.1"], "--aperture"), (["--aperture", "wide"], "--aperture"), (["--aperture", "nan"], "--aperture"),
    (["--focus-distance"], "--focus-distance"), (["--focus-distance", "0"], "--focus-distance"), (["--focus-distance", "-2"], "--focus-distance"),
    (["--focus-distance", "far"], "--focus-distance"), (["--focus-pixel"], "--focus-pixel"), (["--focus-pixel", "3"], "--focus-pixel"),
    (["--focus-pixel", "-1", "4"], "--focus-pixel"), (["--focus-pixel", "3", "x"], "--focus-pixel"), (["--focus-pixel", "1.5", "2"], "--focus-pixel"),
    (["--focus-pixel", "3", "4", "--focus-distance", "2"], "does not go with"),
])
def test_cli_rejects_bad_lens_options_before_the_scene_is_opened(tmp_path, args, word):
    exe = os.path.join(_capi.LIB_DIR, "nori")
    p = subprocess.run([exe, str(tmp_path / "missing.xml")] + args, capture_output=True, text=True, timeout=120)
    out = p.stdout + p.stderr
    assert p.returncode != 0 and "Usage" in out and word in out and "missing.xml" not in out, out


# ------------------------------------------------------------------ 6. host
XML = """<scene><integrator type="normals"/>
  <sampler type="independent"><integer name="sampleCount" value="2"/></sampler>
  <camera type="perspective"><integer name="width" value="40"/><integer name="height" value="24"/><float name="fov" value="50"/>%s
    <transform name="toWorld"><lookat target="0, 0.5, 0" origin="0, 1, 4" up="0, 1, 0"/></transform></camera>
  <mesh type="obj"><string name="filename" value="floor.obj"/><bsdf type="diffuse"/></mesh>
</scene>"""


def test_host_reads_the_lens_of_the_camera(tmp_path):
    (tmp_path / "floor.obj").write_text("v -3 0 -3\nv -3 0 3\nv 3 0 3\nv 3 0 -3\nf 1 2 3 4\n")
    (tmp_path / "lens.xml").write_text(XML % '<float name="apertureRadius" value="0.125"/><float name="focusDistance" value="3.5"/>')
    (tmp_path / "pin.xml").write_text(XML % "")
    (tmp_path / "bad.xml").write_text(XML % '<float name="apertureRadius" value="0.125"/><float name="focusDistance" value="0"/>')
    root = host.HostRoot(str(tmp_path / "lens.xml"))
    assert root.lens() == (0.125, 3.5)
    cam = root.scene().camera
    assert (cam.aperture_radius, cam.focus_distance) == (0.125, 3.5)
    assert host.HostRoot(str(tmp_path / "pin.xml")).lens() == (0.0, 1.0)
    with pytest.raises(Exception, match="focusDistance"):
        host.HostRoot(str(tmp_path / "bad.xml"))


def test_a_shipped_scene_is_a_pinhole(tmp_path):
    import tarfile
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "reference_scenes.tar.xz")) as tar:
        tar.extractall(tmp_path, filter="data")
    root = host.HostRoot(str(tmp_path / "scenes" / "pa5" / "cbox" / "cbox_mis.xml"))
    assert root.lens() == (0.0, 1.0) and root.scene().camera.aperture_radius == 0.0


# ------------------------------------------------------------------ 7. the compiled kernel set
def test_wavefront_keeps_its_kernel_set(wavefront_kernels):
    """The lens is a branch inside first_vertex, uniform over a launch: no template parameter, no instantiation.  The names are those
    of the commit before the lens (tests/golden/wavefront_kernels.txt); the register budgets are tests/test_build_guards.py's, whose
    compile of wavefront.hip this test shares."""
    rows, _ = wavefront_kernels
    names = sorted(n.split("(")[0] for n in rows)
    want = sorted(w for w in open(os.path.join(ROOT, "tests", "golden", "wavefront_kernels.txt")).read().split("\n") if w)
    assert len(want) == 216 and all("wf_" in w for w in want)
    assert names == want, (sorted(set(names) - set(want)), sorted(set(want) - set(names)))
