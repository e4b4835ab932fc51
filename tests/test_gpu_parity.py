"""Parity of the HIP path (through the C ABI of include/nori_hip.h) with the
CPU oracle, on a real MI355X.  Tolerances:
  * ray/triangle hits, camera rays, pcg32, filter weights: bit exact
    (IEEE +,-,*,/,sqrt in the reference's order, -ffp-contract=off);
  * warps, BSDF sample / eval / pdf, and the radiance Li of every path: BIT EXACT as well -- sin/cos, log and
    exp are evaluated by one specification on both sides (rt_math.h / oracle_libm.h: binary64 arithmetic
    without FMA, one rounding to binary32), so no libm ulp separates device and oracle any more;
  * images: every camera sample carries identical radiance and identical filter weights; what remains is the
    order in which the film adds the samples of a pixel (float summation order).  Held to SURVEY.md 8(d):
    >= 99.9 % of the pixels within 1e-3 relative and mean relative error <= 1e-4 -- `assert_image_parity`
    below, used by every image test -- and ray counts must be EQUAL.
"""
import os

import numpy as np
import pytest

from nori_amd import NoriError
from nori_amd.scene import Bsdf, RFilter
from tests import scenes
from tests.backends import Oracle

pytestmark = pytest.mark.gpu

ITS_FIELDS = ["p", "t", "uv", "sh_s", "sh_t", "sh_n", "geo_s", "geo_t", "geo_n", "mesh", "tri"]

# 0 = NORI_ACCEL_HOST_SAH: the host's builder, Renderer.upload's default, whose trees the suite's pinned numbers belong to;
# 2 = NORI_ACCEL_AUTO: the library's default and what bench.py, smoke() and the C++ host pass -- the tree is built on the device (lbvh.hip)
BUILDERS = (0, 2)
ORACLE_THREADS = min(16, os.cpu_count() or 1)      # the oracle starts as many threads as it is told (0: as many as the machine has)


def assert_built_where_asked(r, builder):
    """AUTO falls back to the host's builder on any error of the device's and drops the message: only this field tells."""
    info = r.accel_info()
    assert info["built_on_device"] == (1 if builder == 2 else 0), (builder, info)
    return info


# SURVEY.md 8(d), per-sample seeding: the image contract every oracle comparison is held to
PIXEL_REL_TOL, PIXEL_FRACTION, MEAN_REL_TOL = 1e-3, 0.999, 1e-4


def image_parity(ref_rgb, got_rgb, floor=1e-2):
    """(fraction of pixels within PIXEL_REL_TOL, mean relative error) of two developed RGB images; a pixel's
    error is its worst channel, relative to the reference (values below `floor` compared absolutely against it)."""
    rel = (np.abs(ref_rgb - got_rgb) / np.maximum(np.abs(ref_rgb), floor)).max(axis=-1)
    return float((rel <= PIXEL_REL_TOL).mean()), float(rel.mean())


def assert_image_parity(ref_rgbw, got_rgbw, border, what=""):
    from nori_amd.render import develop_host
    # filter weights do not depend on libm: the W channel must agree to summation order
    np.testing.assert_allclose(got_rgbw[..., 3], ref_rgbw[..., 3], rtol=1e-5, atol=1e-6, err_msg=what)
    frac, mean_rel = image_parity(develop_host(ref_rgbw, border), develop_host(got_rgbw, border))
    print(f"[parity] {what}: {frac:.5%} of pixels within {PIXEL_REL_TOL:g}, mean relative error {mean_rel:.2e}")
    assert frac >= PIXEL_FRACTION, (what, frac)
    assert mean_rel <= MEAN_REL_TOL, (what, mean_rel)
    return frac, mean_rel


def assert_within_summation_bound(F, total, abs_total, terms, what=""):
    """A float32 RGBW frame F against the binary64 film of the same render (Oracle.render_f64), at EVERY pixel of the
    bordered frame and every channel:
        |F - total| <= (terms + 16) u abs_total,  u = 2^-24;     F == 0 exactly where abs_total == 0.
    A pixel's value is a sum of `terms` products v wx wy.  Each product is rounded at most twice and every addition a term
    passes through rounds once, so -- to first order, for ANY order and grouping of the additions -- the error is at most
    (n + 1) u sum |term|: a term passes through at most n - 1 additions that are not exact, because adding an exact 0 (an
    empty part, a tile that does not reach the pixel, the cleared frame) rounds nothing.  The 16 is the allowance for the
    merges (at most 8 part accumulators, 4 tiles or blocks, the frame add) and covers the second-order terms
    ((1 + u)^n - 1 - n u < 4 u for the n <= 2^13 a test frame reaches).  Nothing in it is fitted to a measured error.
    Prints and returns the worst error / bound."""
    F = np.asarray(F)
    assert F.dtype == np.float32 and F.shape == total.shape == abs_total.shape and terms.shape == F.shape[:2], what
    assert np.isfinite(F).all(), what
    bound = (terms[..., None].astype(np.float64) + 16.0) * 2.0 ** -24 * abs_total
    err = np.abs(F.astype(np.float64) - total)
    zero = abs_total == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(zero, 0.0, err / bound)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"[film bound] {what}: worst error / bound {worst:.3f}, {int(zero.any(axis=-1).sum())} pixels with a channel no term reaches")
    assert not F[zero].any(), f"{what}: {int((F[zero] != 0).sum())} values differ from 0 where no term has weight"
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values outside the bound, worst error / bound {worst:.3f} at {np.unravel_index(np.argmax(ratio), ratio.shape)}"
    return worst


def test_native_library_is_loaded(renderer_factory):
    import os
    r = renderer_factory(scenes.soup_scene(8))
    maps = open(f"/proc/{os.getpid()}/maps").read()
    assert "libnori_hip.so" in maps
    assert r.accel_info()["n_triangles"] == 8


@pytest.mark.parametrize("n_tris,seed,n_rays", [(1, 3, 10000), (300, 5, 200000), (20000, 6, 20000)])
def test_intersect_bitexact_vs_brute_force(renderer_factory, n_tris, seed, n_rays):
    sc = scenes.soup_scene(n_tris, seed)
    rays = scenes.random_rays(n_rays, seed=seed + 10)
    r, o = renderer_factory(sc), Oracle(sc)
    a, b = o.intersect(rays), r.intersect(rays)
    for k in ITS_FIELDS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(o.intersect(rays, True)["mesh"], r.intersect(rays, True)["mesh"])


def test_intersect_cornell_axis_aligned(renderer_factory):
    sc = scenes.cornell_box(16, 16, 1)
    rays = scenes.random_rays(200000, seed=7, extent=0.9)
    rays["o"] += np.float32([0, 1, 0])
    rays["d"][:3000] = np.float32([0, -1, 0])
    rays["d"][3000:6000] = np.float32([1, 0, 0])
    rays["maxt"][7000:9000] = np.random.default_rng(1).uniform(0.1, 2.0, 2000).astype(np.float32)
    r, o = renderer_factory(sc), Oracle(sc)
    a, b = o.intersect(rays), r.intersect(rays)
    for k in ITS_FIELDS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(o.intersect(rays, True)["mesh"], r.intersect(rays, True)["mesh"])


def test_empty_and_ragged_inputs(renderer_factory):
    sc = scenes.soup_scene(5)
    r = renderer_factory(sc)
    assert r.intersect(scenes.random_rays(0)).shape == (0,)
    assert r.intersect(scenes.random_rays(1)).shape == (1,)
    assert r.intersect(scenes.random_rays(257)).shape == (257,)
    sc.meshes = []
    r2 = renderer_factory(sc)
    assert (r2.intersect(scenes.random_rays(100))["mesh"] == 0xFFFFFFFF).all()
    rgbw, st = r2.render_host(spp_count=2)
    assert st["n_camera_samples"] == 32 * 32 * 2 and st["n_closest_rays"] == 32 * 32 * 2
    assert (rgbw[..., :3] == 0).all() and rgbw[..., 3].max() > 0


def test_camera_rays_and_pcg32_bitexact(renderer_factory):
    sc = scenes.cornell_box(800, 600, 1)
    r, o = renderer_factory(sc), Oracle(sc)
    ps = np.random.default_rng(3).uniform(0, 600, (50000, 2)).astype(np.float32)
    assert np.array_equal(o.sample_rays(ps), r.sample_rays(ps))
    st = np.random.default_rng(4).integers(0, 2 ** 63, 1000, dtype=np.uint64)
    assert np.array_equal(Oracle.pcg32_floats(st, st[::-1].copy(), 100), r.pcg32_floats(st, st[::-1].copy(), 100))


def test_warps_and_bsdfs(renderer_factory):
    r = renderer_factory(scenes.soup_scene(4))
    rng = np.random.default_rng(5)
    n = 100000
    s = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    for name, param in [("square", 0), ("tent", 0), ("disk", 0), ("uniform_sphere", 0), ("uniform_hemisphere", 0),
                        ("cosine_hemisphere", 0), ("beckmann", 0.3)]:
        a, b = Oracle.warp(name, s, param), r.warp(name, s, param)
        assert np.array_equal(a, b), name                                         # same sincos / log specification: same bits
        assert np.array_equal(r.warp_pdf(name, a, param), Oracle.warp_pdf(name, a, param)), name
    wi = rng.normal(size=(n, 3)).astype(np.float32); wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wo = rng.normal(size=(n, 3)).astype(np.float32); wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    for b in [Bsdf("diffuse", (0.2, 0.5, 0.7)), Bsdf("mirror"), Bsdf("dielectric"),
              Bsdf("microfacet", (0.1, 0.2, 0.15), 0.1, 1.5), Bsdf("microfacet", (0.4, 0.2, 0.3), 0.6, 1.8, 1.3)]:
        o_wo, o_w, o_eta, o_m = Oracle.bsdf_sample(b, wi, s)
        g_wo, g_w, g_eta, g_m = r.bsdf_sample(b, wi, s)
        assert np.array_equal(o_m, g_m) and np.array_equal(o_eta, g_eta)
        assert np.array_equal(g_wo, o_wo) and np.array_equal(g_w, o_w), b.type
        assert np.array_equal(r.bsdf_eval(b, wi, wo), Oracle.bsdf_eval(b, wi, wo)), b.type
        assert np.array_equal(r.bsdf_pdf(b, wi, wo), Oracle.bsdf_pdf(b, wi, wo)), b.type


def test_division_edge_operands_inside_the_domain(renderer_factory):
    """The device replaces `/`, `1 / x` and sqrt of the shading code by short sequences that are bit-identical to the
    IEEE operations on a stated domain (rt_types.h: divisors in [2^-126, 2^126), numerators from 2^-100, normal quotients).
    Edge operands INSIDE it -- grazing directions with cosines of exactly zero, ks = 0 and ks = 1, indices of refraction
    thirty orders of magnitude apart, equal indices, a very smooth and a very rough microfacet lobe -- must give the
    oracle's plain-IEEE results bit for bit, NaN and infinity patterns included.  (Outside the domain -- zero, infinite or
    denormal divisors -- the last bit is unspecified and IEEE's inf / 0 may come out as NaN; such samples are dropped by
    the film either way, and test_shading_arithmetic_stays_inside_its_verified_domain shows no golden scene gets there.)"""
    r = renderer_factory(scenes.soup_scene(4))
    rng = np.random.default_rng(17)
    n = 20000
    s = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    s[::40, 0] = 0.0; s[1::40, 1] = 0.0                       # samples on the edge of the unit square
    wi = rng.normal(size=(n, 3)).astype(np.float32); wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wo = rng.normal(size=(n, 3)).astype(np.float32); wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    wi[::50] = np.float32([1.0, 0.0, 0.0]); wo[1::50] = np.float32([0.0, -1.0, 0.0])      # grazing: cos theta exactly 0
    wi[2::50] = np.float32([0.0, 0.0, 1.0])                                                 # along the normal: tan theta exactly 0
    cases = [Bsdf("dielectric", int_ior=1e15, ext_ior=1e-15), Bsdf("dielectric", int_ior=1e-15, ext_ior=1e15), Bsdf("dielectric", int_ior=1.3, ext_ior=1.3),
             Bsdf("microfacet", (0.0, 0.0, 0.0), 0.3, 1.5), Bsdf("microfacet", (1.0, 1.0, 1.0), 0.3, 1.5),      # ks = 1 and ks = 0
             Bsdf("microfacet", (0.2, 0.2, 0.2), 1e-4, 1.5), Bsdf("microfacet", (0.2, 0.2, 0.2), 50.0, 1.5), Bsdf("microfacet", (0.3, 0.3, 0.3), 0.2, 1.0, 1.0)]
    for b in cases:
        o_wo, o_w, o_eta, o_m = Oracle.bsdf_sample(b, wi, s)
        g_wo, g_w, g_eta, g_m = r.bsdf_sample(b, wi, s)
        tag = f"{b.type} alpha={b.alpha} int={b.int_ior} ext={b.ext_ior} kd={b.albedo}"
        assert np.array_equal(o_m, g_m), tag
        assert np.array_equal(o_eta, g_eta, equal_nan=True), tag
        assert np.array_equal(o_wo, g_wo, equal_nan=True) and np.array_equal(o_w, g_w, equal_nan=True), tag
        assert np.array_equal(r.bsdf_eval(b, wi, wo), Oracle.bsdf_eval(b, wi, wo), equal_nan=True), tag
        assert np.array_equal(r.bsdf_pdf(b, wi, wo), Oracle.bsdf_pdf(b, wi, wo), equal_nan=True), tag


def test_shading_arithmetic_stays_inside_its_verified_domain():
    """libnori_hip_count.so = the product sources built with -DNORI_COUNT_EXCURSIONS: every operand of exact_rcp / exact_div /
    exact_sqrt outside the domain on which they are verified against the IEEE operations is counted, and every result the
    result that came out NaN or infinite.  On the golden scenes -- seven integrators, every shipped material, both
    engines -- all four counts are zero: the bit-exactness claims of the parity tests rest on verified arithmetic only."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "nori_amd", "lib", "libnori_hip_count.so")
    assert os.path.exists(lib), "libnori_hip_count.so missing: __graft_entry__.build() makes it"
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "excursion_probe.py"), "8"], capture_output=True, text=True, cwd=root,
                       env=dict(os.environ, NORI_HIP_LIBRARY=lib), timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    rows = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == 18
    for row in rows:
        print("[excursions]", row)
        assert row["rays"] > 0
        assert (row["rcp_out_of_domain"], row["div_out_of_domain"], row["sqrt_out_of_domain"], row["fallbacks"]) == (0, 0, 0, 0), row


@pytest.mark.parametrize("integ", ["normals", "ao", "simple", "whitted", "path_mats", "path_ems", "path_mis"])
def test_li_matches_oracle(renderer_factory, integ):
    sb = [Bsdf("mirror"), Bsdf("dielectric")] if integ in ("whitted", "path_mis") else \
        [Bsdf("microfacet", (0.2, 0.3, 0.1), 0.2), Bsdf("diffuse")]
    sc = scenes.cornell_box(16, 16, 1, integ, sphere_bsdfs=sb)
    sc.integrator.position, sc.integrator.energy = (0, 1.5, 0.5), (30, 30, 30)
    r, o = renderer_factory(sc), Oracle(sc, use_bvh=True)
    rng = np.random.default_rng(11)
    n = 100000
    rays = o.sample_rays(rng.uniform(0, 16, (n, 2)).astype(np.float32))
    ss = rng.integers(0, 2 ** 62, n, dtype=np.uint64)
    sq = rng.integers(0, 2 ** 62, n, dtype=np.uint64)
    a, b = o.li(rays, ss, sq), r.li(rays, ss, sq)
    assert np.isfinite(b).all()
    # every path: the same radiance, bit for bit (same pcg32 stream, same IEEE operations in the same order,
    # same sin / cos / log / exp specification)
    differ = int((a != b).any(axis=1).sum())
    print(f"[parity] li {integ}: {differ} of {n} paths differ from the oracle")
    assert differ == 0


def test_splat_matches_imageblock_put(renderer_factory):
    for rf in ["gaussian", "mitchell", "tent", "box"]:
        sc = scenes.cornell_box(40, 24, 1, rfilter=RFilter(rf))
        r, o = renderer_factory(sc), Oracle(sc)
        rng = np.random.default_rng(2)
        pos = rng.uniform(0, 1, (5000, 2)).astype(np.float32) * np.float32([40, 24])
        val = rng.uniform(0, 2, (5000, 3)).astype(np.float32)
        val[::97] = np.nan          # invalid radiance is dropped (block.cpp:63-67)
        val[1::97, 1] = -1.0
        a, b = o.splat(pos, val), r.splat(pos, val)
        np.testing.assert_allclose(b, a, rtol=1e-5, atol=1e-6, err_msg=rf)


@pytest.mark.parametrize("integ,rf,size", [("path_mis", "gaussian", (40, 24)), ("path_ems", "mitchell", (64, 64)),
                                          ("whitted", "tent", (33, 17)), ("normals", "box", (16, 16))])
def test_render_matches_oracle(renderer_factory, integ, rf, size):
    sc = scenes.cornell_box(size[0], size[1], 8, integ, rfilter=RFilter(rf))
    r, o = renderer_factory(sc), Oracle(sc, use_bvh=True)
    A, sa = o.render_host()
    B, sb = r.render_host()
    assert sb["n_camera_samples"] == sa["n_camera_samples"] == size[0] * size[1] * 8
    assert sb["n_invalid"] == 0
    for k in ("n_closest_rays", "n_shadow_rays"):
        assert int(sa[k]) == int(sb[k]), k              # identical paths: identical ray counts
    assert_image_parity(A, B, r.border, f"{integ}/{rf} {size}")


def test_render_matches_the_host_libm_oracle(renderer_factory, tmp_path):
    """Device and oracle evaluate sin / cos / log / exp by one pinned specification -- which is why they agree bit for bit,
    and why their agreement says nothing about the specification itself.  The independent witness is the oracle built with
    the HOST libm's functions (oracle/liboracle_glibc.so: std::sin / cos / log / exp, as the reference calls them): the
    device render must meet the image contract against it too, with equal ray counts."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "oracle", "liboracle_glibc.so")
    subprocess.run(["make", "-C", os.path.join(root, "oracle"), "liboracle_glibc.so"], check=True, capture_output=True)
    out = tmp_path / "glibc.npy"
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "oracle_render.py"), "cornell", "64", "48", "8", "path_mis", str(out)],
                       capture_output=True, text=True, cwd=root, env=dict(os.environ, NORI_ORACLE_LIBRARY=lib), timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    sc = scenes.cornell_box(64, 48, 8, "path_mis", sphere_bsdfs=[Bsdf("microfacet", (0.2, 0.3, 0.1), 0.2), Bsdf("dielectric")])
    r = renderer_factory(sc)
    got, st = r.render_host()
    assert [str(st["n_closest_rays"]), str(st["n_shadow_rays"])] == p.stdout.split()
    assert_image_parity(np.load(out), got, r.border, "device vs host-libm oracle")


def test_tile_and_sample_split_sum_to_whole(renderer_factory):
    sc = scenes.cornell_box(72, 40, 12, "path_mis")
    r = renderer_factory(sc)
    whole, st = r.render_host()
    # the parts carry the same samples with the same weights; only the order of the additions differs (per pixel: the
    # samples of one tile, then the tiles; or the two sample ranges) -- held to the image contract, W to summation order
    parts = sum(r.render_host(tile_mod=4, tile_rem=k)[0] for k in range(4))
    assert_image_parity(whole, parts, r.border, "tile split x4")
    parts = r.render_host(spp_count=5, spp_begin=0)[0] + r.render_host(spp_count=7, spp_begin=5)[0]
    assert_image_parity(whole, parts, r.border, "sample split 5 + 7")


def test_render_into_torch_and_develop(renderer_factory):
    import torch
    sc = scenes.cornell_box(64, 48, 4, "path_mis")
    r = renderer_factory(sc)
    frame = torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        st = r.render_into(frame, stream=s)
        rgb = r.develop(frame, stream=s)
    s.synchronize()
    host, _ = r.render_host()
    np.testing.assert_allclose(frame.cpu().numpy(), host, rtol=1e-4, atol=1e-5)
    from nori_amd.render import develop_host
    np.testing.assert_allclose(rgb.cpu().numpy(), develop_host(frame.cpu().numpy(), r.border), rtol=1e-6)
    assert st["kernel_ms"] > 0


def test_counters_and_instrumented_build(renderer_factory):
    sc = scenes.cornell_box(64, 64, 4, "path_mis")
    r, o = renderer_factory(sc), Oracle(sc, use_bvh=True)
    a, sa = r.render_host(count_traversal=True)
    b, sb = r.render_host(count_traversal=False)
    assert sa["n_node_tests"] > sa["n_closest_rays"] and sa["n_tri_tests"] > 0
    assert sb["n_node_tests"] == 0
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5)


def test_error_behaviour():
    from nori_amd.render import Renderer
    r = Renderer(0)
    with pytest.raises(NoriError, match="NOT_READY"):
        r.build_accel()
    sc = scenes.soup_scene(4)
    r.upload(sc, build=False)
    with pytest.raises(NoriError, match="NOT_READY"):
        r.intersect(scenes.random_rays(4))
    sc.meshes[0].indices[0, 0] = 999
    with pytest.raises(NoriError, match="out of range"):
        r.upload(sc)
    with pytest.raises(NoriError):
        Renderer(99)
    r.close()


@pytest.mark.parametrize("seed,margin,budget,layout", [(21, 1.0, 1.0, "bvh2"), (22, 0.99, 0.3, "bvh2"), (23, 1.0, 4.0, "bvh4q")])
def test_spatial_splits_give_the_scans_answers(monkeypatch, seed, margin, budget, layout):
    """Spatial splits in the host builder (scene_prep.cpp, build_tree_spatial): triangles hang in several leaves.  Every field of
    the intersection record is the linear scan's (src/accel.cpp:23-99) -- a leaf step tests the whole triangle whichever leaf it is
    reached through, and the tie rule replaces a hit by itself -- through the batch kernels and, in a render, through the
    hand-written node loop on the 32-B records or the wide-node walk: the frame and ray counts of the tree without spatial splits."""
    from nori_amd.render import Renderer
    from tests.test_device_logic_cpu import _mixed_soup
    sc = _mixed_soup(seed)
    rays = scenes.random_rays(50000, seed=seed + 10)
    o = Oracle(sc)

    def make(scene, sbvh):
        monkeypatch.setenv("NORI_HIP_SBVH", str(sbvh)); monkeypatch.setenv("NORI_HIP_SBVH_MARGIN", str(margin))
        r = Renderer(0); r.set_option("accel_layout", layout); r.upload(scene)
        return r
    plain, r = make(sc, 0), make(sc, budget)
    info, pinfo = r.accel_info(), plain.accel_info()
    assert info["node_children"] == (4 if layout == "bvh4q" else 2)
    assert info["total_bytes"] > pinfo["total_bytes"] and info["sah_cost"] < pinfo["sah_cost"]
    a, b = o.intersect(rays), r.intersect(rays)
    for k in ITS_FIELDS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(o.intersect(rays, True)["mesh"], r.intersect(rays, True)["mesh"])
    plain.close(); r.close()
    sc.integrator.type = "ao"; sc.sample_count = 4; sc.camera.width, sc.camera.height = 96, 64
    p2, r2 = make(sc, 0), make(sc, budget)
    for eng in (("wavefront",) if layout == "bvh4q" else ("megakernel", "wavefront")):
        p2.set_option("engine", eng); r2.set_option("engine", eng)
        A, sa = p2.render_host()
        B, sb = r2.render_host()
        assert np.array_equal(A, B), eng
        assert sa["n_closest_rays"] == sb["n_closest_rays"] and sa["n_shadow_rays"] == sb["n_shadow_rays"]
    p2.close(); r2.close()


def test_tree_optimised_by_reinsertion_gives_the_scans_answers(monkeypatch):
    """optimize_tree_reinsertion in the host builder (scene_prep.cpp; kept when the SAH cost drops by 2 %): the records of the scan,
    field by field, and a render with the bits and ray counts of the top-down builder's tree -- fewer node tests for the same rays."""
    from nori_amd.render import Renderer
    from tests.test_device_logic_cpu import _objects_on_planes
    sc = _objects_on_planes()
    rays = scenes.random_rays(50000, seed=61, extent=1.5, target_extent=0.3)
    o = Oracle(sc)

    def make(scene, passes):
        monkeypatch.setenv("NORI_HIP_REINSERT", str(passes))
        return Renderer(0).upload(scene)
    plain, r = make(sc, 0), make(sc, 10)
    assert r.accel_info()["sah_cost"] < 0.95 * plain.accel_info()["sah_cost"]
    a, b = o.intersect(rays), r.intersect(rays)
    for k in ITS_FIELDS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(o.intersect(rays, True)["mesh"], r.intersect(rays, True)["mesh"])
    plain.close(); r.close()
    sc.integrator.type = "ao"; sc.sample_count = 4; sc.camera.width, sc.camera.height = 96, 64
    p2, r2 = make(sc, 0), make(sc, 10)
    for eng in ("megakernel", "wavefront"):
        p2.set_option("engine", eng); r2.set_option("engine", eng)
        A, sa = p2.render_host(count_traversal=True)
        B, sb = r2.render_host(count_traversal=True)
        assert np.array_equal(A, B), eng
        assert sa["n_closest_rays"] == sb["n_closest_rays"] and sa["n_shadow_rays"] == sb["n_shadow_rays"]
        assert sb["n_node_tests"] < sa["n_node_tests"]
    p2.close(); r2.close()


@pytest.mark.parametrize("builder", [1, 3])
@pytest.mark.parametrize("n_tris,seed", [(1, 3), (3, 4), (5, 5), (6, 2), (300, 6), (20000, 7)])
def test_gpu_lbvh_builder_same_hits_as_brute_force(renderer_factory, n_tris, seed, builder):
    """Accel::build on the device (1: Morton order + radix tree, 3: Morton order + PLOC clustering): any valid BVH must give the
    scan's answers."""
    sc = scenes.soup_scene(n_tris, seed)
    rays = scenes.random_rays(50000, seed=seed + 20)
    r, o = renderer_factory(sc, builder=builder), Oracle(sc)
    info = r.accel_info()
    assert info["n_triangles"] == n_tris and info["max_depth"] < 64
    a, b = o.intersect(rays), r.intersect(rays)
    for k in ITS_FIELDS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(o.intersect(rays, True)["mesh"], r.intersect(rays, True)["mesh"])


def test_gpu_triangle_splitting_and_reinsertion_in_the_device_builder(renderer_factory):
    """lbvh.hip, round 6: references (a triangle whose box is several times the scene's typical one and holds other geometry enters the tree
    as several parts) and parallel re-insertion.  The pa5 table scene: the device tree's hits are the host tree's, record for record, at
    no more node tests and fewer triangle tests than the host's SAH + SBVH tree needs by more than 5 %; the Cornell box is not cut.  The
    kernels are one thread per element over the steps the CPU harness runs as loops (tests/emu/emu_builder.h) and every decision is made
    in integer sums or in IEEE operations both compilers round alike: the device's tree has the harness's reference, node and level
    counts (computed on the CPU, pinned here).  And every triangle of a soup cut as often as the cap allows: the scan's answers."""
    import os
    from nori_amd.scene import Scene
    table = Scene.load_npz(os.path.join(os.path.dirname(__file__), "golden", "pa5-table_mis.npz"))
    table.camera.width, table.camera.height, table.sample_count = 160, 120, 2
    cbox = Scene.load_npz(os.path.join(os.path.dirname(__file__), "golden", "pa4-cbox-path_mis.npz"))
    cbox.camera.width, cbox.camera.height, cbox.sample_count = 96, 96, 2
    for sc, pinned in ((table, (22766, 26100, 11436, 33)), (cbox, (7948, 7948, 3778, 23))):
        host, dev = renderer_factory(sc, builder=0), renderer_factory(sc, builder=3)
        ih, idv = host.accel_info(), dev.accel_info()
        assert ih["built_on_device"] == 0 and idv["built_on_device"] == 1
        assert (idv["n_triangles"], idv["n_references"], idv["n_nodes"], idv["max_depth"]) == pinned, idv
        v = np.concatenate([m.positions for m in sc.meshes])
        centre, half = 0.5 * (v.min(0) + v.max(0)), 0.5 * float(np.linalg.norm(v.max(0) - v.min(0)))
        rays = scenes.random_rays(200000, seed=77, extent=1.5, target_extent=0.5)      # a shell around the scene, aimed into it
        rays["o"] = (rays["o"] * half + centre).astype(np.float32)
        rays["mint"] = 1e-4 * half
        a, b = host.intersect(rays), dev.intersect(rays)
        for k in ITS_FIELDS:
            assert np.array_equal(a[k], b[k]), k
        fa, sa = host.render_host(count_traversal=True)
        fb, sb = dev.render_host(count_traversal=True)
        assert sa["n_closest_rays"] == sb["n_closest_rays"] and sa["n_shadow_rays"] == sb["n_shadow_rays"]
        np.testing.assert_allclose(fb, fa, rtol=1e-4, atol=1e-5)
        assert sb["n_node_tests"] <= 1.05 * sa["n_node_tests"] and sb["n_tri_tests"] <= 1.05 * sa["n_tri_tests"], (sa, sb)
    sc = scenes.soup_scene(20000, 7)
    rays = scenes.random_rays(50000, seed=27)
    env = {"NORI_HIP_SPLIT_BUDGET": "3.0", "NORI_HIP_SPLIT_SCALE": "0", "NORI_HIP_SPLIT_INSIDE": "0"}
    os.environ.update(env)
    try:
        r = renderer_factory(sc, builder=3)
    finally:
        for k in env:
            del os.environ[k]
    info = r.accel_info()
    assert (info["n_references"], info["n_nodes"], info["max_depth"]) == (79924, 42706, 28), info
    o = Oracle(sc)
    a, b = o.intersect(rays), r.intersect(rays)
    for k in ITS_FIELDS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(o.intersect(rays, True)["mesh"], r.intersect(rays, True)["mesh"])


def test_treelet_wave_builds_the_tree_of_the_serial_form():
    """Treelet restructuring on the device: a WAVE per treelet (lbvh.hip, treelet_optimize_wave: subset areas two per lane, the dynamic
    programme's (subset, partition) pairs spread over the lanes, winners by a 64-bit LDS minimum that keeps the serial loop's tie rule)
    against one thread per treelet (NORI_HIP_TREELET_SERIAL=1 -- the form the CPU harness runs, lbvh_steps.h): the same tree.  Checked
    by what a tree determines: node count, depth, SAH cost, and the node / triangle tests of a render."""
    from nori_amd.render import Renderer
    from nori_amd.scene import Scene
    import os
    jobs = [scenes.soup_scene(30000, seed=11, width=96, height=64, integrator="path_mis"),
            Scene.load_npz(os.path.join(os.path.dirname(__file__), "golden", "pa5-table_mis.npz"))]
    jobs[0].sample_count = 2
    jobs[1].camera.width, jobs[1].camera.height, jobs[1].sample_count = 160, 120, 2
    for sc in jobs:
        got = {}
        for serial in (0, 1):
            os.environ["NORI_HIP_TREELET_SERIAL"] = str(serial)
            os.environ["NORI_HIP_TREELET_SWEEPS"] = "2"
            try:
                r = Renderer(0).upload(sc, builder=3)
            finally:
                del os.environ["NORI_HIP_TREELET_SERIAL"], os.environ["NORI_HIP_TREELET_SWEEPS"]
            info = r.accel_info()
            frame, st = r.render_host(count_traversal=True)
            got[serial] = (info["n_nodes"], info["max_depth"], info["sah_cost"], st["n_node_tests"], st["n_tri_tests"], frame)
            r.close()
        assert got[0][:5] == got[1][:5], (got[0][:5], got[1][:5])
        assert np.array_equal(got[0][5], got[1][5])


def test_two_device_builds_of_one_scene_give_one_tree():
    """The device builder decides in integer sums and settles conflicts by 64-bit maxima (lbvh.hip): which thread comes first is a
    matter of timing, what is built is not.  Two contexts, builder = auto, one scene: the same tree -- by what a tree determines: node,
    reference and level counts, SAH cost, the node and triangle tests of a render in either engine -- and the same frame, bit for bit.
    (test_reference_scenes_both_engines_and_oracle compares the counters of two contexts' trees and rests on this.)  The pa5 table
    (triangles cut into references, re-insertion), the headline Cornell box at a reduced frame, a 30,000-triangle soup."""
    from nori_amd.render import Renderer
    from nori_amd.scene import Mesh, Scene
    golden = os.path.join(os.path.dirname(__file__), "golden")
    table = Scene.load_npz(os.path.join(golden, "pa5-table_mis.npz"))
    table.camera.width, table.camera.height, table.sample_count = 160, 120, 2
    cbox = Scene.load_npz(os.path.join(golden, "pa4-cbox-path_mis.npz"))
    cbox.camera.width, cbox.camera.height, cbox.sample_count = 256, 256, 2
    soup = scenes.soup_scene(30000, seed=3, width=80, height=56, integrator="path_mis")
    soup.sample_count = 4
    v, f = scenes.quad((-3, 3, -3), (3, 3, -3), (3, 3, 3), (-3, 3, 3))
    soup.meshes.append(Mesh(v, f, bsdf=Bsdf("diffuse", (0, 0, 0)), radiance=(5.0, 5.0, 5.0), name="light"))
    for name, sc in (("table", table), ("cbox", cbox), ("soup", soup)):
        a, b = Renderer(0).upload(sc, builder=2), Renderer(0).upload(sc, builder=2)
        ia, ib = assert_built_where_asked(a, 2), assert_built_where_asked(b, 2)
        if name == "table":
            assert ia["n_references"] > ia["n_triangles"]
        for k in ("n_triangles", "n_nodes", "n_leaves", "n_references", "max_depth", "sah_cost", "node_children", "node_records_32b", "total_bytes"):
            assert ia[k] == ib[k], (name, k, ia[k], ib[k])
        for engine in ("megakernel", "wavefront"):
            a.set_option("engine", engine); b.set_option("engine", engine)
            A, sa = a.render_host(count_traversal=True)
            B, sb = b.render_host(count_traversal=True)
            for k in ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_node_tests", "n_tri_tests", "n_invalid"):
                assert sa[k] == sb[k], (name, engine, k, sa[k], sb[k])
            assert sa["n_node_tests"] > 0 and sa["n_tri_tests"] > 0
            assert np.array_equal(A, B), (name, engine)
        a.close(); b.close()


def test_gpu_lbvh_render_equals_sah_render(renderer_factory):
    from tests import stat_harness  # noqa: F401
    from nori_amd.scene import Scene
    import os
    sc = Scene.load_npz(os.path.join(os.path.dirname(__file__), "golden", "pa5-cbox_mis.npz"))
    sc.camera.width, sc.camera.height, sc.sample_count = 160, 120, 8
    a, sa = renderer_factory(sc, builder=0).render_host(count_traversal=True)
    cost = {0: sa["n_node_tests"] + 2 * sa["n_tri_tests"]}
    for builder in (1, 3):
        b, sb = renderer_factory(sc, builder=builder).render_host(count_traversal=True)
        # same hits -> same paths: images differ by float summation order only
        np.testing.assert_allclose(b, a, rtol=1e-4, atol=1e-5)
        assert sa["n_closest_rays"] == sb["n_closest_rays"] and sa["n_shadow_rays"] == sb["n_shadow_rays"]
        cost[builder] = sb["n_node_tests"] + 2 * sb["n_tri_tests"]
    print(f"[builders] node + 2 x triangle tests per frame: host SAH {cost[0]}, radix tree {cost[1]}, PLOC {cost[3]}")
    assert cost[3] < cost[1]              # what the clustering is for


def test_gpu_lbvh_large_scene_build(renderer_factory):
    """1 M triangles: build on the device, spot-check hits against the SAH tree."""
    v, f, n = scenes.icosphere(0)
    rng = np.random.default_rng(9)
    nt = 1_000_000
    c = rng.uniform(-1, 1, (nt, 1, 3)).astype(np.float32)
    tri = (c + rng.uniform(-0.01, 0.01, (nt, 3, 3)).astype(np.float32)).reshape(-1, 3)
    from nori_amd.scene import Mesh
    sc = scenes.soup_scene(1)
    sc.meshes = [Mesh(tri, np.arange(3 * nt, dtype=np.uint32).reshape(nt, 3))]
    rays = scenes.random_rays(20000, seed=4)
    r0 = renderer_factory(sc, builder=0)
    a = r0.intersect(rays)
    for builder in (1, 3):
        r1 = renderer_factory(sc, builder=builder)
        info = r1.accel_info()
        print(f"[builders] 1 M triangles, builder {builder}: {info['build_ms']:.1f} ms, {info['n_nodes']} nodes, depth {info['max_depth']}")
        assert info["build_ms"] < 2000 and info["max_depth"] < 64
        b = r1.intersect(rays)
        for k in ITS_FIELDS:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("radius,engine", [(0.5, "megakernel"), (3.4, "megakernel"), (4.6, "wavefront"), (8.4, "megakernel"), (8.4, "wavefront")])
def test_film_wide_filters(renderer_factory, radius, engine):
    """ImageBlock::put with borders 0 .. 8 (film_gather keeps 2*border+1 taps per axis per sample);
    image size not a multiple of the 16-px tile nor of Nori's 32-px block."""
    sc = scenes.cornell_box(45, 37, 3, "normals", rfilter=RFilter("gaussian", radius=radius, stddev=radius / 4))
    r, o = renderer_factory(sc), Oracle(sc, use_bvh=True)
    r.set_option("engine", engine)
    A, _ = o.render_host()
    B, sb = r.render_host()
    assert sb["n_invalid"] == 0 and A.shape == B.shape
    assert_image_parity(A, B, r.border, f"gaussian r={radius} {engine}")


def test_film_radius_beyond_limit_fails_loudly(renderer_factory):
    sc = scenes.cornell_box(32, 32, 1, "normals", rfilter=RFilter("gaussian", radius=9.6, stddev=2.0))
    r = renderer_factory(sc)
    with pytest.raises(NoriError, match="UNSUPPORTED|radius"):
        r.render_host()


def test_fuzz_intersect_short():
    """A few rounds of tests/fuzz_intersect.py (randomised scene shapes, all three BVH builders, bit-exact hits).
    The fuzzer exempts a mismatching ray only when the reference's own answer is ill-posed (ray within
    2e-3 rad of the triangle's plane); the exemptions are counted, logged, and on these seeds there are none."""
    from nori_amd.render import Renderer
    from tests import fuzz_intersect
    fuzz_intersect.TOLERATED[0] = 0
    hits = 0
    for seed in range(1000, 1015):
        hits += fuzz_intersect.one_round(seed, Renderer, n_rays=8000)
    print(f"[fuzz] {hits} hits bit-identical on all builders, {fuzz_intersect.TOLERATED[0]} ill-posed rays exempted")
    assert hits > 10000
    assert fuzz_intersect.TOLERATED[0] == 0, f"{fuzz_intersect.TOLERATED[0]} rays needed the ill-posed exemption"


def test_headline_workload_matches_oracle(renderer_factory):
    """BASELINE config 3 -- the bench workload: pa4 Cornell box geometry, path_mis, full 1024 x 1024 frame, at
    a sample count the CPU oracle finishes in seconds -- wavefront engine against the oracle, per-sample
    seeding, held to the SURVEY 8(d) image contract; ray counts equal.  On the host builder's tree and on the tree the
    benchmark itself renders through (builder = auto: built on the device)."""
    import os
    from nori_amd.scene import Scene
    sc = Scene.load_npz(os.path.join(os.path.dirname(__file__), "golden", "pa4-cbox-path_mis.npz"))
    assert (sc.camera.width, sc.camera.height, sc.integrator.type) == (1024, 1024, "path_mis")
    sc.sample_count = 8
    A, sa = Oracle(sc, use_bvh=True).render_host(threads=ORACLE_THREADS)      # once: the oracle's frame does not depend on the device's tree
    for builder in BUILDERS:
        r = renderer_factory(sc, builder=builder)
        assert_built_where_asked(r, builder)
        r.set_option("engine", "wavefront")
        B, sb = r.render_host()
        assert sb["n_camera_samples"] == sa["n_camera_samples"] == 1024 * 1024 * 8 and sb["n_invalid"] == 0
        for k in ("n_closest_rays", "n_shadow_rays"):
            assert int(sa[k]) == int(sb[k]), (builder, k, sa[k], sb[k])
        assert_image_parity(A, B, r.border, f"pa4-cbox-path_mis 1024x1024x8, builder {builder}")
        r.close()


def test_nori_block_seeding_zscore(renderer_factory):
    """The reference seeds ONE serial pcg32 stream per 32x32 block (src/independent.cpp:36-41); the device's
    default seeds one stream per camera sample.  Different streams, same estimator: SURVEY 8(d)'s check for
    that case -- per-pixel z-score of the oracle's NORI_SEED_NORI_BLOCK render against the GPU per-sample
    render, <= 1 % of the pixels beyond 4 sigma and the whole-image mean within 0.5 %.  The per-pixel variance of
    the mean comes from 16 independent GPU renders of spp / 16 samples each (disjoint sample indices)."""
    from nori_amd import _capi as capi
    from nori_amd.render import develop_host
    sc = scenes.cornell_box(160, 160, 64, "path_mis", rfilter=RFilter("box"))
    r, o = renderer_factory(sc), Oracle(sc, use_bvh=True)
    groups, per = 16, 4
    parts = np.stack([develop_host(r.render_host(spp_count=per, spp_begin=g * per)[0], r.border) for g in range(groups)])
    gpu = develop_host(r.render_host()[0], r.border)
    cpu = develop_host(o.render_host(seed_mode=capi.SEED_NORI_BLOCK)[0], o.border)
    lum = lambda x: x @ np.float32([0.212671, 0.715160, 0.072169])
    var_mean = lum(parts).var(axis=0, ddof=1) / groups           # variance of a 64-spp pixel mean
    z = np.abs(lum(cpu) - lum(gpu)) / np.sqrt(2.0 * var_mean + 1e-12)
    beyond = float((z > 4.0).mean())
    print(f"[parity] nori-block seeding: {beyond:.3%} of pixels beyond 4 sigma, image means {cpu.mean():.5f} / {gpu.mean():.5f}")
    assert beyond <= 0.01, beyond
    assert abs(cpu.mean() - gpu.mean()) <= 5e-3 * cpu.mean()



def test_wide_nodes_on_device(renderer_factory):
    """accel_layout = bvh4q (WIDE nodes: BVH4, quantised child boxes, the layout of scenes beyond the caches) on the
    GPU: fuzzed hit records bit-identical to the oracle's linear scan, and a render equal -- frame bits and ray counts --
    to the BVH2 layout with about half the node visits."""
    from nori_amd.render import Renderer
    from nori_amd.scene import Scene
    from tests import fuzz_intersect
    import os

    class WideRenderer(Renderer):
        def upload(self, sc, build=True, builder=0):
            self.set_option("accel_layout", "bvh4q")
            return super().upload(sc, build, builder)      # the fuzzer passes every builder: host SAH, device radix tree, device PLOC

    fuzz_intersect.TOLERATED[0] = 0
    hits = sum(fuzz_intersect.one_round(seed, WideRenderer, n_rays=8000) for seed in range(3000, 3012))
    print(f"[fuzz] wide nodes: {hits} hits bit-identical, {fuzz_intersect.TOLERATED[0]} ill-posed rays exempted")
    assert hits > 10000 and fuzz_intersect.TOLERATED[0] == 0
    sc = Scene.load_npz(os.path.join(os.path.dirname(__file__), "golden", "pa5-table_mis.npz"))
    sc.camera.width, sc.camera.height, sc.sample_count = 200, 150, 4
    a = Renderer(0); a.set_option("accel_layout", "bvh2"); a.upload(sc); a.set_option("engine", "wavefront")
    b = Renderer(0); b.set_option("accel_layout", "bvh4q"); b.upload(sc)          # engine: wide trees always take the wavefront engine
    assert a.accel_info()["node_children"] == 2 and b.accel_info()["node_children"] == 4
    A, sa = a.render_host(count_traversal=True)
    B, sb = b.render_host(count_traversal=True)
    assert np.array_equal(A, B)
    for k in ("n_closest_rays", "n_shadow_rays", "n_camera_samples"):
        assert sa[k] == sb[k], k
    assert sb["n_node_tests"] < 0.6 * sa["n_node_tests"]
    assert_image_parity(Oracle(sc, use_bvh=True).render_host()[0], B, b.border, "pa5-table_mis wide nodes")
    for builder in (1, 3):                                                                 # wide nodes emitted on the device (lbvh.hip): radix tree, PLOC
        c = Renderer(0); c.set_option("accel_layout", "bvh4q"); c.upload(sc, builder=builder)
        assert c.accel_info()["node_children"] == 4
        C_, sc_ = c.render_host()
        np.testing.assert_allclose(C_, A, rtol=1e-4, atol=1e-5)                            # same hits -> same paths; film summation order only
        assert sc_["n_closest_rays"] == sa["n_closest_rays"] and sc_["n_shadow_rays"] == sa["n_shadow_rays"]
        c.close()
    a.close(); b.close()



@pytest.mark.parametrize("integ,size,spp", [("path_mis", (72, 40), 6), ("whitted", (64, 64), 3), ("path_ems", (33, 17), 5)])
def test_nori_block_seeding_on_device(renderer_factory, integ, size, spp):
    """NORI_SEED_NORI_BLOCK on the device: one lane per 32x32 block walks the block in the reference's order with the
    block's own pcg32 stream (Independent::prepare, src/independent.cpp:36-41; renderBlock, src/main.cpp:27-56).  Same
    streams, same arithmetic as the oracle in that mode: equal ray counts, frames equal to film summation order."""
    from nori_amd import NoriError
    from nori_amd import _capi as capi
    sb = [Bsdf("mirror"), Bsdf("dielectric")] if integ != "path_ems" else [Bsdf("microfacet", (0.2, 0.3, 0.1), 0.2), Bsdf("diffuse")]
    sc = scenes.cornell_box(size[0], size[1], spp, integ, sphere_bsdfs=sb)
    r, o = renderer_factory(sc), Oracle(sc, use_bvh=True)
    A, sa = o.render_host(seed_mode=capi.SEED_NORI_BLOCK)
    B, sb_ = r.render_host(seed_mode=capi.SEED_NORI_BLOCK)
    for k in ("n_camera_samples", "n_closest_rays", "n_shadow_rays"):
        assert int(sa[k]) == int(sb_[k]), k
    assert_image_parity(A, B, r.border, f"nori-block seeding {integ} {size}")
    # and it is a different realisation than the per-sample streams
    C_, _ = r.render_host()
    assert not np.allclose(C_, B, rtol=1e-3, atol=1e-4)
    with pytest.raises(NoriError, match="UNSUPPORTED|whole frames"):
        r.render_host(seed_mode=capi.SEED_NORI_BLOCK, tile_mod=2)
    with pytest.raises(NoriError, match="UNSUPPORTED|whole frames"):
        r.render_host(seed_mode=capi.SEED_NORI_BLOCK, spp_begin=1, spp_count=2)


@pytest.mark.parametrize("engine,integ,rf,size,spp", [("wavefront", "path_mis", "gaussian", (72, 40), 6), ("megakernel", "path_ems", "mitchell", (64, 64), 5),
                                                      ("wavefront", "whitted", "tent", (33, 17), 4), ("megakernel", "normals", "box", (45, 37), 3)])
def test_reference_film_order_gives_bit_identical_frames(renderer_factory, engine, integ, rf, size, spp):
    """film_order = reference: the device adds the samples of a frame in the order of renderBlock / ImageBlock::put /
    BlockGenerator (src/main.cpp:33-53, src/block.cpp:62-152).  With bit-identical radiance per camera sample the whole
    RGBW frame -- every bit of every pixel, the W channel included -- equals a single-threaded render of the oracle;
    frame sizes that are no multiple of the 32-pixel block or the 16-pixel tile included.  Whichever builder made the tree."""
    from nori_amd import NoriError
    sb = [Bsdf("mirror"), Bsdf("dielectric")] if integ in ("whitted", "path_mis") else [Bsdf("microfacet", (0.2, 0.3, 0.1), 0.2), Bsdf("diffuse")]
    sc = scenes.cornell_box(size[0], size[1], spp, integ, sphere_bsdfs=sb, rfilter=RFilter(rf))
    A, sa = Oracle(sc, use_bvh=True).render_host(threads=1)
    for builder in BUILDERS:
        r = renderer_factory(sc, builder=builder)
        assert_built_where_asked(r, builder)
        r.set_option("engine", engine)
        r.set_option("film_order", "reference")
        B, sb_ = r.render_host()
        assert sa["n_closest_rays"] == sb_["n_closest_rays"] and sa["n_shadow_rays"] == sb_["n_shadow_rays"], builder
        assert np.array_equal(A, B), f"builder {builder}: {int((A != B).sum())} of {A.size} floats differ, max {np.abs(A - B).max():.3e}"
        with pytest.raises(NoriError, match="UNSUPPORTED|whole frames"):
            r.render_host(tile_mod=2)
        r.set_option("film_order", "fast")
        C_, _ = r.render_host()
        np.testing.assert_allclose(C_, B, rtol=1e-4, atol=1e-5)            # same samples, the fast film's summation order


def test_reference_film_order_with_the_reference_sampler(renderer_factory):
    """Both compatibility modes together: the reference's sampler streams (one pcg32 stream per 32x32 block) and the
    reference's film order -- the frame a single-threaded run of the reference's loops produces, bit for bit."""
    from nori_amd import _capi as capi
    sc = scenes.cornell_box(80, 48, 5, "path_mis", sphere_bsdfs=[Bsdf("mirror"), Bsdf("dielectric")])
    r, o = renderer_factory(sc), Oracle(sc, use_bvh=True)
    r.set_option("film_order", "reference")
    A, _ = o.render_host(seed_mode=capi.SEED_NORI_BLOCK, threads=1)
    B, _ = r.render_host(seed_mode=capi.SEED_NORI_BLOCK)
    assert np.array_equal(A, B)


def test_headline_geometry_frame_is_bit_identical_in_reference_order(renderer_factory):
    """The headline workload's scene and full 1024 x 1024 frame (1,024 blocks of 32 x 32, 4,096 tiles), 2 samples per
    pixel so that the single-threaded oracle finishes in seconds: wavefront engine + film_order = reference -> the RGBW
    frame equals the oracle's bit for bit, through the host builder's tree and through the device-built one."""
    import os
    from nori_amd.scene import Scene
    sc = Scene.load_npz(os.path.join(os.path.dirname(__file__), "golden", "pa4-cbox-path_mis.npz"))
    sc.sample_count = 2
    A, sa = Oracle(sc, use_bvh=True).render_host(threads=1)      # once: single-threaded, the expensive half
    for builder in BUILDERS:
        r = renderer_factory(sc, builder=builder)
        assert_built_where_asked(r, builder)
        r.set_option("engine", "wavefront")
        r.set_option("film_order", "reference")
        B, sb = r.render_host()
        assert sa["n_closest_rays"] == sb["n_closest_rays"] and sa["n_shadow_rays"] == sb["n_shadow_rays"], builder
        assert np.array_equal(A, B), f"builder {builder}: {int((A != B).sum())} of {A.size} floats differ"
        r.close()
