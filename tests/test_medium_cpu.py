"""The homogeneous medium without a GPU: the numpy restatement (tests/medium_ref.py) against closed forms -- the phase function
integrates to 1 and has mean cosine g, its sampler follows it, free-flight distances have mean 1 / sigma_t --, the header and the
bindings, the scene's .npz form, the host's XML, and the kernels of the two new units."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi
from tests import medium_ref as mr, stat_harness as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GS = (0.0, 0.6, -0.7, 0.99)


def np_sincos(x):
    x = np.asarray(x, np.float64)
    return np.sin(x).astype(F), np.cos(x).astype(F)


def np_log(x):
    return np.log(np.asarray(x, np.float64)).astype(F)


def axis_dirs():
    d = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], F)
    r = np.random.default_rng(3).normal(size=(50, 3))
    return np.concatenate([d, (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F)])


# ------------------------------------------------------------------ 1. the phase function
@pytest.mark.parametrize("g", GS + (1e-3, 0.0005, -0.99))
def test_hg_integrates_to_one_and_has_mean_cosine_g(g):
    m = mr.Medium(1.0, (1, 1, 1), g)
    assert m.g == (0 if abs(g) < 1e-3 else F(g))
    # over the sphere: 2 pi int_{-1}^{1} HG(c) dc, by Gauss-Legendre on 64 panels that shrink geometrically towards the peak
    # (|g| = 0.99 peaks like (1 - |c|)^-1.5), in binary64 from the float32 density at float32 cosines
    x, w = np.polynomial.legendre.leggauss(32)
    edges = 1.0 - np.geomspace(2.0, 1e-9, 65)
    edges[0], edges[-1] = -1.0, 1.0
    c = np.concatenate([(a + b) / 2 + (b - a) / 2 * x for a, b in zip(edges[:-1], edges[1:])])
    wt = np.concatenate([(b - a) / 2 * w for a, b in zip(edges[:-1], edges[1:])])
    g64 = float(m.g)
    if g64 < 0:
        c = -c
    c32 = c.astype(F)
    p = mr.hg_eval(m, c32).astype(np.float64)
    exact = lambda cc: (1 - g64 * g64) / (4 * np.pi * (1 + g64 * g64 - 2 * g64 * cc) ** 1.5)
    # the quadrature itself, on the exact density
    assert abs(2 * np.pi * (wt * exact(c)).sum() - 1) < 1e-9 and abs(2 * np.pi * (wt * exact(c) * c).sum() - g64) < 1e-9
    # the float32 density at a float32 cosine.  u = 2^-24.  k = B - G2 c carries three absolute errors of at most 2 u each (B's own
    # rounding, the product's, the difference's) and enters as k^-1.5; A = 1 - g g carries u absolutely; the product, the root, the
    # product k sqrt(k) and the quotient one u each, relatively.  The cosine's own rounding moves the exact density by
    # 1.5 G2 u / k relatively.
    u = 2.0 ** -24
    k = 1 + g64 * g64 - 2 * g64 * c
    rel = 1.5 * 6 * u / k + u / (1 - g64 * g64) + 4 * u + 1.5 * 2 * abs(g64) * u / k
    assert (np.abs(p / exact(c) - 1) <= rel).all()
    bound = 2 * np.pi * (wt * exact(c) * rel).sum()
    assert bound < (3e-3 if abs(g64) > 0.9 else 2e-5)      # (what the format allows: k falls to 1e-4 at |g| = 0.99, where 8 u / k is 0.5 %)
    assert abs(2 * np.pi * (wt * p).sum() - 1) <= bound + 1e-9
    assert abs(2 * np.pi * (wt * p * c).sum() - g64) <= bound + 1e-9
    if m.g == 0:
        assert (mr.hg_eval(m, c.astype(F)) == mr.KINVFOURPI).all()


@pytest.mark.parametrize("g", GS)
def test_hg_sample_follows_hg_eval(g):
    """chi^2 on 20 bins of the cosine x 10 of the azimuth, the expected frequencies from HG's closed-form CDF; sample count and
    generator as the environment map's sampler test has them.  (At g = 0.99 the last cosine bin is 94 float32 steps of the cosine
    wide, so up to half a percent of its samples sit on the other side of a binary64 edge: at this count a sixth of a cell's
    standard deviation.  A first version drew 200000 numbers from a generator whose RAW numbers, binned 20 x 10 before any warp,
    already stood at p = 0.019.)"""
    m = mr.Medium(1.0, (1, 1, 1), g)
    n = 100000
    rng = np.random.default_rng(12)
    xi = rng.random((n, 2), dtype=F)
    d = np.broadcast_to(np.array([0.36, -0.48, 0.8], F), (n, 3))
    wo, pdf = mr.hg_sample(m, d, xi, np_sincos)
    assert np.abs(np.linalg.norm(wo.astype(np.float64), axis=1) - 1).max() < 1e-5
    assert pdf.tobytes() == mr.hg_eval(m, mr.dot(d, wo)).tobytes()
    s, t = mr.coordinate_system(d)
    c = np.clip(mr.dot(d, wo).astype(np.float64), -1, 1)
    phi = np.arctan2(mr.dot(wo, t).astype(np.float64), mr.dot(wo, s).astype(np.float64)) % (2 * np.pi)
    assert abs(c.mean() - float(m.g)) < 4 / np.sqrt(n)      # the mean cosine is g (a cosine's standard deviation is below 1)
    g64 = float(m.g)

    def cdf(x):      # P(cos <= x)
        if g64 == 0:
            return (x + 1) / 2
        return (1 - g64 * g64) / (2 * g64) * (1 / np.sqrt(1 + g64 * g64 - 2 * g64 * x) - 1 / (1 + g64))

    # equal-probability cosine bins: the inverse of the CDF in binary64
    u = np.linspace(0, 1, 21)
    if g64 == 0:
        edges = 2 * u - 1
    else:
        sq = (1 - g64 * g64) / (1 - g64 + 2 * g64 * u)
        edges = (1 + g64 * g64 - sq * sq) / (2 * g64)
    assert np.abs(cdf(edges) - u).max() < 1e-9
    ci = np.clip(np.searchsorted(edges, c, side="right") - 1, 0, 19)
    pj = np.minimum((phi / (2 * np.pi) * 10).astype(np.int64), 9)
    obs = np.bincount(ci * 10 + pj, minlength=200).astype(np.float64)
    ok, info = sh.chi2_test(obs, np.full(200, n / 200.0), n, 5, 0.01, len(GS))
    assert ok, (g, info)


def test_distance_has_mean_one_over_sigma_t():
    n = 400000
    xi = np.random.default_rng(5).random(n, dtype=F)
    for sigma in (0.4, 7.0):
        m = mr.Medium(sigma, (1, 1, 1))
        s = mr.distance(m, xi, np_log).astype(np.float64)
        assert (s >= 0).all() and np.isfinite(s).all()
        assert abs(s.mean() * sigma - 1) < 4 / np.sqrt(n)      # an exponential's standard deviation equals its mean
    z = mr.distance(m, np.array([0.0], F), np_log)
    assert z[0] == 0 and not np.signbit(z[0])      # xi = 0: +0
    tr = mr.transmittance(m, np.array([0.0, 1.0], F), lambda x: np.exp(x.astype(np.float64)).astype(F))
    assert tr[0] == 1 and abs(tr[1] / np.exp(-7.0) - 1) < 1e-6


def test_default_transcendentals_are_the_pinned_ones():
    from tests.backends import Oracle
    x = np.array([0.25, 1.0, 3.0], F)
    assert mr.default_log(x).tobytes() == Oracle.libm("log", x).tobytes() and mr.default_exp(-x).tobytes() == Oracle.libm("exp", -x).tobytes()
    sn, cs = mr.default_sincos(x)
    assert sn.tobytes() == Oracle.libm("sin", x).tobytes() and cs.tobytes() == Oracle.libm("cos", x).tobytes()


# ------------------------------------------------------------------ 2. the header and the bindings
NEW = ("nori_hip_set_medium", "nori_hip_get_medium", "nori_hip_medium_distance", "nori_hip_medium_transmittance", "nori_hip_phase_eval",
       "nori_hip_phase_sample", "nori_hip_group_set_medium")


def test_bindings_declare_every_new_entry_point_with_the_headers_arity():
    text = open(os.path.join(ROOT, "include", "nori_hip.h")).read()
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_capi.HIP_PROTOTYPES[name][1]), name
    body = re.search(r"typedef struct nori_medium_desc \{(.*?)\} nori_medium_desc;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [f for f, _ in _capi.MediumDesc._fields_] == re.findall(r"(\w+)(?:\[\d+\])?;", body) == ["sigma_t", "albedo", "g"]
    assert C.sizeof(_capi.MediumDesc) == 5 * 4
    # appended after the environment's section; the ABI version is the one it was
    assert text.index("int nori_hip_group_set_environment(") < text.index("typedef struct nori_medium_desc")
    assert re.search(r"#define NORI_HIP_ABI_VERSION\s+8\b", text)
    assert "first SURFACE" in text      # the feature pass is said to be unchanged
    lib = _capi.load_hip()
    for name in NEW:
        assert getattr(lib, name)


# ------------------------------------------------------------------ 3. the scene's .npz form
def test_scene_carries_a_medium_and_a_scene_without_one_is_saved_as_before(tmp_path):
    from nori_amd.scene import Medium, Scene
    golden = os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz")
    sc = Scene.load_npz(golden)
    assert sc.medium is None
    sc.save_npz(str(tmp_path / "plain.npz"))
    a, b = np.load(golden), np.load(str(tmp_path / "plain.npz"))
    assert sorted(a.files) == sorted(b.files) and all(a[k].tobytes() == b[k].tobytes() for k in a.files)      # the meta JSON included, key for key
    sc.medium = Medium(0.4, (0.9, 0.6, 0.3), 0.6)
    d = sc.medium.desc()
    assert d.sigma_t == F(0.4) and list(d.albedo) == [F(0.9), F(0.6), F(0.3)] and d.g == F(0.6)
    sc.save_npz(str(tmp_path / "fog.npz"))
    back = Scene.load_npz(str(tmp_path / "fog.npz"))
    assert back.medium == sc.medium
    c = np.load(str(tmp_path / "fog.npz"))
    assert sorted(c.files) == sorted(a.files) and all(a[k].tobytes() == c[k].tobytes() for k in a.files if k != "meta")
    assert Medium(1.0).g == 0 and Medium(1.0).albedo == (1.0, 1.0, 1.0)


# ------------------------------------------------------------------ 4. the host: <medium> and <phase>
XML = """<scene><integrator type="%s"/>
  <sampler type="independent"><integer name="sampleCount" value="2"/></sampler>
  <camera type="perspective"><integer name="width" value="24"/><integer name="height" value="17"/><float name="fov" value="50"/>
    <transform name="toWorld"><lookat target="0, 0.5, 0" origin="0, 1, 4" up="0, 1, 0"/></transform></camera>
  <mesh type="obj"><string name="filename" value="floor.obj"/><bsdf type="diffuse"/></mesh>
  <mesh type="obj"><string name="filename" value="light.obj"/><emitter type="area"><color name="radiance" value="8, 8, 8"/></emitter></mesh>
  %s
</scene>"""
MEDIUM = '<medium type="homogeneous"><float name="sigmaT" value="%s"/><color name="albedo" value="%s"/>%s</medium>'
HG = '<phase type="hg"><float name="g" value="%s"/></phase>'


def write_scene(tmp_path, name, integrator="path_mis", medium=MEDIUM % ("0.4", "0.9, 0.6, 0.3", HG % "0.6")):
    (tmp_path / "floor.obj").write_text("v -3 0 -3\nv -3 0 3\nv 3 0 3\nv 3 0 -3\nf 1 2 3 4\n")
    (tmp_path / "light.obj").write_text("v -1 2 -1\nv 1 2 -1\nv 1 2 1\nv -1 2 1\nf 1 2 3 4\n")
    (tmp_path / name).write_text(XML % (integrator, medium))
    return str(tmp_path / name)


def test_host_reads_a_medium(tmp_path):
    from nori_amd import host
    from nori_amd.scene import Medium
    sc = host.HostRoot(write_scene(tmp_path, "a.xml")).scene()
    assert sc.medium == Medium(float(F(0.4)), (float(F(0.9)), float(F(0.6)), float(F(0.3))), float(F(0.6)))
    iso = host.HostRoot(write_scene(tmp_path, "b.xml", medium=MEDIUM % ("2", "1, 1, 1", '<phase type="isotropic"/>'))).medium()
    assert iso == Medium(2.0, (1.0, 1.0, 1.0), 0.0)
    none = host.HostRoot(write_scene(tmp_path, "c.xml", medium=MEDIUM % ("2", "0.5, 0.5, 0.5", ""))).medium()
    assert none.g == 0 and none.albedo == (0.5, 0.5, 0.5)
    assert host.HostRoot(write_scene(tmp_path, "d.xml", medium="")).scene().medium is None


@pytest.mark.parametrize("integrator, medium, word", [
    ("path_mis", MEDIUM % ("0", "1, 1, 1", ""), "sigmaT"),
    ("path_mis", MEDIUM % ("1e5", "1, 1, 1", ""), "sigmaT"),
    ("path_mis", MEDIUM % ("1", "1, 1.5, 1", ""), "albedo"),
    ("path_mis", MEDIUM % ("1", "1, 1, 1", HG % "0.995"), "g must lie"),
    ("path_mis", MEDIUM % ("1", "1, 1, 1", HG % "-1"), "g must lie"),
    ("whitted", MEDIUM % ("1", "1, 1, 1", ""), "path_mats, path_ems and path_mis"),
    ("path_mis", MEDIUM % ("1", "1, 1, 1", "") + MEDIUM % ("1", "1, 1, 1", ""), "one medium"),
])
def test_cli_rejects_a_bad_medium_before_a_device_is_asked_for(tmp_path, integrator, medium, word):
    from nori_amd import host
    path = write_scene(tmp_path, "bad.xml", integrator, medium)
    exe = os.path.join(_capi.LIB_DIR, "nori")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # no device: a refusal must come from the parse
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=env)
    out = p.stdout + p.stderr
    assert p.returncode != 0 and word in out, out
    with pytest.raises(Exception, match=word):
        host.HostRoot(path)


# ------------------------------------------------------------------ 5. the kernels of the new units
@pytest.fixture(scope="module")
def medium_unit_kernels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as ge
    from kernel_resources import kernels
    rows = {}
    for unit in ("wavefront_medium.hip", "medium.hip"):
        assert unit in ge.HIP_SOURCES
        out = tmp_path_factory.mktemp("asm") / (unit + ".s")
        flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")]
        p = subprocess.run([ge.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(ge.DEV, unit), "-o", str(out)], capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        rows[unit] = {r["demangled"].replace("(anonymous namespace)::", "").replace("nrt::", "").split("(")[0]: r for r in kernels(str(out))}
    return rows


def test_medium_kernels_are_one_variant_per_integrator(medium_unit_kernels):
    """wavefront_medium.hip holds wf_shade / wf_finish for MATSET 95 = every BSDF | textured | medium and nothing else: three
    integrators x three modes x two table places, and three tails.  (wavefront.hip's own set is pinned by tests/test_lens_cpu.py.)"""
    rows = medium_unit_kernels["wavefront_medium.hip"]
    want = {f"void wf_shade<{i}, {m}, {t}, 95>" for i in (4, 5, 6) for m in (0, 1, 2) for t in ("true", "false")} | {f"void wf_finish<{i}, 95>" for i in (4, 5, 6)}
    assert set(rows) == want, sorted(set(rows) ^ want)
    for name, k in rows.items():
        print(name, {x: k[x] for x in ("vgpr", "sgpr", "scratch", "lds")})
        assert k["vgpr"] <= 128 and k["agpr"] == 0, (name, k)      # four workgroups of 256 per CU, as every wf_shade
    twins = medium_unit_kernels["medium.hip"]
    assert set(twins) == {"medium_scalar_kernel", "medium_phase_kernel"}
    for name, k in twins.items():
        assert k["scratch"] == 0 and k["lds"] == 0, (name, k)
