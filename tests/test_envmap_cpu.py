"""The environment-map emitter without a GPU: the numpy restatement (tests/envmap_ref.py) against its own scalar statement, the
geometry of the octahedral map, the density's normalisation, the bindings, the kernels the new units compile to, and the host's
XML."""
from __future__ import annotations

import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi
from tests import envmap_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 7, 64)


# ------------------------------------------------------------------ 1. the restatement against a scalar per-direction loop
@pytest.mark.parametrize("kind", ["random", "zeros", "range"])
def test_restatement_equals_the_scalar_statement(kind):
    n = 7
    env = er.EnvRef(er.make_map(n, kind), (0.5, 1.25, 2.0), er.rotation())
    d = er.directions(300)
    d = (d.astype(np.float64) @ env.m.astype(np.float64).T).astype(np.float32)      # the seams are the LOCAL frame's
    le, pdf, (i, j) = env.eval(d)
    for k in range(d.shape[0]):
        le1, pdf1, (i1, j1) = er.eval_scalar(env, d[k])
        assert (i1, j1) == (i[k], j[k]) and le1.tobytes() == le[k].tobytes() and np.float32(pdf1).tobytes() == pdf[k].tobytes(), k
    xi = er.samples(env, 300)
    ds, les, pdfs, (si, sj) = env.sample(xi)
    for k in range(xi.shape[0]):
        d1, le1, pdf1, (i1, j1) = er.sample_scalar(env, xi[k])
        assert (i1, j1) == (si[k], sj[k]), (k, xi[k])
        assert d1.tobytes() == ds[k].tobytes() and le1.tobytes() == les[k].tobytes() and np.float32(pdf1).tobytes() == pdfs[k].tobytes(), (k, xi[k])
    assert np.isfinite(ds).all() and np.isfinite(pdfs).all() and (pdfs >= 0).all()
    # the tables are DiscretePDFs: non-decreasing from 0 to 1; a row without light keeps its zeros and is never chosen
    assert (np.diff(env.row_cdf) >= 0).all() and env.row_cdf[0] == 0 and env.row_cdf[-1] == 1
    lit = env.col_cdf[:, -1] > 0
    assert (np.diff(env.col_cdf, axis=1) >= 0).all() and (env.col_cdf[lit, -1] == 1).all() and (env.col_cdf[~lit] == 0).all()
    assert (np.diff(env.row_cdf)[~lit] == 0).all()
    # a random sample lands in the texel the CDFs chose; the boundary values may land next to it (sample reuse gives 0 or 1 there)
    # or, on the square's outer edge, in the texel the fold identifies that edge with -- which is why the density returned is the
    # final direction's
    _, _, (ei, ej) = env.eval(ds)
    off = (ei != si) | (ej != sj)
    assert off[:300].mean() < 0.02 and off.mean() < 0.25


def test_constant_map_is_close_to_the_uniform_sphere():
    """A constant map.  Sampling is uniform over a texel's square, not over its solid angle, so inside a texel the density follows
    |q|^3 while the weight took |c|^3 at the centre: pdf 4 pi = |q|^3 / |c|^3 up to the tables' one-point quadrature.  On a face
    n = |q|^2 has the gradient 2 (x - z, y - z) in (px, py), at most 2 sqrt(2) (at a vertex, where n = 1), so ln |q|^3 changes by at
    most 1.5 * 2 sqrt(2) per unit; a texel's half diagonal is sqrt(2) / N: a factor exp(6 / N), and 1 % for the quadrature."""
    n = 64
    env = er.EnvRef(np.full((n, n, 3), 0.7, np.float32))
    _, pdf, _ = env.eval(er.directions(2000))
    dev = np.abs(pdf.astype(np.float64) * 4 * np.pi - 1)
    assert dev.max() < np.exp(6 / n) * 1.01 - 1 and dev.mean() < 0.04


# ------------------------------------------------------------------ 2. texel centre -> direction -> the same texel
@pytest.mark.parametrize("n", SIZES)
def test_texel_centres_round_trip(n):
    env = er.EnvRef(er.make_map(n), to_world=er.rotation(9))
    local = env.texel_centre_dirs().reshape(-1, 3)
    d = (local @ env.m.astype(np.float64).T).astype(np.float32)
    _, _, (i, j) = env.eval(d)
    jj, ii = np.divmod(np.arange(n * n), n)
    assert np.array_equal(i, ii) and np.array_equal(j, jj)
    # and the directions cover the sphere: every octant (the four centres of N = 2 lie on the equator, z = 0)
    if n >= 7:
        assert len({tuple(s) for s in np.sign(local).astype(int) if 0 not in s}) == 8


# ------------------------------------------------------------------ 3. the density integrates to 1
@pytest.mark.parametrize("kind,n", [("contrast", 7), ("random", 7), ("random", 2), ("zeros", 7), ("random", 1)])
def test_density_integrates_to_one(kind, n):
    """Midpoint rule on a latitude-longitude grid of 384 x 768 cells (a parametrisation the map knows nothing of), d omega =
    sin(theta) d theta d phi.  The integrand is smooth inside a texel (proportional to |q|^3) and jumps at texel borders, so the
    error has two parts.  A cell that a border crosses -- found by looking up the texel at the cell's 9 half-step points -- can be
    wrong by at most the spread of the density over those points times its solid angle.  Inside a texel the midpoint rule's
    relative error is h^2 / 24 times the integrand's relative second derivative; |q|^3 varies by 3^1.5 over an octant face, second derivative below 40 in relative
    terms, h = pi / 384: below 2e-4."""
    env = er.EnvRef(er.make_map(n, kind), (1.0, 0.5, 0.25), er.rotation(3))
    nt, nphi = 384, 768
    th = np.arange(2 * nt + 1) * (np.pi / (2 * nt))            # half steps: odd indices are cell centres
    ph = np.arange(2 * nphi + 1) * (np.pi / nphi)
    st, ct = np.sin(th)[:, None], np.cos(th)[:, None]
    d = np.stack([st * np.cos(ph)[None, :], ct + 0 * ph[None, :], st * np.sin(ph)[None, :]], axis=-1).astype(np.float32)
    _, pdf, (i, j) = env.eval(d.reshape(-1, 3))
    pdf, tex = pdf.reshape(2 * nt + 1, 2 * nphi + 1).astype(np.float64), (j * n + i).reshape(2 * nt + 1, 2 * nphi + 1)
    dw = (np.cos(th[0:-1:2]) - np.cos(th[2::2]))[:, None] * (2 * np.pi / nphi)      # exact solid angle of a cell
    assert abs(dw.sum() * nphi - 4 * np.pi) < 1e-9
    total = (pdf[1::2, 1::2] * dw).sum()
    crossed = np.zeros((nt, nphi), bool)
    lo, hi = pdf[1::2, 1::2].copy(), pdf[1::2, 1::2].copy()
    for a in range(3):
        for b in range(3):
            crossed |= tex[a:2 * nt - 1 + a:2, b:2 * nphi - 1 + b:2] != tex[1::2, 1::2]
            lo, hi = np.minimum(lo, pdf[a:2 * nt - 1 + a:2, b:2 * nphi - 1 + b:2]), np.maximum(hi, pdf[a:2 * nt - 1 + a:2, b:2 * nphi - 1 + b:2])
    bound = ((hi - lo) * crossed * dw).sum() + 2e-4
    print(f"{kind} N={n}: integral {total:.6f}, bound {bound:.4f} ({crossed.mean():.2%} of the cells crossed)")
    assert bound < 0.1 and abs(total - 1.0) <= bound      # (0.08 for the map with a sun: the worst case along the sun's border; 0.01 - 0.02 else)
    # the sampling side of the same statement: the mean of 1 / pdf over samples is the sphere's 4 pi (only texels with light are hit)
    _, le, p, _ = env.sample(np.random.default_rng(0).random((20000, 2), dtype=np.float32))
    assert (p > 0).all() and (le.max(axis=1) > 0).all()


# ------------------------------------------------------------------ 4. the bindings
NEW = ("nori_hip_set_environment", "nori_hip_get_environment", "nori_hip_env_eval", "nori_hip_env_sample", "nori_hip_debug_env_tables",
       "nori_hip_group_set_environment")


def test_bindings_declare_every_new_entry_point_with_the_headers_arity():
    text = open(os.path.join(ROOT, "include", "nori_hip.h")).read()
    assert re.search(r"#define NORI_HIP_ABI_VERSION 8\b", text) and _capi.HIP_ABI_VERSION == 8
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_capi.HIP_PROTOTYPES[name][1]), name
    # the struct: uint32, pointer, 3 + 9 floats, in the header's order
    body = re.search(r"typedef struct nori_env_desc \{(.*?)\} nori_env_desc;", text, re.S).group(1)
    assert [f for f, _ in _capi.EnvDesc._fields_] == re.findall(r"(\w+)(?:\[\d+\])?;", body) == ["size", "texels", "scale", "to_world"]
    import ctypes as C
    assert C.sizeof(_capi.EnvDesc) == 8 + 8 + 12 * 4
    # appended: nothing declared before them moved (the lens's entry points are still where they were, the group's last)
    assert text.index("int nori_hip_group_render_host(") < text.index("typedef struct nori_env_desc")


def test_scene_carries_an_environment(tmp_path):
    from nori_amd.scene import Environment, Scene
    sc = Scene.load_npz(os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz"))
    assert sc.environment is None
    sc.environment = Environment(er.make_map(7), (1, 2, 3), er.rotation())
    d = sc.environment.desc()
    assert d.size == 7 and list(d.scale) == [1, 2, 3] and np.allclose(np.array(d.to_world).reshape(3, 3), er.rotation())
    sc.save_npz(str(tmp_path / "e.npz"))
    back = Scene.load_npz(str(tmp_path / "e.npz"))
    assert back.environment.texels.tobytes() == sc.environment.texels.tobytes() and tuple(back.environment.scale) == (1, 2, 3)
    assert back.environment.to_world.tobytes() == sc.environment.to_world.tobytes()
    with pytest.raises(AssertionError):
        Environment(np.zeros((3, 4, 3), np.float32))


# ------------------------------------------------------------------ 5. the kernels of the new units
@pytest.fixture(scope="module")
def env_unit_kernels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as ge
    from kernel_resources import kernels
    rows = {}
    for unit in ("wavefront_env.hip", "env_map.hip"):
        assert unit in ge.HIP_SOURCES
        out = tmp_path_factory.mktemp("asm") / (unit + ".s")
        flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")]
        p = subprocess.run([ge.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(ge.DEV, unit), "-o", str(out)], capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        rows[unit] = {r["demangled"].replace("(anonymous namespace)::", "").replace("nrt::", "").split("(")[0]: r for r in kernels(str(out))}
    return rows


def test_environment_kernels_are_one_variant_per_integrator(env_unit_kernels):
    """wavefront_env.hip holds wf_shade / wf_finish for MATSET 63 = every BSDF | textured | environment and nothing else: three
    integrators x three modes x two table places, and three tails.  (wavefront.hip's own set is pinned by tests/test_lens_cpu.py.)"""
    rows = env_unit_kernels["wavefront_env.hip"]
    want = {f"void wf_shade<{i}, {m}, {t}, 63>" for i in (4, 5, 6) for m in (0, 1, 2) for t in ("true", "false")} | {f"void wf_finish<{i}, 63>" for i in (4, 5, 6)}
    assert set(rows) == want, sorted(set(rows) ^ want)
    for name, k in rows.items():
        print(name, {x: k[x] for x in ("vgpr", "sgpr", "scratch", "lds")})
        assert k["vgpr"] <= 128 and k["agpr"] == 0, (name, k)      # four workgroups of 256 per CU, as every wf_shade
    tables = env_unit_kernels["env_map.hip"]
    assert set(tables) == {"env_weight_kernel", "env_row_cdf_kernel", "env_rows_kernel", "env_eval_kernel", "env_sample_kernel"}
    for name, k in tables.items():
        assert k["scratch"] == 0 and k["lds"] == 0, (name, k)


# ------------------------------------------------------------------ 6. the host: <emitter type="envmap"> as a child of <scene>
XML = """<scene><integrator type="%s"/>
  <sampler type="independent"><integer name="sampleCount" value="2"/></sampler>
  <camera type="perspective"><integer name="width" value="24"/><integer name="height" value="17"/><float name="fov" value="50"/>
    <transform name="toWorld"><lookat target="0, 0.5, 0" origin="0, 1, 4" up="0, 1, 0"/></transform></camera>
  <mesh type="obj"><string name="filename" value="floor.obj"/><bsdf type="diffuse"/></mesh>
  %s
</scene>"""
ENV = '<emitter type="envmap"><string name="filename" value="%s"/>%s</emitter>'


def latlong_image(h=16, w=32):
    """a sky: brighter towards +y, a warm spot around +x"""
    from nori_amd import host
    theta = (np.arange(h) + 0.5) / h * np.pi
    phi = ((np.arange(w) + 0.5) / w - 0.5) * 2 * np.pi
    y = np.cos(theta)[:, None] + 0 * phi[None, :]
    x = np.sin(theta)[:, None] * np.sin(phi)[None, :]
    img = np.stack([0.2 + 0.8 * np.maximum(y, 0) + 4 * np.maximum(x, 0) ** 8, 0.3 + 0.7 * np.maximum(y, 0), 0.5 + 0.5 * np.maximum(y, 0)], axis=-1)
    return img.astype(np.float32), host


def write_scene(tmp_path, name, integrator="path_mis", props="", filename="sky.exr", extra=""):
    (tmp_path / "floor.obj").write_text("v -3 0 -3\nv -3 0 3\nv 3 0 3\nv 3 0 -3\nf 1 2 3 4\n")
    (tmp_path / name).write_text(XML % (integrator, ENV % (filename, props) + extra))
    return str(tmp_path / name)


def test_host_reads_an_environment_map(tmp_path):
    img, host = latlong_image()
    host.save_images(str(tmp_path / "sky"), img)
    root = host.HostRoot(write_scene(tmp_path, "a.xml", props='<integer name="resolution" value="8"/><color name="scale" value="1, 0.5, 2"/>'))
    sc = root.scene()
    env = sc.environment
    assert env.texels.shape == (8, 8, 3) and tuple(env.scale) == (1.0, 0.5, 2.0) and np.array_equal(env.to_world, np.eye(3, dtype=np.float32))
    # the resampling: a texel holds the image's value in its centre's direction (bilinear: within the image's variation nearby)
    d = er.EnvRef(env.texels).texel_centre_dirs()
    want_r = 0.2 + 0.8 * np.maximum(d[..., 1], 0) + 4 * np.maximum(d[..., 0], 0) ** 8
    assert np.abs(env.texels[..., 0] - want_r).max() < 0.5 and np.abs(env.texels[..., 1] - (0.3 + 0.7 * np.maximum(d[..., 1], 0))).max() < 0.08
    # the default resolution, a rotation
    r2 = host.HostRoot(write_scene(tmp_path, "b.xml", props='<transform name="toWorld"><rotate axis="0, 1, 0" angle="90"/></transform>'))
    e2 = r2.environment()
    assert e2.texels.shape == (512, 512, 3)
    assert np.allclose(e2.to_world, [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-6)
    # a scene without one: none, as ever
    (tmp_path / "c.xml").write_text(XML % ("path_mis", ""))
    assert host.HostRoot(str(tmp_path / "c.xml")).scene().environment is None


@pytest.mark.parametrize("integrator, props, filename, extra, word", [
    ("path_mis", "", "missing.exr", "", "missing.exr"),
    ("path_mis", "", "sky.png", "", "OpenEXR"),
    ("path_mis", '<integer name="resolution" value="0"/>', "sky.exr", "", "resolution"),
    ("path_mis", '<integer name="resolution" value="4097"/>', "sky.exr", "", "resolution"),
    ("path_mis", '<color name="scale" value="1, -1, 1"/>', "sky.exr", "", "scale"),
    ("path_mis", '<color name="scale" value="0, 0, 0"/>', "sky.exr", "", "black"),
    ("path_mis", '<transform name="toWorld"><scale value="2, 1, 1"/></transform>', "sky.exr", "", "rotation"),
    ("whitted", "", "sky.exr", "", "whitted"),
    ("path_mis", "", "sky.exr", ENV % ("sky.exr", ""), "one environment map"),
    ("path_mis", "", "sky.exr", '<emitter type="area"><color name="radiance" value="1, 1, 1"/></emitter>', "area lights"),
])
def test_cli_rejects_a_bad_environment_before_a_device_is_asked_for(tmp_path, integrator, props, filename, extra, word):
    img, host = latlong_image()
    host.save_images(str(tmp_path / "sky"), img)
    path = write_scene(tmp_path, "bad.xml", integrator, props, filename, extra)
    exe = os.path.join(_capi.LIB_DIR, "nori")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # no device: a refusal must come from the parse
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=env)
    out = p.stdout + p.stderr
    assert p.returncode != 0 and word in out and "device" not in out.lower().replace("devices", ""), out
    with pytest.raises(Exception, match=word):
        host.HostRoot(path)


def test_cli_accepts_an_environment_and_only_then_asks_for_a_device(tmp_path):
    """without a GPU the good scene parses -- the configuration is printed with the map in it -- and fails where the render starts"""
    img, host = latlong_image()
    host.save_images(str(tmp_path / "sky"), img)
    path = write_scene(tmp_path, "good.xml", props='<integer name="resolution" value="16"/>')
    exe = os.path.join(_capi.LIB_DIR, "nori")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=env)
    out = p.stdout + p.stderr
    assert "Reading a 32x16 OpenEXR file" in out, out
    assert p.returncode != 0 and not os.path.exists(str(tmp_path / "good.exr")), out
