"""Delta lights without a GPU: the numpy restatement (tests/delta_lights_ref.py) against binary64 closed forms, the events and the
deliberate departures on the very inputs the GPU tests render (tests/delta_light_cases.py), the header and the bindings, the
scene's .npz form, the host's XML, and the kernels of the two new units."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi
from nori_amd.scene import Light
from tests import delta_light_cases as dc, delta_lights_ref as dl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24      # the unit roundoff of float32


# ------------------------------------------------------------------ 1. incident() against closed forms
def unit64(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def test_incident_point_and_directional_against_binary64():
    r = np.random.default_rng(1)
    p = r.uniform(-2, 2, (4000, 3)).astype(F)
    lights = [Light("point", (0.3, 1.5, -0.2), intensity=(5, 4, 3)), Light("directional", direction=(1, -2, 0.5), intensity=(1, 2, 3))]
    d, hi, R = dl.incident(lights, np.zeros(4000, np.int64), p)
    dv = np.array([0.3, 1.5, -0.2], F).astype(np.float64) - p
    dist = np.linalg.norm(dv, axis=1)
    # dvec: one rounding per component (relative u of a value below 4); dist2: three products and two sums; the root and the quotient
    # one each -- 8 u relative on every component of dir is generous, and so on maxt (whose subtraction adds u of a value below 8)
    assert np.abs(d - dv / dist[:, None]).max() <= 8 * U * 4 / dist.min()
    assert np.abs(hi - (dist - 1e-4)).max() <= 8 * U * 8
    assert (R == np.array([5, 4, 3], F)).all()
    d, hi, R = dl.incident(lights, np.ones(4000, np.int64), p)
    assert np.abs(d - -unit64([1, -2, 0.5])).max() <= 4 * U and np.isinf(hi).all() and (R == np.array([1, 2, 3], F)).all()
    assert (d == d[0]).all()      # no distance, no dependence on p
    # a point at the light: no sample, zeros
    d, hi, R = dl.incident(lights, [0], np.array([[0.3, 1.5, -0.2]], F))
    assert not d.any() and not hi.any() and not R.any()


def test_incident_spot_falloff_is_0_at_the_outer_cone_1_at_the_inner_and_monotone():
    ci, co = dc.cos_deg(20), dc.cos_deg(35)
    spot = Light("spot", (0, 2, 0), (0, -1, 0), (4, 4, 4), ci, co)
    ang = np.radians(np.linspace(0, 50, 2001))
    p = np.stack([2 * np.tan(ang), np.zeros_like(ang), np.zeros_like(ang)], 1).astype(F)      # on the plane y = 0, the angle to the axis = ang
    ok, dirs, hi, R, dist2, dist, band = dl.incident_full([spot], np.zeros(len(p), np.int64), p)
    fall = np.where(ok, R[:, 0] / F(4), 0).astype(np.float64)
    c64 = (unit64(np.array([0, 2, 0]) - p.astype(np.float64)) * -np.array([0, -1, 0.0])).sum(1)
    t = np.clip((c64 - F(co)) / (np.float64(F(ci)) - F(co)), 0, 1)
    want = t * t * (3 - 2 * t)
    # c is a dot product of unit vectors whose components carry 4 u each: 8 u absolutely is generous.  It enters t divided by the band's
    # width (the difference itself is exact to u, the quotient to u), and smoothstep's slope is 1.5 at most; its own three products and
    # one difference add 4 u.
    tol = 1.5 * (8 * U / (ci - co) + 2 * U) + 4 * U
    assert np.abs(fall - want).max() <= tol, np.abs(fall - want).max()
    assert (fall[c64 >= ci + 8 * U] == 1).all() and (fall[c64 <= co - 8 * U] == 0).all()
    assert (np.diff(fall) <= tol).all()      # monotone in the angle, up to the rounding above
    assert band.sum() > 400 and ((fall[band] > 0) & (fall[band] <= 1)).all()
    # exactly at the cones: the cones taken from the float32 c of chosen points
    c32 = dl.dot(dl.Lights([spot]).direction[[0] * len(p)], -dirs)
    a, b = 600, 1200
    edge = Light("spot", (0, 2, 0), (0, -1, 0), (4, 4, 4), float(c32[a]), float(c32[b]))
    ok, _, _, R, *_ = dl.incident_full([edge], np.zeros(len(p), np.int64), p)
    assert ok[a] and (R[a] == 4).all() and not ok[b] and ok[b - 1] and 0 < R[b - 1, 0] < 1e-3
    # a hard edge: no band, no quotient
    hard = Light("spot", (0, 2, 0), (0, -1, 0), (4, 4, 4), float(c32[a]), float(c32[a]))
    with np.errstate(all="raise", divide="ignore", invalid="ignore"):
        ok, _, _, R, _, _, band = dl.incident_full([hard], np.zeros(len(p), np.int64), p)
    assert not band.any() and ok[:a].all() and not ok[a:].any() and (R[:a] == 4).all()


# ------------------------------------------------------------------ 2. the GPU cases reach every branch; a wrong branch changes them
@pytest.fixture(scope="module")
def walked():
    """the reference of every case under path_mis, sample 0, shared"""
    return {case: dc.reference(case, "path_mis", 0) for case in dc.CASES}


def test_every_event_occurs_where_its_branch_exists_and_nowhere_else(walked):
    seen = set()
    for case, (L, nc, ns, ev) in walked.items():
        sc = dc.scene_of(case, "path_mis")
        want = dc.applicable(sc, "path_mis")
        for k in dl.EVENTS:
            paths = int((ev[k] > 0).sum())
            print(case, k, paths)
            assert (paths >= 8) if k in want else (paths == 0), (case, k, paths)
        seen |= set(want)
        assert int(ev["vertices"].max()) <= dc.LONGEST      # three quarters of the walker's cap
    assert seen == set(dl.EVENTS)
    # under path_ems the same paths draw the same picks
    L, nc, ns, ev = dc.reference("a_each_type", "path_ems", 0)
    assert all((ev[k] > 0).sum() >= 8 for k in dc.applicable(dc.scene_of("a_each_type", "path_ems"), "path_ems"))


@pytest.mark.parametrize("mutation", list(dl.MUTATIONS))
def test_each_departure_changes_the_radiance_of_paths_the_gpu_renders(walked, mutation):
    assert set(dc.SHOWN_ON) == set(dl.MUTATIONS)
    for case in dc.SHOWN_ON[mutation]:
        L, nc, ns, ev = walked[case]
        M, mc, ms, _ = dc.walk(case, "path_mis", 0, mutate=mutation)
        changed = (L.view(np.uint32) != M.view(np.uint32)).any(axis=1)
        names = dl.MUTATIONS[mutation]
        counter = sum(ev[k] for k in ((names,) if isinstance(names, str) else names))
        print(mutation, case, int(changed.sum()), "paths change;", int((counter > 0).sum()), "carry the counter")
        assert changed.sum() >= 8, (mutation, case)
        assert (counter[changed] > 0).all(), (mutation, case)      # only paths that took the branch can change


def test_path_ems_equals_path_mis_where_delta_lights_are_the_only_lights():
    a, b = dc.reference("e_lights_only", "path_ems", 0), dc.reference("e_lights_only", "path_mis", 0)
    assert a[0].tobytes() == b[0].tobytes() and a[1:3] == b[1:3] and (a[0] > 0).any()


# ------------------------------------------------------------------ 3. the header and the bindings
NEW = ("nori_hip_set_lights", "nori_hip_get_lights", "nori_hip_light_incident", "nori_hip_group_set_lights")


def test_bindings_declare_every_new_entry_point_with_the_headers_arity():
    text = open(os.path.join(ROOT, "include", "nori_hip.h")).read()
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_capi.HIP_PROTOTYPES[name][1]), name
    body = re.search(r"typedef struct nori_light_desc \{(.*?)\} nori_light_desc;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])?[;,]", body)
    assert [f for f, _ in _capi.LightDesc._fields_] == names == ["type", "position", "direction", "intensity", "cos_inner", "cos_outer"]
    assert C.sizeof(_capi.LightDesc) == 48
    enum = re.search(r"typedef enum nori_light_type \{(.*?)\}", text, re.S).group(1)
    assert [(n.lower(), int(v)) for n, v in re.findall(r"NORI_LIGHT_(\w+) = (\d+)", enum)] == list(zip(_capi.LIGHT_TYPES, range(3)))
    assert int(re.search(r"#define NORI_MAX_LIGHTS\s+(\d+)", text).group(1)) == _capi.MAX_LIGHTS == 4096
    # appended after the medium's section; the ABI version is the one it was
    assert text.index("int nori_hip_group_set_medium(") < text.index("typedef struct nori_light_desc")
    assert re.search(r"#define NORI_HIP_ABI_VERSION\s+8\b", text)
    types = open(os.path.join(ROOT, "nori_amd", "csrc", "device", "rt_types.h")).read()
    assert "sizeof(LightRec) == 48" in types
    path = open(os.path.join(ROOT, "nori_amd", "csrc", "device", "rt_path.h")).read()
    assert re.search(r"constexpr int kDeltaLit = 0x80;", path)
    lib = _capi.load_hip()
    for name in NEW:
        assert getattr(lib, name)


# ------------------------------------------------------------------ 4. the scene's .npz form
def test_scene_carries_lights_and_a_scene_without_them_is_saved_as_before(tmp_path):
    from nori_amd.scene import Scene
    golden = os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz")
    sc = Scene.load_npz(golden)
    assert sc.lights == []
    sc.save_npz(str(tmp_path / "plain.npz"))
    a, b = np.load(golden), np.load(str(tmp_path / "plain.npz"))
    assert sorted(a.files) == sorted(b.files) and all(a[k].tobytes() == b[k].tobytes() for k in a.files)      # the meta JSON included, key for key
    sc.lights = [dc.POINT, dc.SPOT, dc.SUN]
    d = dc.SPOT.desc()
    assert d.type == 1 and list(d.position) == [F(x) for x in dc.SPOT.position] and d.cos_inner == F(dc.SPOT.cos_inner) and d.cos_outer == F(dc.SPOT.cos_outer)
    assert dc.SUN.desc().type == 2 and dc.POINT.desc().type == 0
    sc.save_npz(str(tmp_path / "lit.npz"))
    back = Scene.load_npz(str(tmp_path / "lit.npz"))
    assert back.lights == sc.lights
    c = np.load(str(tmp_path / "lit.npz"))
    assert sorted(c.files) == sorted(a.files) and all(a[k].tobytes() == c[k].tobytes() for k in a.files if k != "meta")
    assert Light.from_desc(d) == Light("spot", tuple(float(F(x)) for x in dc.SPOT.position), tuple(float(F(x)) for x in dc.SPOT.direction),
                                       tuple(float(F(x)) for x in dc.SPOT.intensity), float(F(dc.SPOT.cos_inner)), float(F(dc.SPOT.cos_outer)))


# ------------------------------------------------------------------ 5. the host: <emitter type="point|spot|directional">
XML = """<scene><integrator type="%s"/>
  <sampler type="independent"><integer name="sampleCount" value="2"/></sampler>
  <camera type="perspective"><integer name="width" value="24"/><integer name="height" value="17"/><float name="fov" value="50"/>
    <transform name="toWorld"><lookat target="0, 0.5, 0" origin="0, 1, 4" up="0, 1, 0"/></transform></camera>
  <mesh type="obj"><string name="filename" value="floor.obj"/><bsdf type="diffuse"/></mesh>
  %s
</scene>"""
PT = '<emitter type="point"><point name="position" value="0.5, 2, -1"/><color name="intensity" value="3, 2, 1"/></emitter>'
PW = '<emitter type="point"><point name="position" value="0, 1, 0"/><color name="power" value="8, 4, 2"/></emitter>'
SP = ('<emitter type="spot"><point name="position" value="0, 3, 0"/><vector name="direction" value="0, -2, 0"/><color name="intensity" value="5, 5, 5"/>'
      '<float name="cutoffAngle" value="30"/><float name="beamWidth" value="20"/></emitter>')
ST = '<emitter type="spot"><point name="position" value="1, 3, 0"/><point name="target" value="0, 0, 0.5"/><color name="intensity" value="1, 1, 1"/></emitter>'
DR = '<emitter type="directional"><vector name="direction" value="0.2, -1, 0.1"/><color name="irradiance" value="2, 2, 1.5"/></emitter>'
FOG = '<medium type="homogeneous"><float name="sigmaT" value="0.4"/></medium>'


def write_scene(tmp_path, name, integrator, body):
    (tmp_path / "floor.obj").write_text("v -3 0 -3\nv -3 0 3\nv 3 0 3\nv 3 0 -3\nf 1 2 3 4\n")
    (tmp_path / name).write_text(XML % (integrator, body))
    return str(tmp_path / name)


def test_host_reads_the_three_lights(tmp_path):
    from nori_amd import host
    sc = host.HostRoot(write_scene(tmp_path, "a.xml", "path_mis", PT + PW + SP + ST + DR)).scene()
    f = lambda *v: tuple(float(F(x)) for x in v)
    assert [l.type for l in sc.lights] == ["point", "point", "spot", "spot", "directional"]
    assert sc.lights[0] == Light("point", f(0.5, 2, -1), intensity=f(3, 2, 1))
    k = F(0.31830988618379067154) * F(0.25)      # I = power (kInvPi 0.25f), float32
    assert sc.lights[1].intensity == tuple(float(F(x) * k) for x in (8, 4, 2)) and abs(sc.lights[1].intensity[0] - 8 / (4 * np.pi)) < 1e-6
    assert sc.lights[2] == Light("spot", f(0, 3, 0), f(0, -2, 0), f(5, 5, 5), float(F(np.cos(np.radians(20.0)))), float(F(np.cos(np.radians(30.0)))))
    assert sc.lights[3].direction == f(-1, -3, 0.5)      # target - position
    assert sc.lights[3].cos_outer == float(F(np.cos(np.radians(20.0)))) and sc.lights[3].cos_inner == float(F(np.cos(np.radians(15.0))))      # the defaults: 20 and 3/4 of it
    assert sc.lights[4] == Light("directional", direction=f(0.2, -1, 0.1), intensity=f(2, 2, 1.5))
    assert host.HostRoot(write_scene(tmp_path, "b.xml", "path_mis", "")).scene().lights == []
    fog = host.HostRoot(write_scene(tmp_path, "c.xml", "path_ems", PT + SP + FOG)).scene()      # point and spot light a medium
    assert len(fog.lights) == 2 and fog.medium is not None


@pytest.mark.parametrize("integrator, body, word", [
    ("path_mats", PT, "path_ems and path_mis only"),
    ("whitted", DR, "path_ems and path_mis only"),
    ("path_mis", DR + FOG, "directional light cannot light a medium"),
    ("path_mis", PT.replace("3, 2, 1", "3, -2, 1"), "finite and not negative"),
    ("path_mis", DR.replace("0.2, -1, 0.1", "0, 0, 0"), "non-zero length"),
    ("path_mis", SP.replace('value="20"', 'value="40"'), "beamWidth must lie in"),
    ("path_mis", SP.replace('value="30"', 'value="200"'), "cutoffAngle must lie in"),
    ("path_mis", PW.replace("</emitter>", '<color name="intensity" value="1, 1, 1"/></emitter>'), "intensity or power, not both"),
])
def test_cli_rejects_bad_lights_before_a_device_is_asked_for(tmp_path, integrator, body, word):
    from nori_amd import host
    path = write_scene(tmp_path, "bad.xml", integrator, body)
    exe = os.path.join(_capi.LIB_DIR, "nori")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # no device: a refusal must come from the parse
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=env)
    out = p.stdout + p.stderr
    assert p.returncode != 0 and word in out, out
    with pytest.raises(Exception, match=word):
        host.HostRoot(path)


# ------------------------------------------------------------------ 6. the kernels of the new units
@pytest.fixture(scope="module")
def light_unit_kernels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as ge
    from kernel_resources import kernels
    rows = {}
    for unit in ("wavefront_lights.hip", "lights.hip"):
        assert unit in ge.HIP_SOURCES
        out = tmp_path_factory.mktemp("asm") / (unit + ".s")
        flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")]
        p = subprocess.run([ge.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(ge.DEV, unit), "-o", str(out)], capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        rows[unit] = {r["demangled"].replace("(anonymous namespace)::", "").replace("nrt::", "").split("(")[0]: r for r in kernels(str(out))}
    return rows


def test_light_kernels_are_three_sets_for_two_integrators(light_unit_kernels):
    """wavefront_lights.hip holds wf_shade / wf_finish for MATSET 159 = every BSDF | textured | delta lights, 191 = that with an
    environment and 223 = that with a medium, and nothing else: two integrators x three modes x two table places, and two tails, per
    set.  wf_shade stays within 128 VGPRs without scratch (four workgroups of 256 per CU, as every wf_shade); wf_finish may keep the
    few bytes of scratch its neighbours have (wavefront_medium.hip: 20)."""
    rows = light_unit_kernels["wavefront_lights.hip"]
    want = {f"void wf_shade<{i}, {m}, {t}, {s}>" for s in (159, 191, 223) for i in (5, 6) for m in (0, 1, 2) for t in ("true", "false")}
    want |= {f"void wf_finish<{i}, {s}>" for s in (159, 191, 223) for i in (5, 6)}
    assert set(rows) == want, sorted(set(rows) ^ want)
    for name, k in rows.items():
        print(name, {x: k[x] for x in ("vgpr", "sgpr", "scratch", "lds")})
        assert k["vgpr"] <= 128 and k["agpr"] == 0, (name, k)
        if "wf_shade" in name:
            assert k["scratch"] == 0, (name, k)
        else:
            assert k["scratch"] <= 32, (name, k)
    twins = light_unit_kernels["lights.hip"]
    assert set(twins) == {"light_incident_kernel"}
    for name, k in twins.items():
        assert k["scratch"] == 0 and k["lds"] == 0, (name, k)
