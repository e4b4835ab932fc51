"""The grid medium without a GPU: the numpy restatement (tests/grid_medium_ref.py) against binary64 closed forms, the branches the
adversarial rays of tests/grid_medium_cases.py reach, the departures the walker's paths show, the header and the bindings, the
scene's .npz form, and the kernels of the two new units."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi
from tests import grid_medium_cases as gc, grid_medium_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24
INF = F(np.inf)


def np_log(x):
    return np.log(np.asarray(x, np.float64)).astype(F)


def np_exp(x):
    return np.exp(np.asarray(x, np.float64)).astype(F)


# ------------------------------------------------------------------ 1. closed forms
def slab_rays(n=512, seed=1):
    """rays that cross the box (-1, -1, -1) .. (1, 1, 1) from its face x = -1 to its face x = 1"""
    r = np.random.default_rng(seed)
    a, b = r.uniform(-0.5, 0.5, (n, 2)), r.uniform(-0.5, 0.5, (n, 2))
    o = np.concatenate([np.full((n, 1), -3.0), a * 2 - (b - a)], 1)      # the line through (-1, a) and (1, b), from x = -3
    d = np.concatenate([np.full((n, 1), 2.0), b - a], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F), d.astype(F)


def test_optical_depth_through_two_slabs_against_the_closed_form():
    """Two voxels in x, each 1 thick, sigma 0.7 and 2.2: tau = (0.7 + 2.2) / |d_x| for a ray that crosses both.  u = 2^-24.  A
    crossing t = (plane - o) inv carries the difference's, the reciprocal's and the product's rounding, 3 u of |t| <= 5: 15 u
    absolutely; a length is the difference of two, 30 u plus its own u, over a length of at least 1; sigma = sigma_scale rho, the
    product sigma len and the sum add one u each: 35 u relatively, 40 allowed."""
    rho = np.array([0.7, 2.2], F).reshape(1, 1, 2)
    g = gr.Grid(rho, (-1, -1, -1), (1, 1, 1), 1.0)
    o, d = slab_rays()
    tau, steps = gr.optical_depth(g, o, d, INF)
    assert (steps == 2).all()
    want = (float(rho[0, 0, 0]) + float(rho[0, 0, 1])) / np.abs(d[:, 0].astype(np.float64))
    rel = np.abs(tau.astype(np.float64) / want - 1)
    print("largest deviation", rel.max() / U, "u of 40")
    assert rel.max() <= 40 * U
    # a tmax inside the first slab: sigma_1 (tmax - t_in); and transmittance = exp(-tau), 1 exactly for a miss
    t_in = (-1.0 - o[:, 0].astype(np.float64)) / d[:, 0].astype(np.float64)
    tmax = (t_in + 0.5).astype(F)
    tau1, steps1 = gr.optical_depth(g, o, d, tmax)
    assert (steps1 == 1).all() and np.abs(tau1 / (float(rho[0, 0, 0]) * (tmax.astype(np.float64) - t_in)) - 1).max() <= 80 * U      # (a length of 0.5: twice the 30 u)
    tr = gr.transmittance(g, np.concatenate([o, o]), np.concatenate([d, -d]), INF, np_exp)
    assert (tr[512:] == 1).all() and np.abs(tr[:512] / np.exp(-want) - 1).max() <= 40 * U * want.max() + 2 * U


@pytest.mark.parametrize("name", [n for n in gc.GRIDS if n not in gc.TIE_GRIDS])      # (the tie grids are all but empty)
def test_distance_inverts_the_optical_depth(name):
    """tau(s(xi)) = -log(1 - xi) where there is an event.  s = (t_cur + (tau_stop - tau) / sigma) + 0 carries three roundings of
    its own, 3 u s, on top of t_cur's 15 u (above); walked again up to s, every whole segment carries the 35 u of above and the last
    one ends at s: |tau(s) - tau_stop| <= 40 u tau_stop + sigma_max (45 u + 6 u s), all crossings |t| <= 8 here."""
    g = gr.as_grid(gc.grid(name))
    o, d, tmax, xi = gc.rays(name)
    unit = np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1) < 1e-3      # (the bound is stated for unit directions)
    s, ev = gr.distance(g, o, d, tmax, xi, np_log)
    ev = ev & unit & (s > 0)
    assert ev.sum() > 150
    assert (s[ev] <= tmax[ev] * (1 + 4 * U)).all()
    tau, steps = gr.optical_depth(g, o[ev], d[ev], s[ev])
    stop = (-np_log(F(1.0) - xi[ev])).astype(np.float64)
    smax = float(g.sigma_scale) * float(g.rho.max())
    bound = 40 * U * stop + smax * (45 * U + 6 * U * s[ev].astype(np.float64))
    err = np.abs(tau.astype(np.float64) - stop)
    print(name, "events", int(ev.sum()), "largest error / bound", (err / bound).max())
    assert (err <= bound).all()


def test_a_walk_never_takes_more_than_nx_ny_nz_trips_and_every_branch_occurs():
    total = {k: 0 for k in gr.BRANCHES}
    n_rays = 0
    for name in gc.GRIDS:
        g = gr.as_grid(gc.grid(name))
        o, d, tmax, xi = gc.rays(name)
        n_rays += o.shape[0]
        tau, s, ev, steps, br = gr.grid_walk(g, o, d, tmax, (-np_log(F(1.0) - xi)).astype(F))      # (asserts the bound itself, too)
        assert steps.max() <= int(g.n.sum()) and (steps[br["miss"] | br["parallel_outside"]] == 0).all()
        assert (tau >= 0).all() and np.isfinite(tau).all() and np.isfinite(s[ev]).all() and np.isinf(s[~ev]).all()
        for k in gr.BRANCHES:
            total[k] += int(br[k].sum())
    print(n_rays, "rays", total)
    assert 3500 <= n_rays <= 8000      # (about 1170 per grid: four grids of the kinds the twins are asked on, two where a tie's order shows)
    assert all(v >= 8 for v in total.values()), total
    # the special values are among them
    o, d, tmax, xi = gc.rays("g235")
    assert (xi == 0).sum() >= 8 and (xi == gc.XI_MAX).sum() >= 8 and np.isinf(tmax).sum() >= 8 and (np.signbit(d) & (d == 0)).sum() >= 8


def test_the_walks_departures_show_on_the_adversarial_rays():
    """Accumulating the crossings instead of indexing them changes tau or s.  The ORDER of a tie decides which voxel is crossed over
    a length of zero, and that shows in one situation only: tau_stop equals the tau accumulated so far (xi = 0 before any density),
    where a voxel that is not empty gives an event even over a length of zero.  grid_medium_cases.tie_rays builds it: under the
    pinned order x, y, z every such ray has its event AT the tie; stepped z-first it has none.  The twins of the GPU suite run
    the same rays, so the device is held to the order."""
    changed = {"accumulate_boundaries": 0}
    for name in gc.GRIDS:
        g = gr.as_grid(gc.grid(name))
        o, d, tmax, xi = gc.rays(name)
        stop = (-np_log(F(1.0) - xi)).astype(F)
        tau, s, ev, steps, _ = gr.grid_walk(g, o, d, tmax, stop)
        a = gr.grid_walk(g, o, d, tmax, stop, "accumulate_boundaries")
        changed["accumulate_boundaries"] += int(((a[0].view(np.uint32) != tau.view(np.uint32)) | (a[1].view(np.uint32) != s.view(np.uint32))).sum())
    print(changed)
    assert changed["accumulate_boundaries"] >= 8
    for name, families in (("gtie_x", 3), ("gtie_y", 1)):
        g = gr.as_grid(gc.grid(name))
        o, d, tmax, xi = gc.tie_rays(name)
        assert o.shape[0] == 16 * families and (xi == 0).all()
        _, s, ev, steps, br = gr.grid_walk(g, o, d, tmax, np.zeros(o.shape[0], F))
        a = -o.max(axis=1)                                  # the distance to the tie: the components that tie are -a and 1
        assert ev.all() and (s == a).all() and (steps == 2).all(), name
        assert (br["tie_of_two"] | br["tie_of_three"]).all()
        _, sz, evz, stepsz, _ = gr.grid_walk(g, o, d, tmax, np.zeros(o.shape[0], F), "ties_z_first")
        differ = int(((sz.view(np.uint32) != s.view(np.uint32)) | (evz != ev)).sum())
        print(name, "ties z-first changes", differ, "of", o.shape[0], "rays; voxels visited", sorted(set(stepsz.tolist())))
        assert differ == o.shape[0] and not evz.any()
        # and they are among the rays the twins run
        ro = gc.rays(name)[0]
        assert ro[-o.shape[0]:].tobytes() == o.tobytes()


# ------------------------------------------------------------------ 2. the walker's departures on the test scenes
@pytest.mark.parametrize("mutate", ["no_tr_on_emitter_samples", "tr_over_unclipped_distance", "medium_vertex_whenever_not_found", "accumulate_boundaries"])
def test_a_departure_changes_paths_of_the_test_scenes(mutate):
    changed = 0
    for case in ("box_lit", "r3_lit"):
        base = gc.reference(case, "path_mis", 3)[0]
        L = gc.walk(case, "path_mis", 3, mutate=mutate)[0]
        changed += int((L.view(np.uint32) != base.view(np.uint32)).any(axis=1).sum())
    print(mutate, changed, "paths change")
    assert changed >= 8


def test_the_scenes_paths_reach_the_medium_in_every_way():
    for case in gc.CASES:
        for integrator in gc.integrators(case):
            L, nc, ns, ev = gc.reference(case, integrator, 3)
            n_med = ev["medium_vertex"]
            assert (n_med > 0).sum() >= 50 and (n_med == 0).sum() >= 50 and np.isfinite(L).all(), (case, integrator)
            # rays that miss the grid, enter it, start in it, and -- the box is open -- leave the scene through it
            counts = {k: int((v > 0).sum()) for k, v in ev.items()}
            print(case, integrator, counts)
            assert all(counts[k] >= 8 for k in ("miss", "enter_from_outside", "start_inside")), (case, integrator, counts)
            assert counts["left_scene_through_grid"] >= 8 or case.startswith("r3"), (case, integrator, counts)
    g = gr.as_grid(gc.scene_of("box_g06", "path_mis").medium)
    assert (g.rho == 0).sum() >= 3 and tuple(g.n) == (2, 3, 5)


# ------------------------------------------------------------------ 3. the header, the bindings, the .npz form
NEW = ("nori_hip_set_grid_medium", "nori_hip_get_grid_medium", "nori_hip_grid_medium_distance", "nori_hip_grid_medium_transmittance",
       "nori_hip_grid_medium_optical_depth", "nori_hip_group_set_grid_medium")


def test_bindings_declare_every_new_entry_point_with_the_headers_arity():
    text = open(os.path.join(ROOT, "include", "nori_hip.h")).read()
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_capi.HIP_PROTOTYPES[name][1]), name
    body = re.search(r"typedef struct nori_grid_medium_desc \{(.*?)\} nori_grid_medium_desc;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)(?:\[\d+\])?[,;]", body)
    assert [f for f, _ in _capi.GridMediumDesc._fields_] == fields == ["rho", "nx", "ny", "nz", "bmin", "bmax", "sigma_scale", "albedo", "g"]
    assert C.sizeof(_capi.GridMediumDesc) == 8 + 3 * 4 + 6 * 4 + 4 + 3 * 4 + 4
    # appended after the lights' section; the ABI version and nori_medium_desc are the ones they were
    assert text.index("int nori_hip_group_set_lights(") < text.index("typedef struct nori_grid_medium_desc")
    assert re.search(r"#define NORI_HIP_ABI_VERSION\s+8\b", text)
    assert C.sizeof(_capi.MediumDesc) == 5 * 4
    for word in ("PIECEWISE CONSTANT", "INTEGER plane index", "x, then y, then z", "nx + ny + nz", "2^-40", "NAMED BY ITS INDEX", "Coincidence"):
        assert word in text, word
    lib = _capi.load_hip()
    for name in NEW:
        assert getattr(lib, name)


def test_scene_carries_a_grid_medium_and_a_scene_without_one_is_saved_as_before(tmp_path):
    from nori_amd.scene import GridMedium, Medium, Scene
    golden = os.path.join(ROOT, "tests", "golden", "pa4-cbox-path_mis.npz")
    sc = Scene.load_npz(golden)
    sc.save_npz(str(tmp_path / "plain.npz"))
    a, b = np.load(golden), np.load(str(tmp_path / "plain.npz"))
    assert sorted(a.files) == sorted(b.files) and all(a[k].tobytes() == b[k].tobytes() for k in a.files)
    sc.medium = gc.box_grid()
    d = sc.medium.desc()
    assert (d.nx, d.ny, d.nz) == (2, 3, 5) and d.sigma_scale == F(2.0) and list(d.bmin) == [F(-0.4), F(0.15), F(-0.7)] and d.g == F(0.6)
    assert d.rho == sc.medium.rho.ctypes.data and sc.medium.rho.flags["C_CONTIGUOUS"]
    sc.save_npz(str(tmp_path / "grid.npz"))
    back = Scene.load_npz(str(tmp_path / "grid.npz"))
    assert isinstance(back.medium, GridMedium) and back.medium == sc.medium and back.medium != gc.box_grid(0.0)
    c = np.load(str(tmp_path / "grid.npz"))
    assert sorted(set(c.files) - {"grid_medium_rho"}) == sorted(a.files) and all(a[k].tobytes() == c[k].tobytes() for k in a.files if k != "meta")
    sc.medium = Medium(0.4)      # a homogeneous medium is saved as it was
    sc.save_npz(str(tmp_path / "fog.npz"))
    assert Scene.load_npz(str(tmp_path / "fog.npz")).medium == Medium(0.4)


# ------------------------------------------------------------------ 3b. the host: <medium type="grid"> and the VOL file
GRID = '<medium type="grid"><string name="filename" value="%s"/><float name="sigmaScale" value="%s"/><color name="albedo" value="%s"/>%s</medium>'
HG = '<phase type="hg"><float name="g" value="%s"/></phase>'
SUN = '<emitter type="directional"><vector name="direction" value="0.2, -0.6, -0.8"/><color name="irradiance" value="1.5, 1.4, 1.2"/></emitter>'
VOL_RHO = np.random.default_rng(4).uniform(0.5, 2.0, (5, 3, 2)).astype(F)      # (nz, ny, nx)
VOL_RHO[1, 2, 0] = 0
VOL_BOX = ((-2.0, 0.25, -2.0), (2.0, 1.75, 2.0))


def write_vol(path, rho=VOL_RHO, box=VOL_BOX, magic=b"VOL\x03", encoding=1, channels=1, cut=0):
    """the common VOL layout, little-endian: 'V' 'O' 'L', version 3, int32 encoding (1: float32), nx ny nz, channels, the box, the voxels"""
    nz, ny, nx = rho.shape
    data = magic + np.array([encoding, nx, ny, nz, channels], "<i4").tobytes() + np.array(box, "<f4").tobytes() + rho.astype("<f4").tobytes()
    with open(path, "wb") as f:
        f.write(data[:len(data) - cut])


def write_grid_scene(tmp_path, name, integrator="path_mis", medium=None, extra=""):
    from tests.test_medium_cpu import write_scene
    if medium is None:
        medium = GRID % ("cloud.vol", "1.5", "0.9, 0.6, 0.3", HG % "0.6")
    if not (tmp_path / "cloud.vol").exists():
        write_vol(str(tmp_path / "cloud.vol"))
    return write_scene(tmp_path, name, integrator, medium + extra)


def test_host_reads_a_grid_medium_from_a_vol_file(tmp_path):
    from nori_amd import host
    from nori_amd.scene import GridMedium
    root = host.HostRoot(write_grid_scene(tmp_path, "a.xml"))
    sc = root.scene()
    want = GridMedium(VOL_RHO, VOL_BOX[0], VOL_BOX[1], float(F(1.5)), (float(F(0.9)), float(F(0.6)), float(F(0.3))), float(F(0.6)))
    assert isinstance(sc.medium, GridMedium) and sc.medium == want
    # boxMin / boxMax override the file's box; no <phase>: isotropic; sigmaScale and albedo default to 1
    over = '<medium type="grid"><string name="filename" value="cloud.vol"/><point name="boxMin" value="-1, 0, -1"/><point name="boxMax" value="1, 1.5, 3"/></medium>'
    m = host.HostRoot(write_grid_scene(tmp_path, "b.xml", medium=over)).medium()
    assert m == GridMedium(VOL_RHO, (-1.0, 0.0, -1.0), (1.0, 1.5, 3.0), 1.0, (1.0, 1.0, 1.0), 0.0)
    # a directional light beside a grid medium is read; beside the homogeneous medium it is refused, as before
    lit = host.HostRoot(write_grid_scene(tmp_path, "c.xml", extra=SUN)).scene()
    assert isinstance(lit.medium, GridMedium) and [l.type for l in lit.lights] == ["directional"]
    from tests.test_medium_cpu import MEDIUM
    with pytest.raises(Exception, match="directional light cannot light a medium that fills all space"):
        host.HostRoot(write_grid_scene(tmp_path, "d.xml", medium=MEDIUM % ("1", "1, 1, 1", ""), extra=SUN))
    # the C entry points: the homogeneous one says none for a grid, and the other way round
    from tests.test_medium_cpu import write_scene
    fog = host.HostRoot(write_scene(tmp_path, "e.xml"))
    d, gd = _capi.MediumDesc(), _capi.GridMediumDesc()
    assert root._lib.nori_host_medium(root._h, C.byref(d)) == 0 and root._lib.nori_host_grid_medium(root._h, C.byref(gd)) == 1
    assert (gd.nx, gd.ny, gd.nz) == (2, 3, 5) and gd.rho
    assert fog._lib.nori_host_medium(fog._h, C.byref(d)) == 1 and fog._lib.nori_host_grid_medium(fog._h, C.byref(gd)) == 0 and not gd.rho


def _bad_vols(tmp_path):
    bad = VOL_RHO.copy(); bad[2, 1, 1] = -1.0      # voxel (1, 1, 2): index (2 * 3 + 1) * 2 + 1 = 15
    nan = VOL_RHO.copy(); nan[0, 0, 0] = np.nan
    write_vol(str(tmp_path / "magic.vol"), magic=b"VOX\x03")
    write_vol(str(tmp_path / "version.vol"), magic=b"VOL\x02")
    write_vol(str(tmp_path / "half.vol"), encoding=2)
    write_vol(str(tmp_path / "rgb.vol"), channels=3)
    write_vol(str(tmp_path / "short.vol"), cut=8)
    write_vol(str(tmp_path / "wide.vol"), rho=np.ones((1, 1, 257), F))
    write_vol(str(tmp_path / "flat.vol"), box=((0, 0, 0), (1, 0, 1)))
    write_vol(str(tmp_path / "neg.vol"), rho=bad)
    write_vol(str(tmp_path / "nan.vol"), rho=nan)


G1 = '<medium type="grid"><string name="filename" value="%s"/>%s</medium>'


@pytest.mark.parametrize("integrator, medium, word", [
    ("path_mis", G1 % ("none.vol", ""), "cannot open"),
    ("path_mis", G1 % ("magic.vol", ""), "not a VOL file of version 3"),
    ("path_mis", G1 % ("version.vol", ""), "not a VOL file of version 3"),
    ("path_mis", G1 % ("half.vol", ""), "encoding 2"),
    ("path_mis", G1 % ("rgb.vol", ""), "3 channels"),
    ("path_mis", G1 % ("short.vol", ""), "ends before"),
    ("path_mis", G1 % ("wide.vol", ""), "1 .. 256"),
    ("path_mis", G1 % ("flat.vol", ""), "boxMin < boxMax"),
    ("path_mis", G1 % ("cloud.vol", '<point name="boxMax" value="-3, 1, 1"/>'), "boxMin < boxMax"),
    ("path_mis", G1 % ("neg.vol", ""), "voxel 15"),
    ("path_mis", G1 % ("nan.vol", ""), "voxel 0"),
    ("path_mis", G1 % ("cloud.vol", '<float name="sigmaScale" value="1e5"/>'), "voxel 0"),
    ("path_mis", G1 % ("cloud.vol", '<float name="sigmaScale" value="-1"/>'), "sigmaScale"),
    ("path_mis", G1 % ("cloud.vol", '<color name="albedo" value="1, 1.5, 1"/>'), "albedo"),
    ("path_mis", G1 % ("cloud.vol", HG % "0.995"), "g must lie"),
    ("whitted", G1 % ("cloud.vol", ""), "path_mats, path_ems and path_mis"),
    ("path_mis", G1 % ("cloud.vol", "") + G1 % ("cloud.vol", ""), "one medium"),
])
def test_cli_rejects_a_bad_grid_medium_before_a_device_is_asked_for(tmp_path, integrator, medium, word):
    from nori_amd import host
    _bad_vols(tmp_path)
    path = write_grid_scene(tmp_path, "bad.xml", integrator, medium)
    exe = os.path.join(_capi.LIB_DIR, "nori")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # no device: a refusal must come from the parse
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=env)
    out = p.stdout + p.stderr
    assert p.returncode != 0 and word in out, out
    with pytest.raises(Exception, match=re.escape(word)):
        host.HostRoot(path)


# ------------------------------------------------------------------ 4. the kernels of the new units
@pytest.fixture(scope="module")
def grid_unit_kernels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as ge
    from kernel_resources import kernels
    rows = {}
    procs = []
    for unit in ("wavefront_grid_medium.hip", "grid_medium.hip"):
        assert unit in ge.HIP_SOURCES
        out = tmp_path_factory.mktemp("asm") / (unit + ".s")
        flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")]
        procs.append((unit, out, subprocess.Popen([ge.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(ge.DEV, unit), "-o", str(out)],
                                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for unit, out, p in procs:
        log = p.communicate(timeout=900)[0]
        assert p.returncode == 0, log[-3000:]
        rows[unit] = {r["demangled"].replace("(anonymous namespace)::", "").replace("nrt::", "").split("(")[0]: r for r in kernels(str(out))}
    return rows


def test_grid_medium_kernels_are_two_sets_within_the_budget(grid_unit_kernels):
    """wavefront_grid_medium.hip holds wf_shade / wf_finish for MATSET 351 = every BSDF | textured | medium | grid (three integrators)
    and 479 = that | delta lights (path_ems, path_mis) and nothing else; wf_shade fits 128 VGPRs without scratch, wf_finish carries
    the 20 B of scratch its homogeneous neighbours carry."""
    rows = grid_unit_kernels["wavefront_grid_medium.hip"]
    sets = [(i, 351) for i in (4, 5, 6)] + [(i, 479) for i in (5, 6)]
    want = {f"void wf_shade<{i}, {m}, {t}, {s}>" for i, s in sets for m in (0, 1, 2) for t in ("true", "false")} | {f"void wf_finish<{i}, {s}>" for i, s in sets}
    assert set(rows) == want, sorted(set(rows) ^ want)
    for name, k in rows.items():
        print(name, {x: k[x] for x in ("vgpr", "sgpr", "scratch", "lds")})
        assert k["agpr"] == 0, (name, k)
        if "wf_shade" in name:
            assert k["vgpr"] <= 128 and k["scratch"] == 0, (name, k)      # four workgroups of 256 per CU, as every wf_shade
        else:
            assert k["scratch"] <= 20, (name, k)
    twins = grid_unit_kernels["grid_medium.hip"]
    assert set(twins) == {"grid_medium_kernel"}
    assert twins["grid_medium_kernel"]["scratch"] == 0 and twins["grid_medium_kernel"]["lds"] == 0
