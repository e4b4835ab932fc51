"""The first pass by per-tile candidate lists (nori_amd/csrc/device/wavefront_first.hip, first_lists.h) against the first pass it
replaces, wf_extend<..., kFreshOnly, ...>: a camera ray tested against a superset of the pair records its walk could accept returns
the walk's hit, so EVERY BIT of the bordered RGBW frame and the ray counts must be equal.

The switches are read once per process, so every variant renders all cases of this file in a child process of its own:
NORI_HIP_WF_FIRST=0 (the old first pass), =2 (the lists, whatever share of the tiles overflows), =2 with NORI_HIP_WF_FIRST_K=0 (every
tile overflows: the generic walk in the new kernel) and with K=1, and the default (the lists unless more than one of the call's tiles in
sixteen overflows).  With NORI_HIP_CENSUS set the engine says on stderr which first pass ran and how many tiles were on lists; the children print a marker per case, so the lines can be told apart."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import workloads
from nori_amd.scene import Integrator
from tests import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_KEYS = ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid")
SIZES = ((64, 64), (40, 24))      # 4 x 4 whole tiles; 3 x 2 tiles whose edge tiles hang over the image
SPP = 4
DEFAULT_K = int(re.search(r"kFirstListDefaultK = (\d+)u", open(os.path.join(ROOT, "nori_amd", "csrc", "device", "first_lists.h")).read()).group(1))
# NORI_HIP_WF_FIRST=2: the lists whatever share of the tiles overflows; the default ("auto") keeps the old kernel above one tile in sixteen
VARIANTS = {"old": {"NORI_HIP_WF_FIRST": "0"}, "lists": {"NORI_HIP_WF_FIRST": "2"}, "k0": {"NORI_HIP_WF_FIRST": "2", "NORI_HIP_WF_FIRST_K": "0"},
            "k1": {"NORI_HIP_WF_FIRST": "2", "NORI_HIP_WF_FIRST_K": "1"}, "auto": {}}


def cbox(size, integrator, spp=SPP):
    return scenes.cornell_box(size[0], size[1], spp, integrator)


def dense(size, integrator, spp=SPP):
    """the Cornell box with finely tessellated spheres (2 x 5120 triangles): tiles on them overflow, the others keep lists"""
    return scenes.cornell_box(size[0], size[1], spp, integrator, sphere_subdiv=4)


def bunny(size, integrator, spp=SPP):
    sc = workloads.load("c1-bunny-normals", size[0], size[1], spp).scene
    sc.integrator = Integrator(integrator)
    return sc


def cases():
    """[(key, scene, options, render_host's keywords or {"tiles": [...]}, lens radius, the first pass the default must take)]"""
    out = []
    for name, make in (("cbox", cbox), ("dense", dense)):
        for size in SIZES:
            for integ in ("path_mis", "normals"):
                out.append((f"{name}-{size[0]}x{size[1]}-{integ}", make(size, integ), {}, {}, 0.0, "lists"))
    out.append(("bunny-64x64-normals", bunny((64, 64), "normals"), {}, {}, 0.0, "lists"))
    out.append(("bunny-40x24-path_mis", bunny((40, 24), "path_mis"), {}, {}, 0.0, "lists"))
    out.append(("tile-list", cbox((64, 64), "path_mis"), {}, {"tiles": [1, 2, 5, 10, 15], "spp_begin": 3}, 0.0, "lists"))
    out.append(("tile-list-dense", dense((40, 24), "normals"), {}, {"tiles": [0, 2, 4, 5]}, 0.0, "lists"))
    # two batches of two samples per pixel each
    out.append(("batches", cbox((64, 64), "path_mis"), {"wavefront_samples": 16 * 256 * 2}, {}, 0.0, "lists"))
    # regeneration: a pool of 2048 paths under a batch of the whole frame -- new paths start behind stored ones (n_f0 > 0)
    out.append(("pool", dense((64, 64), "path_mis"), {"wavefront_paths": 2048, "wavefront_samples": 1 << 30}, {}, 0.0, "lists"))
    out.append(("pool-tiles", cbox((40, 24), "path_mis"), {"wavefront_paths": 1024, "wavefront_samples": 1 << 30}, {"tile_mod": 2, "tile_rem": 1}, 0.0, "lists"))
    # frames on which the default rule must take the lists: 256 tiles of which the spheres put about 8 on overflow (at most 16 may be);
    # 64 tiles of coarse spheres (80 triangles each), none on overflow; and a share of the first frame's tiles
    out.append(("cbox-256x256-path_mis", scenes.cornell_box(256, 256, 2, "path_mis"), {}, {}, 0.0, "lists"))
    out.append(("cbox-128x128-coarse-normals", scenes.cornell_box(128, 128, 2, "normals", sphere_subdiv=1), {}, {}, 0.0, "lists"))
    out.append(("cbox-256x256-share", scenes.cornell_box(256, 256, 2, "path_mis"), {}, {"tile_mod": 3, "tile_rem": 1}, 0.0, "lists"))
    # a lens: the old kernel, whatever the switch says
    out.append(("lens", cbox((64, 64), "path_mis"), {}, {}, 0.05, "walk"))
    return out


_CASES = cases()
KEYS = [c[0] for c in _CASES]
EXPECTED = {c[0]: c[5] for c in _CASES}
AUTO_MUST_LIST = ("cbox-256x256-path_mis", "cbox-128x128-coarse-normals")      # the default rule takes the lists there, with list tiles
TILES = {c[0]: ((c[1].camera.width + 15) // 16) * ((c[1].camera.height + 15) // 16) for c in _CASES}


def render_cases(out_dir):
    """Every case through the wavefront engine, the device's builder (the tree a context builds by default): <key>.npy and
    stats.json in out_dir; a marker per case on stderr.  Then one context through two uploads (cache invalidation)."""
    from nori_amd.render import Renderer
    stats = {}
    for key, scene, options, kw, lens, _ in _CASES:
        sys.stderr.write(f"\nCASE {key}\n"); sys.stderr.flush()
        r = Renderer(0).upload(scene, builder=2)
        r.set_option("engine", "wavefront")
        for k, v in options.items():
            r.set_option(k, v)
        if lens > 0.0:
            r.set_lens(lens, 4.0)
        if "tiles" in kw:
            F, _, st = r.render_tiles_host(kw["tiles"], **{k: v for k, v in kw.items() if k != "tiles"})
        else:
            F, st = r.render_host(**kw)
        r.close()
        np.save(os.path.join(out_dir, key + ".npy"), F)
        stats[key] = {k: int(st[k]) for k in STAT_KEYS + ("engine",)}
    # one context: a camera, another camera (a new upload), the first again, then a lens and the pinhole again
    sys.stderr.write("\nCASE reuse\n"); sys.stderr.flush()
    a, b = cbox((64, 64), "path_mis"), cbox((64, 64), "path_mis")
    b.camera.to_world = scenes.lookat((0.6, 1.3, 3.9), (0, 0.8, 0), (0, 1, 0))
    r = Renderer(0).upload(a, builder=2)
    r.set_option("engine", "wavefront")
    for name, sc in (("reuse-a", None), ("reuse-a-again", None), ("reuse-b", b), ("reuse-a-back", a)):
        if sc is not None:
            r.upload(sc, builder=2)
            r.set_option("engine", "wavefront")
        np.save(os.path.join(out_dir, name + ".npy"), r.render_host()[0])
    r.set_lens(0.05, 4.0)
    np.save(os.path.join(out_dir, "reuse-a-lens.npy"), r.render_host()[0])
    r.set_lens(0.0, 1.0)
    np.save(os.path.join(out_dir, "reuse-a-pinhole.npy"), r.render_host()[0])
    r.close()
    for name, sc in (("fresh-a", a), ("fresh-b", b)):
        r = Renderer(0).upload(sc, builder=2)
        r.set_option("engine", "wavefront")
        np.save(os.path.join(out_dir, name + ".npy"), r.render_host()[0])
        r.close()
    with open(os.path.join(out_dir, "stats.json"), "w") as f:
        json.dump(stats, f)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_first_lists import render_cases
render_cases(sys.argv[2])
"""

_LISTS = re.compile(r"\[wavefront first pass\] lists: K (\d+), (\d+) list tiles, (\d+) overflow tiles, build ([0-9.]+) ms \((built in this call|kept)\)")


def first_pass_lines(stderr):
    """case -> [("lists", K, list tiles, overflow tiles, built) | ("walk",)] in the order the render calls made them"""
    out, key = {}, None
    for line in stderr.splitlines():
        if line.startswith("CASE "):
            key = line[5:].strip()
            out[key] = []
        m = _LISTS.search(line)
        if m and key:
            out[key].append(("lists", int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(5) == "built in this call"))
        elif "[wavefront first pass] walk" in line and key:
            out[key].append(("walk",))
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """variant -> (directory of frames, stats, first-pass lines per case); the five children run side by side"""
    for k in ("NORI_HIP_WF_FIRST", "NORI_HIP_WF_FIRST_K", "NORI_HIP_WF_FIRST_REBUILD"):
        assert os.environ.get(k) is None, "the children set the switches"
    procs = {}
    for name, env in VARIANTS.items():
        d = tmp_path_factory.mktemp("first_" + name)
        log = open(d / "stderr.txt", "w")      # (files, not pipes: a child never waits for this process to read)
        procs[name] = (d, log, subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, str(d)], env=dict(os.environ, NORI_HIP_CENSUS="1", **env),
                                                stdout=subprocess.DEVNULL, stderr=log))
    out = {}
    for name, (d, log, p) in procs.items():
        rc = p.wait(timeout=600)
        log.close()
        se = open(d / "stderr.txt").read()
        assert rc == 0, (name, se[-4000:])
        out[name] = (d, json.load(open(d / "stats.json")), first_pass_lines(se))
    return out


@pytest.mark.parametrize("variant", ["lists", "k0", "k1", "auto"])
@pytest.mark.parametrize("key", KEYS)
def test_same_bits_as_the_old_first_pass(runs, key, variant):
    d0, s0, l0 = runs["old"]
    d1, s1, l1 = runs[variant]
    assert s0[key]["engine"] == s1[key]["engine"] == 1, (key, s0[key], s1[key])
    for k in STAT_KEYS:
        assert s0[key][k] == s1[key][k], (key, variant, k, s0[key][k], s1[key][k])
    assert s1[key]["n_camera_samples"] > 0 and s1[key]["n_closest_rays"] >= s1[key]["n_camera_samples"]
    A, B = np.load(d0 / (key + ".npy")), np.load(d1 / (key + ".npy"))
    assert A.dtype == B.dtype == np.float32 and A.shape == B.shape and (B[..., 3] > 0).any(), key
    diff = A.view(np.uint32) != B.view(np.uint32)
    assert not diff.any(), f"{key} / {variant}: {int(diff.sum())} of {A.size} floats differ, max {np.abs(A - B).max():.3e}, first at {tuple(np.argwhere(diff)[0])}"
    # which first pass ran
    assert l0[key] and all(x == ("walk",) for x in l0[key]), (key, l0[key])
    assert l1[key], (key, variant)
    if EXPECTED[key] == "walk":
        assert all(x == ("walk",) for x in l1[key]), (key, variant, l1[key])
        return
    n_tiles = TILES[key]
    if variant == "auto":      # the lists (at most one tile in sixteen on overflow) or the old kernel, by the frame
        for x in l1[key]:
            # (the line names the whole frame's tiles; a share of them -- tile_mod -- is judged by its own tiles)
            share = any("tile_mod" in c[3] for c in _CASES if c[0] == key)
            assert x == ("walk",) or (x[0] == "lists" and x[1] == DEFAULT_K and x[2] + x[3] == n_tiles and (share or 16 * x[3] <= n_tiles)), (key, x)
        if key.startswith("bunny"):
            assert all(x == ("walk",) for x in l1[key]), (key, l1[key])      # the mesh fills the view
        if key in AUTO_MUST_LIST:
            assert all(x[0] == "lists" and x[2] > 0 for x in l1[key]), (key, l1[key])      # the list path ran, with > 0 list tiles
        if key == "cbox-256x256-path_mis":
            assert l1[key][0][3] > 0, (key, l1[key])      # ... beside overflow tiles
        return
    for x in l1[key]:
        assert x[0] == "lists" and x[2] + x[3] == n_tiles, (key, variant, x)
        if variant == "lists":
            assert x[1] == DEFAULT_K, (key, x)                               # the product's K
            assert x[2] > 0 or key.startswith("bunny"), (key, x)     # some tiles are on lists (the bunny fills every tile of a small frame)
        elif variant == "k0":
            assert x[1] == 0 and x[2] == 0, (key, x)                 # every tile overflows
        else:
            assert x[1] == 1, (key, x)
    if variant == "lists" and key.startswith("dense"):
        assert l1[key][0][3] > 0, (key, l1[key])                      # the tessellated spheres overflow


@pytest.mark.parametrize("variant", ["old", "lists", "k0", "k1"])
def test_lists_follow_the_camera(runs, variant):
    """One context, uploads with another camera and back, a lens and the pinhole again: every frame equals that of a fresh context,
    and the lists are built when (and only when) what they were built for has changed."""
    d, _, lines = runs[variant]
    f = {n: np.load(d / (n + ".npy")) for n in ("reuse-a", "reuse-a-again", "reuse-b", "reuse-a-back", "reuse-a-lens", "reuse-a-pinhole", "fresh-a", "fresh-b")}
    same = lambda x, y: x.shape == y.shape and not (x.view(np.uint32) != y.view(np.uint32)).any()
    assert same(f["reuse-a"], f["fresh-a"]) and same(f["reuse-a-again"], f["fresh-a"]) and same(f["reuse-a-back"], f["fresh-a"]) and same(f["reuse-a-pinhole"], f["fresh-a"])
    assert same(f["reuse-b"], f["fresh-b"]) and not same(f["fresh-a"], f["fresh-b"]) and not same(f["reuse-a-lens"], f["fresh-a"])
    got = lines["reuse"]
    assert len(got) == 8
    if variant == "old":
        assert all(x == ("walk",) for x in got)
    else:
        # a, a again (kept), b (built), a back (built), lens (walk), pinhole (built: set_lens drops the lists), fresh a, fresh b
        assert [x[0] for x in got] == ["lists", "lists", "lists", "lists", "walk", "lists", "lists", "lists"]
        assert [x[4] for x in got if x[0] == "lists"] == [True, False, True, True, True, True, True]
