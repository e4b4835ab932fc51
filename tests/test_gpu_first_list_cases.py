"""The per-tile candidate lists of the first pass on the GPU, over the cases of tests/first_list_cases.py (adversarial scenes, cameras
that are no rigid lookat, scaled scenes, odd and one-tile frames, slivers, coplanar duplicates):

(a) the lists wf_first_build writes, read back (Renderer.first_lists -> nori_hip_debug_first_lists), equal the lists the CPU harness
    computes from the same header on the same tree (the host's SAH builder: the same scene_prep.cpp on both sides), entry for entry.
    Both sides are binary64 with -ffp-contract=off, correctly rounded / and sqrt and the same walk order: there is no tolerance.
(b) for the trees of every builder, no camera ray of a tile with a list hits a triangle that is not among the tile's listed pair
    records -- seeded jitters of every pixel and the extreme jitters of every tile's corner pixels, traced by nori_hip_intersect.
(c) whole frames through wf_first_extend, in child processes (the switches are read once per process): the old first pass, the lists
    at the product's K and at K = 64.  The bordered RGBW frame and the ray counts must be the old first pass's bit for bit, and the
    census line must name the first pass the case expects.  Further, on the base scene at 100 x 60: passes that start at unaligned
    sample indices (pools of 1000 and 777 paths, batches of 1000 samples), the last sample indices below 2^32, renders by tile list,
    and a second upload with moved vertices under the same camera and triangle count (stale lists)."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi as capi
from nori_amd.scene import Integrator
from tests import first_list_cases as flc
from tests.test_first_lists_cpu import DEFAULT_K, MAX_K, OVERFLOW, Harness, lib      # noqa: F401 (lib: the fixture that builds the harness)
from tests.test_gpu_first_lists import STAT_KEYS, first_pass_lines
from tests.tree_audit import decode_pairs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPP = 4
VARIANTS = {"old": {"NORI_HIP_WF_FIRST": "0"}, "lists": {"NORI_HIP_WF_FIRST": "2"}, "k64": {"NORI_HIP_WF_FIRST": "2", "NORI_HIP_WF_FIRST_K": "64"}}
VARIANT_K = {"lists": DEFAULT_K, "k64": 64}
assert MAX_K == 64


def tri_offsets(sc):
    return np.concatenate([[0], np.cumsum([m.indices.shape[0] for m in sc.meshes])]).astype(np.int64)


@pytest.fixture(scope="module")
def renderer():
    from nori_amd.render import Renderer
    r = Renderer(0)
    yield r
    r.close()


# ------------------------------------------------------------------------------------------------ (a) the device's lists are the header's
@pytest.mark.parametrize("key", flc.KEYS)
def test_device_lists_equal_the_harness_lists(renderer, lib, key):
    sc = flc.case(key)
    r = renderer.upload(sc, builder=0)
    h = Harness(lib, sc, builder=0)
    try:
        tree, info = r.tree(), h.info()
        assert (tree["n_nodes"], tree["n_pairs"], tree["root"], tree["wide"]) == (info["n_nodes"], info["n_pairs"], info["root"], 0)
        for K in (2, DEFAULT_K, 64):
            got_c, got_p = r.first_lists(K)
            want_c, want_p = h.lists(K)
            assert got_c.shape == want_c.shape == (flc.n_tiles(key),) and got_p.shape == want_p.shape
            assert (got_c == want_c).all(), (key, K, got_c.tolist(), want_c.tolist())
            for t in np.flatnonzero(got_c != OVERFLOW):
                n = int(got_c[t])
                assert n <= K and (got_p[t, :n] == want_p[t, :n]).all(), (key, K, int(t), got_p[t, :n].tolist(), want_p[t, :n].tolist())
                assert (got_p[t, :n] < tree["n_pairs"]).all()
            lists = int((got_c != OVERFLOW).sum())
            print(f"READBACK builder 0 {key}: K {K}: {lists} list tiles, {len(got_c) - lists} overflow tiles")
            if K == 64:
                if flc.EXPECT[key] == "lists":
                    assert lists > 0, (key, got_c)
                else:
                    assert lists == 0, (key, got_c)
    finally:
        h.close()


def test_read_back_refuses_what_it_states(renderer):
    """K > 64 and a context without a tree are invalid arguments with a message; K = 0 and a lens give overflow everywhere; the call
    leaves the lists a render keeps alone (the render after it still finds them: "kept" is checked in the children)."""
    from nori_amd.render import Renderer
    sc = flc.case("base")
    r = renderer.upload(sc, builder=0)
    with pytest.raises(capi.NoriError, match="INVALID_ARGUMENT.*debug_first_lists"):
        r.first_lists(65)
    c, p = r.first_lists(0)
    assert (c == OVERFLOW).all() and p.shape == (flc.n_tiles("base"), 1) and not p.any()
    a = r.first_lists(DEFAULT_K)
    r.set_lens(0.05, 4.0)
    assert (r.first_lists(DEFAULT_K)[0] == OVERFLOW).all()
    r.set_lens(0.0, 1.0)
    b = r.first_lists(DEFAULT_K)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[0] != OVERFLOW).any()
    fresh = Renderer(0)
    try:
        fresh.upload(sc, build=False)
        with pytest.raises(capi.NoriError, match="INVALID_ARGUMENT.*debug_first_lists"):
            fresh.first_lists(DEFAULT_K)
        fresh.build_accel(0)
        assert (fresh.first_lists(DEFAULT_K)[0] == a[0]).all()      # the context stays usable
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ (b) superset by rays
def tile_samples(cam, seed):
    """(ps [n, 2] float32, tile [n]): per pixel four seeded jitters, per tile the jitters 0 and nextafter(1, 0) on both axes of its four
    corner pixels.  ps = (float) px + j in binary32, which may round up to px + 1: the tile is that of the integer pixel."""
    W, H = cam.width, cam.height
    tx = (W + 15) // 16
    py, px = (a.reshape(-1) for a in np.mgrid[0:H, 0:W])
    rng = np.random.default_rng(seed)
    pix = [np.stack([np.repeat(px, 4), np.repeat(py, 4)], 1)]
    jit = [rng.random((pix[0].shape[0], 2), dtype=np.float32)]
    below_one = np.nextafter(np.float32(1), np.float32(0))
    for y0 in range(0, H, 16):
        for x0 in range(0, W, 16):
            for cx in (x0, min(x0 + 16, W) - 1):
                for cy in (y0, min(y0 + 16, H) - 1):
                    for jx in (np.float32(0), below_one):
                        for jy in (np.float32(0), below_one):
                            pix.append(np.array([[cx, cy]])); jit.append(np.array([[jx, jy]], np.float32))
    pix, jit = np.concatenate(pix), np.concatenate(jit).astype(np.float32)
    assert (jit >= 0).all() and (jit < 1).all()
    ps = pix.astype(np.float32) + jit      # binary32, as first_vertex adds them
    return ps, (pix[:, 1] // 16) * tx + pix[:, 0] // 16


@pytest.mark.parametrize("builder", [0, 1, 3, 2])
@pytest.mark.parametrize("key", flc.KEYS)
def test_no_ray_hits_outside_its_tiles_list(renderer, key, builder):
    sc, expect = flc.case(key), flc.EXPECT[key]
    r = renderer.upload(sc, builder=builder)
    tree = r.tree()
    assert tree["wide"] == 0
    gid = decode_pairs(tree["pairs"])[3].astype(np.int64).reshape(-1, 2)      # [pair record, slot]
    ps, tile = tile_samples(sc.camera, 7)
    its = r.intersect(r.sample_rays(ps))
    hit = its["mesh"] != capi.NO_HIT
    hit_gid = np.where(hit, tri_offsets(sc)[np.where(hit, its["mesh"], 0).astype(np.int64)] + its["tri"], -1)
    n_tiles = flc.n_tiles(key)
    for K in (64, DEFAULT_K):
        count, pairs = r.first_lists(K)
        judged = 0
        for t in np.flatnonzero(count != OVERFLOW):
            listed = gid[pairs[t, :int(count[t])].astype(np.int64)].reshape(-1)
            g = hit_gid[(tile == t) & hit]
            judged += len(g)
            missing = g[~np.isin(g, listed)]
            assert len(missing) == 0, (key, builder, K, int(t), np.unique(missing).tolist(), ps[(tile == t) & hit][~np.isin(g, listed)][:4].tolist())
        lists = int((count != OVERFLOW).sum())
        if builder == 2:
            print(f"READBACK builder 2 {key}: K {K}: {lists} list tiles, {n_tiles - lists} overflow tiles, {judged} hits judged")
        if K == 64:
            if expect == "lists":
                assert judged > 0, (key, builder, count.tolist())
                if builder == 2:
                    assert lists >= (n_tiles + 1) // 2, (key, count.tolist())
            else:
                assert lists == 0


# ------------------------------------------------------------------------------------------------ (c) frames through the kernels
def with_integrator(sc, integrator, spp=SPP):
    return dataclasses.replace(sc, integrator=Integrator(integrator), sample_count=spp)


def big(moved=False):
    """the base scene at 100 x 60 (7 x 4 tiles, the last column 4 pixels wide, the last row 12 high), path_mis"""
    return with_integrator(flc.base_scene(size=(100, 60), meshes=flc.base_meshes(moved=moved)), "path_mis")


BIG_TILES = 28
# tile lists: every second tile counted down from the last one (a list must be strictly ascending: see test_a_descending_tile_list_is_refused),
# and the single last tile, the one that hangs over the image on both axes
EXTRA = (("pool-1000", {"wavefront_paths": 1000, "wavefront_samples": 1 << 30}, {}),
         ("pool-777", {"wavefront_paths": 777, "wavefront_samples": 1 << 30}, {}),
         ("samples-1000", {"wavefront_samples": 1000}, {}),
         ("last-sample-index", {}, {"spp_count": 4, "spp_begin": 2 ** 32 - 4}),
         ("tiles-from-the-last", {}, {"tiles": sorted(range(BIG_TILES - 1, -1, -2))}),
         ("tiles-last-alone", {}, {"tiles": [BIG_TILES - 1]}))
FRAME_KEYS = tuple(f"{key}/{integ}" for key in flc.KEYS for integ in flc.frame_integrators(key))
EXTRA_KEYS = tuple("big/" + e[0] for e in EXTRA)
STALE = ("stale/first", "stale/moved", "stale/fresh-moved")


def render_cases(out_dir):
    """every frame of this file through the wavefront engine on the tree a context builds by default: <name>.npy and stats.json in
    out_dir, a marker per frame on stderr (the census lines follow it)"""
    from nori_amd.render import Renderer
    stats = {}

    def one(name, scene, options, kw, r=None):
        sys.stderr.write(f"\nCASE {name}\n"); sys.stderr.flush()
        own = r is None
        if own:
            r = Renderer(0)
        r.upload(scene, builder=2)
        r.set_option("engine", "wavefront")
        for k, v in options.items():
            r.set_option(k, v)
        if "tiles" in kw:
            F, _, st = r.render_tiles_host(kw["tiles"], **{k: v for k, v in kw.items() if k != "tiles"})
        else:
            F, st = r.render_host(**kw)
        if own:
            r.close()
        np.save(os.path.join(out_dir, name.replace("/", "--") + ".npy"), F)
        stats[name] = {k: int(st[k]) for k in STAT_KEYS + ("engine",)}

    shared = Renderer(0)      # (every upload drops what the engine keeps per tree and camera)
    for key in flc.KEYS:
        for integ in flc.frame_integrators(key):
            one(f"{key}/{integ}", with_integrator(flc.case(key), integ), {}, {}, shared)
    shared.close()
    for name, options, kw in EXTRA:
        one("big/" + name, big(), options, kw)
    # the API's statement on tile lists, where the kernels index them
    r = Renderer(0).upload(big(), builder=2)
    r.set_option("engine", "wavefront")
    try:
        r.render_tiles_host(list(range(BIG_TILES - 1, -1, -1)))
        refused = ""
    except capi.NoriError as e:
        refused = str(e)
    stats["descending-refused"] = refused
    r.close()
    # stale lists: one context, the same camera and triangle count, moved vertices
    r = Renderer(0)
    one(STALE[0], big(), {}, {}, r)
    one(STALE[1], big(moved=True), {}, {}, r)
    r.close()
    one(STALE[2], big(moved=True), {}, {})
    with open(os.path.join(out_dir, "stats.json"), "w") as f:
        json.dump(stats, f)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_first_list_cases import render_cases
render_cases(sys.argv[2])
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """variant -> (directory of frames, stats, first-pass lines per frame); the three children run side by side"""
    for k in ("NORI_HIP_WF_FIRST", "NORI_HIP_WF_FIRST_K", "NORI_HIP_WF_FIRST_REBUILD"):
        assert os.environ.get(k) is None, "the children set the switches"
    procs = {}
    for name, env in VARIANTS.items():
        d = tmp_path_factory.mktemp("first_cases_" + name)
        log = open(d / "stderr.txt", "w")      # (files, not pipes: a child never waits for this process to read)
        procs[name] = (d, log, subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, str(d)], env=dict(os.environ, NORI_HIP_CENSUS="1", **env),
                                                stdout=subprocess.DEVNULL, stderr=log))
    out, failed = {}, []
    for name, (d, log, p) in procs.items():
        rc = p.wait(timeout=300)
        log.close()
        se = open(d / "stderr.txt").read()
        if rc != 0:
            failed.append((name, rc, se[-4000:]))
            continue
        out[name] = (d, json.load(open(d / "stats.json")), first_pass_lines(se))
    assert not failed, failed
    return out


def load(d, name):
    return np.load(d / (name.replace("/", "--") + ".npy"))


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and not (a.view(np.uint32) != b.view(np.uint32)).any()


@pytest.mark.parametrize("variant", ["lists", "k64"])
@pytest.mark.parametrize("name", FRAME_KEYS + EXTRA_KEYS + STALE)
def test_frames_have_the_bits_of_the_old_first_pass(runs, name, variant):
    d0, s0, l0 = runs["old"]
    d1, s1, l1 = runs[variant]
    assert s0[name]["engine"] == s1[name]["engine"] == 1, (name, s0[name], s1[name])
    for k in STAT_KEYS:
        assert s0[name][k] == s1[name][k], (name, variant, k, s0[name][k], s1[name][k])
    assert s1[name]["n_camera_samples"] > 0 and s1[name]["n_closest_rays"] >= s1[name]["n_camera_samples"]
    A, B = load(d0, name), load(d1, name)
    assert A.dtype == B.dtype == np.float32 and A.shape == B.shape and (B[..., 3] > 0).any(), name
    diff = A.view(np.uint32) != B.view(np.uint32)
    assert not diff.any(), f"{name} / {variant}: {int(diff.sum())} of {A.size} floats differ, max {np.abs(A - B).max():.3e}, first at {tuple(np.argwhere(diff)[0])}"
    # which first pass ran
    assert l0[name] and all(x == ("walk",) for x in l0[name]), (name, l0[name])
    assert l1[name], (name, variant)
    key = name.split("/")[0]
    expect = flc.EXPECT[key] if key in flc.EXPECT else "lists"
    n_tiles = flc.n_tiles(key) if key in flc.EXPECT else BIG_TILES
    for x in l1[name]:
        if expect == "walk":
            assert x == ("walk",), (name, variant, x)
            continue
        assert x[0] == "lists" and x[1] == VARIANT_K[variant] and x[2] + x[3] == n_tiles, (name, variant, x)
        if expect == "all-overflow":
            assert x[2] == 0, (name, variant, x)
        elif variant == "k64" or key not in flc.OLD_KEYS:
            # ("lists" is stated at K = 64; every case but those the CPU file has had keeps list tiles at the product's K as well)
            assert x[2] > 0, (name, variant, x)


def test_frames_see_what_they_should(runs):
    """the frames are not empty shells: the normals frames of the base scene differ between cameras, and the two tie scenes -- the
    same triangles in opposite mesh orders -- differ in radiance"""
    d, _, _ = runs["k64"]
    assert not same_bits(load(d, "base/normals"), load(d, "rolled-37/normals")) and not same_bits(load(d, "base/normals"), load(d, "mirrored/normals"))
    a, b = load(d, "ties/path_mats"), load(d, "ties-reversed/path_mats")
    assert a[..., :3].max() > 0 and b[..., :3].max() > 0 and not same_bits(a, b)
    assert (a[..., 3] == b[..., 3]).all()      # the same samples landed


@pytest.mark.parametrize("variant", ["old", "lists", "k64"])
def test_a_descending_tile_list_is_refused(runs, variant):
    """nori_hip_render_tiles states that a list is strictly ascending and refuses any other before a kernel sees it: a descending
    list cannot reach round_tile.  (The lists rendered above are ascending ones that skip tiles, counted down from the last.)"""
    assert "INVALID_ARGUMENT" in runs[variant][1]["descending-refused"] and "strictly ascending" in runs[variant][1]["descending-refused"]


@pytest.mark.parametrize("variant", ["old", "lists", "k64"])
def test_lists_do_not_outlive_the_geometry(runs, variant):
    """One context: the base scene, then the same scene with every filler vertex moved under the same camera and triangle count.  The
    second frame is the frame of a fresh context and not the first one's, and the lists are built in both calls."""
    d, _, lines = runs[variant]
    first, moved, fresh = (load(d, n) for n in STALE)
    assert same_bits(moved, fresh) and not same_bits(moved, first)
    got = [x for n in STALE for x in lines[n]]
    assert len(got) == 3
    if variant == "old":
        assert all(x == ("walk",) for x in got)
    else:
        assert all(x[0] == "lists" and x[2] > 0 and x[4] for x in got), got      # x[4]: "built in this call"
