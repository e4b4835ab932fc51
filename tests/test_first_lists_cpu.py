"""The per-tile candidate lists of the first pass (nori_amd/csrc/device/first_lists.h) on the CPU, through the shared culling step:
tests/first_lists/harness.cpp is built here with g++ into a library of its own and called through ctypes.

For every tile that has a list and every ray of a deterministic set -- the extreme jitters (0 and the largest float below 1 on both
axes) of the tile's four corner pixels, and seeded samples of every pixel drawn as first_vertex draws them -- the triangle the walk
of rt_trace.h finds must be in the tile's list, and the list must return the walk's (t, u, v, triangle) bit for bit; every 64th ray
(every ray of the tiny scenes) is also held to the linear scan over all pair records.  The margin is the one derived in first_lists.h
(margin_scale 1); the exactly representable axis-aligned case also runs at margin 0."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nori_amd import _capi as capi
from nori_amd import workloads
from tests import scenes
from tests.first_list_cases import case, filler, only_clipped, tiny_scene, tri_mesh      # noqa: F401 (the helpers keep their names here)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "first_lists", "harness.cpp")
PREP = os.path.join(ROOT, "nori_amd", "csrc", "device", "scene_prep.cpp")
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-comment", "-Wno-unused-function",
            "-Wno-misleading-indentation", "-Wno-class-memaccess"]
OVERFLOW = 0xFFFFFFFF
HEADER = open(os.path.join(ROOT, "nori_amd", "csrc", "device", "first_lists.h")).read()
MAX_K = int(re.search(r"kFirstListMaxK = (\d+)u", HEADER).group(1))
DEFAULT_K = int(re.search(r"kFirstListDefaultK = (\d+)u", HEADER).group(1))      # K of the product
P = C.c_void_p


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("first_lists") / "libfirst_lists.so")
    p = subprocess.run(["g++"] + CXXFLAGS + ["-o", out, SRC, PREP], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    lib = C.CDLL(out)
    lib.fl_create.argtypes = [C.POINTER(capi.SceneDesc), C.c_int, C.POINTER(P)]
    lib.fl_destroy.argtypes = [P]
    lib.fl_destroy.restype = None
    lib.fl_info.argtypes = [P, P]
    lib.fl_info.restype = None
    lib.fl_margin.argtypes = [P, C.c_int, C.c_int, P]
    lib.fl_lists.argtypes = [P, C.c_uint32, C.c_double, P, P]
    lib.fl_lists.restype = C.c_uint32
    lib.fl_tiles_on_big_meshes.argtypes = [P, C.c_uint32, P]
    lib.fl_tiles_on_big_meshes.restype = None
    lib.fl_check.argtypes = [P, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32, P]
    return lib


class Harness:
    def __init__(self, lib, scene, builder=0):
        self.lib, self.scene = lib, scene
        desc, keep = scene.c_desc()
        self.h = P()
        assert lib.fl_create(C.byref(desc), builder, C.byref(self.h)) == 0
        del keep
        cam = scene.camera
        self.n_tiles = ((cam.width + 15) // 16) * ((cam.height + 15) // 16)

    def close(self):
        if self.h:
            self.lib.fl_destroy(self.h)
            self.h = None

    def info(self):
        a = np.zeros(4, np.int64)
        self.lib.fl_info(self.h, a.ctypes.data)
        return dict(n_nodes=int(a[0]), n_pairs=int(a[1]), root=int(a[2]), max_depth=int(a[3]))

    def margin(self, x0=0, y0=0):
        m = np.zeros(3)
        ok = self.lib.fl_margin(self.h, x0, y0, m.ctypes.data)
        return ok, dict(theta=m[0], eps_z=m[1], pad_abs=m[2])

    def lists(self, K, margin_scale=1.0):
        count = np.zeros(self.n_tiles, np.uint32)
        pairs = np.zeros(self.n_tiles * max(K, 1), np.uint32)
        assert self.lib.fl_lists(self.h, K, margin_scale, count.ctypes.data, pairs.ctypes.data) == self.n_tiles
        return count, pairs.reshape(self.n_tiles, max(K, 1))

    def tiles_on_big_meshes(self, min_tris):
        out = np.zeros(self.n_tiles, np.uint8)
        self.lib.fl_tiles_on_big_meshes(self.h, min_tris, out.ctypes.data)
        return out.astype(bool)

    def check(self, K, margin_scale=1.0, per_pixel=2, scan_every=64):
        out = np.zeros(8, np.uint64)
        assert self.lib.fl_check(self.h, K, margin_scale, per_pixel, scan_every, out.ctypes.data) == 0
        keys = ("rays", "hits", "scanned", "not_in_list", "list_differs", "scan_differs", "list_tiles", "overflow_tiles")
        return {k: int(v) for k, v in zip(keys, out)}


def assert_superset(r, what=""):
    assert r["not_in_list"] == 0 and r["list_differs"] == 0 and r["scan_differs"] == 0, (what, r)
    assert r["rays"] == 0 if r["list_tiles"] == 0 else (r["rays"] > 0 and r["scanned"] > 0), (what, r)      # (a small K may leave no tile a list)


# ------------------------------------------------------------------------------------------------ the headline scene, full size
@pytest.fixture(scope="module")
def cbox_1024(lib):
    h = Harness(lib, workloads.load("pa4-cbox-path_mis", 1024, 1024, 1).scene, builder=1)      # the tree a context builds by default
    yield h
    h.close()


def test_cornell_box_1024_lists_hold_every_hit(cbox_1024):
    """1024 x 1024, two seeded samples per pixel and the corner extremes of every tile, at the product's K.  No tile is left out
    on account of overflow but those the histogram of DESIGN.md section 7 names: tiles on the two tessellated spheres that see more
    pair records than the product's K."""
    r = cbox_1024.check(DEFAULT_K, per_pixel=2, scan_every=64)
    assert_superset(r, "pa4 Cornell box 1024^2")
    assert r["list_tiles"] + r["overflow_tiles"] == 4096
    assert r["rays"] == r["list_tiles"] * (16 + 2 * 256)
    count, _ = cbox_1024.lists(MAX_K)
    # the histogram: tiles off the spheres see at most 2 pairs (3 at a few silhouettes), tiles outside the box none
    assert (count == 0).sum() > 1000 and (count <= 2).sum() > 3500
    # the histogram of DESIGN.md section 7, cumulative: tiles with more than K pairs
    assert r["overflow_tiles"] == {8: 463, 16: 288, 32: 85, 64: 24}[DEFAULT_K]
    # ... and every one of them lies on a tessellated sphere: the centre ray of one of its pixels, or of a neighbouring tile's (a
    # silhouette), hits a mesh of a thousand triangles or more; the walls, the light and the space outside the box never overflow
    over = (cbox_1024.lists(DEFAULT_K)[0] == OVERFLOW).reshape(64, 64)
    on = cbox_1024.tiles_on_big_meshes(1000).reshape(64, 64)
    near = np.zeros_like(on)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near[max(0, dy):64 + min(0, dy), max(0, dx):64 + min(0, dx)] |= on[max(0, -dy):64 + min(0, -dy), max(0, -dx):64 + min(0, -dx)]
    assert over.sum() == r["overflow_tiles"] and not (over & ~near).any() and 300 < on.sum() < 700
    ok, m = cbox_1024.margin(512, 512)
    assert ok == 3 and 0.0 < m["theta"] < 1e-4 and 0.0 < m["pad_abs"] < 1e-4      # against a tile 8e-3 rad wide


def test_cornell_box_1024_every_k(cbox_1024):
    """K = 0: every tile overflows; K = 1 and the largest K: supersets all the same (fewer rays per pixel)."""
    count, _ = cbox_1024.lists(0)
    assert (count == OVERFLOW).all()
    for K in (1, MAX_K):
        r = cbox_1024.check(K, per_pixel=1, scan_every=256)
        assert_superset(r, f"K = {K}")


# ------------------------------------------------------------------------------------------------ a dense mesh, an odd frame
@pytest.mark.parametrize("builder", [0, 1])
def test_dense_mesh_odd_frame(lib, builder):
    """the bunny (a dense mesh filling the view) at 200 x 136: width and height are no multiples of 16, edge tiles hang over the image"""
    h = Harness(lib, workloads.load("c1-bunny-normals", 200, 136, 1).scene, builder=builder)
    try:
        r = h.check(MAX_K, per_pixel=2, scan_every=16)
        assert_superset(r, "bunny 200 x 136")
        assert r["list_tiles"] > 0 and r["hits"] > 0
        r = h.check(DEFAULT_K, per_pixel=1, scan_every=64)
        assert_superset(r, "bunny 200 x 136, K of the product")
    finally:
        h.close()


@pytest.mark.parametrize("size", [(40, 24), (64, 64), (100, 60)])
def test_cornell_box_small_frames(lib, size):
    sc = scenes.cornell_box(size[0], size[1], 4, "path_mis")
    for builder in (0, 1):
        h = Harness(lib, sc, builder=builder)
        try:
            for K in (1, DEFAULT_K, MAX_K):
                assert_superset(h.check(K, per_pixel=4, scan_every=1), f"{size} builder {builder} K {K}")
        finally:
            h.close()


# ------------------------------------------------------------------------------------------------ adversarial cases, tiny frames
# (the scenes live in tests/first_list_cases.py, which the GPU tests share)
def check_tiny(lib, sc, what, builders=(0, 1), expect_hits=True):
    for builder in builders:
        h = Harness(lib, sc, builder=builder)
        try:
            for K in (2, MAX_K):
                r = h.check(K, per_pixel=8, scan_every=1)
                assert_superset(r, f"{what} builder {builder} K {K}")
                if expect_hits and K == MAX_K:
                    assert r["hits"] > 0 and r["list_tiles"] > 0, (what, r)
        finally:
            h.close()


def test_edge_in_a_frustum_side_plane(lib):
    """a triangle edge on the plane x = 0, which for this camera (on the z axis, 32 pixels wide) is the side plane between the two
    tile columns -- and one on y = 0, between the rows"""
    check_tiny(lib, case("edge-in-a-side-plane"), "edge in a side plane")


def test_triangle_spanning_the_camera_plane(lib):
    check_tiny(lib, case("through-the-camera-plane"), "triangle through the camera plane")


def test_camera_inside_a_box(lib):
    """the camera inside the scene's box and inside leaf boxes: a shell of triangles around it"""
    check_tiny(lib, case("camera-inside-boxes"), "camera inside boxes")


def test_flat_boxes(lib):
    """axis-aligned triangles: zero-thickness boxes in x, y and z"""
    check_tiny(lib, case("flat-boxes"), "flat boxes")      # (the filler gives the tree inner nodes: a root that is a leaf gets no lists)


def test_near_and_far_clip(lib):
    """one triangle in front of the near clip, one beyond the far clip, one between: only the last is ever hit, and the lists agree"""
    check_tiny(lib, case("near-and-far-clip"), "near / far clip")
    h = Harness(lib, only_clipped())
    try:
        r = h.check(MAX_K, per_pixel=8, scan_every=1)
        assert_superset(r)
        assert r["hits"] == 0      # both are clipped for every ray
    finally:
        h.close()


def test_spatial_split_duplicates(lib):
    """long thin diagonal triangles among small ones: the device builders split them, so leaves hold duplicated references (more
    pair slots than triangles); duplicates give identical candidates"""
    sc = case("split-duplicates")
    h = Harness(lib, sc, builder=1)
    try:
        n_tris = sum(m.indices.shape[0] for m in sc.meshes)
        assert 2 * h.info()["n_pairs"] > n_tris + 1      # more slots than triangles: references were duplicated (or padded)
    finally:
        h.close()
    check_tiny(lib, sc, "split duplicates", builders=(1,))


def test_axis_aligned_case_at_margin_zero(lib):
    """The exactly representable case: camera at (0, 0, 4) looking down -z with fov 90 (the tile borders of a 32 x 32 frame are the
    planes x = 0 and y = 0, slopes 0 and +-1), triangles with small-integer coordinates.  With margin 0 the lists must still hold
    every hit: the margin is not what makes the signs right."""
    sc = case("axis-aligned")
    for builder in (0, 1):
        h = Harness(lib, sc, builder=builder)
        try:
            for scale in (0.0, 1.0):
                r = h.check(MAX_K, margin_scale=scale, per_pixel=16, scan_every=1)
                assert_superset(r, f"axis-aligned, margin x {scale}")
                assert r["hits"] == r["rays"]      # the back wall fills the view
            c0, _ = h.lists(MAX_K, 0.0)
            c1, _ = h.lists(MAX_K, 1.0)
            assert (c0 <= c1).all() and (c1 != OVERFLOW).all()      # margin 0 culls no less
        finally:
            h.close()
