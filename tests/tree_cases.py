"""Scenes for the audit of built trees (tests/tree_audit.py): geometry where builders go wrong, at the smallest sizes that still can.  No GPU.

    sc, env = case(name)          the scene and the builder knobs (environment variables) it is built under
    GROUPS                        the names, grouped so that one test of a group stays within a few seconds

soup-N          N triangles, N around the wave / block sizes of the one-thread-per-element kernels and around PLOC's search radius
coincident-N    N triangles of different size and orientation whose boxes share one centre: equal Morton codes, sorted position is the tie-break
flat            every vertex in the plane z = 0: one scene extent is 0, so its reciprocal is 0
line            every vertex on the x axis: two extents are 0, every triangle is collinear (the tree is the unbounded subtree alone)
far-1e4, -1e6   a unit-size soup translated far from the origin: the Morton codes use a few cells, the pad still follows a diagonal of ~1
giant-dust      three triangles that span the scene over 5000 of 1 / 100 its size; giant-dust-cut: the same with every triangle cut as often as
                the cap allows (NORI_HIP_SPLIT_BUDGET=3.0 NORI_HIP_SPLIT_SCALE=0 NORI_HIP_SPLIT_INSIDE=0)
slivers         slivers and numerically collinear triangles mixed into a soup: the unbounded subtree under the root
dups-N          the same triangle N times; 9 is more than a leaf holds
planes, mixed, table    the three scenes of test_tree_invariants_of_the_device_builders_trees
soup-200000     the largest
"""
from __future__ import annotations

import contextlib
import functools
import os

import numpy as np

from nori_amd.scene import Mesh, Scene
from tests import extend_cases, scenes
from tests.tree_audit import scene_meshes

SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)
CUT_ALL = {"NORI_HIP_SPLIT_BUDGET": "3.0", "NORI_HIP_SPLIT_SCALE": "0", "NORI_HIP_SPLIT_INSIDE": "0"}
KNOBS = ("NORI_HIP_SPLIT_BUDGET", "NORI_HIP_SPLIT_SCALE", "NORI_HIP_SPLIT_INSIDE", "NORI_HIP_ACCEL_LAYOUT", "NORI_EMU_BUILDER", "NORI_HIP_TREELET_SERIAL",
         "NORI_HIP_TREELET_SWEEPS")

GROUPS = {
    "tiny": tuple(f"soup-{n}" for n in SIZES if n <= 257) + ("dups-1", "dups-2", "dups-9", "coincident-2", "coincident-65", "line"),
    "small": ("soup-1023", "soup-1025", "soup-4097", "coincident-1000", "flat", "far-1e4", "far-1e6", "slivers"),
    "cut": ("giant-dust", "giant-dust-cut", "planes", "mixed"),
    "table": ("table",),
    "large": ("soup-200000",),
}
# the scenes on which the device's tree is compared with the harness's, record by record (tests/test_gpu_tree.py)
SAME_AS_HARNESS = ("planes", "mixed", "table", "giant-dust", "giant-dust-cut", "coincident-1000", "soup-4097")


def _scene(meshes):
    sc = scenes.soup_scene(1)
    sc.meshes = meshes
    return sc


def _tri_mesh(tris, name="m"):
    v = np.ascontiguousarray(tris, np.float32).reshape(-1, 3)
    return Mesh(v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3), name=name)


def _coincident(n, seed=7):
    rng = np.random.default_rng([seed, n])
    t = rng.normal(size=(n, 3, 3)) * rng.uniform(0.01, 1.0, (n, 1, 1))
    t -= 0.5 * (t.min(axis=1, keepdims=True) + t.max(axis=1, keepdims=True))      # the box's centre to the origin
    return _scene([_tri_mesh(t + np.array([0.25, -0.5, 0.125]))])


def _giant_dust(seed=9):
    v, f = scenes.triangle_soup(5000, seed, extent=1.0, size=0.01)
    giants = np.float32([[[-1, -1, -1], [1, 1, -0.9], [-1, 1, 1]], [[1, -1, 1], [-1, -0.9, -1], [1, 1, 0.2]], [[-1, -0.2, 1], [1, 0.3, 1], [0, 0.1, -1]]])
    return _scene([Mesh(v, f, name="dust"), _tri_mesh(giants, "giants")])


def _slivers(seed=13):
    rng = np.random.default_rng(seed)
    v, f = scenes.triangle_soup(600, seed)
    a = rng.uniform(-1, 1, (60, 3)); d = rng.normal(size=(60, 3)) * 0.4
    off = rng.normal(size=(60, 3)) * 0.4 * np.repeat([3e-3, 3e-4, 2e-5], 20)[:, None]      # sin ~ 3e-3 (wider pad), 3e-4 (much wider), 2e-5 (collinear)
    sl = np.stack([a, a + d, a + 0.5 * d + off], 1)
    col = np.float32([[[0, 0, 0], [1, 1, 1], [2, 2, 2.0000002]], [[-1, 0.5, 0.25], [-0.5, 0.5, 0.25], [0.75, 0.5, 0.25]], [[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.4, 0.1, 0.0]]])
    return _scene([Mesh(v, f, name="soup"), _tri_mesh(sl, "slivers"), _tri_mesh(col, "collinear")])


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, knobs) of a named case; made once per process"""
    kind, _, arg = name.partition("-")
    env = {}
    if kind == "soup":
        n = int(arg)
        v, f = scenes.triangle_soup(n, 100 + n % 97, size=0.25 if n < 1000 else (0.05 if n < 100000 else 0.01))
        sc = _scene([Mesh(v, f, name="soup")])
    elif kind == "coincident":
        sc = _coincident(int(arg))
    elif kind == "flat":
        v, f = scenes.triangle_soup(700, 31)
        v[:, 2] = 0.0
        sc = _scene([Mesh(v, f, name="flat")])
    elif kind == "line":
        rng = np.random.default_rng(32)
        t = np.zeros((257, 3, 3), np.float32)
        t[:, :, 0] = (rng.uniform(-1, 1, (257, 1)) + rng.uniform(-0.05, 0.05, (257, 3))).astype(np.float32)
        sc = _scene([_tri_mesh(t)])
    elif kind == "far":
        v, f = scenes.triangle_soup(1000, 33, size=0.1)
        sc = _scene([Mesh((v.astype(np.float64) + np.array([1.0, -1.0, 0.5]) * float(arg)).astype(np.float32), f, name="far")])
    elif kind == "giant":
        sc = _giant_dust()
        env = dict(CUT_ALL) if arg == "dust-cut" else {}
    elif kind == "slivers":
        sc = _slivers()
    elif kind == "dups":
        one = np.float32([[[0.1, 0.2, 0.3], [0.9, 0.1, -0.2], [0.3, 0.8, 0.4]]])
        sc = _scene([_tri_mesh(np.repeat(one, int(arg), 0))])
    elif kind == "planes":
        from tests.test_device_logic_cpu import _objects_on_planes
        sc = _objects_on_planes()
    elif kind == "mixed":
        from tests.test_device_logic_cpu import _mixed_soup
        sc = _mixed_soup(23, coincident=False)
    elif kind == "table":
        sc = Scene.load_npz(os.path.join(os.path.dirname(__file__), "golden", "pa5-table_mis.npz"))
        sc.camera.width = sc.camera.height = 16; sc.sample_count = 1
    else:
        raise ValueError(name)
    return sc, env


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(triangles [T, 3, 3] float32, mesh of each [T]) of a case"""
    sc, _ = case(name)
    return extend_cases.scene_triangles(sc), scene_meshes(sc)


@contextlib.contextmanager
def knobs(env):
    """the builder knobs of a case in the environment (both the library and the harness read them when they build), the others unset"""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def emu_tree(name, builder, layout, extra=None):
    """(tree, accel_info) of the harness's tree of a case: builder "lbvh" / "ploc" / "sah", layout "bvh2" / "bvh4q" """
    from tests.backends import Emu
    sc, env = case(name)
    with knobs(dict(env, NORI_EMU_BUILDER=builder, NORI_HIP_ACCEL_LAYOUT=layout, **(extra or {}))):
        e = Emu(sc)
    tree, info = e.tree(), e.accel_info()
    e.close()
    return tree, info
