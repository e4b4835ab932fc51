"""Scenes and cameras for the per-tile candidate lists of the first pass (nori_amd/csrc/device/first_lists.h), at the smallest sizes at
which the lists can still go wrong.  No GPU.  tests/test_first_lists_cpu.py and tests/test_first_list_cases_cpu.py run them through the
CPU harness (tests/first_lists/harness.cpp), tests/test_gpu_first_list_cases.py through the device's kernels.

    cases()          [(key, Scene, expect)], made once per process; OLD_KEYS: the adversarial scenes the CPU file has had, NEW_KEYS: the rest
    expect           "lists": some tiles have a list at K = 64; "all-overflow": the list path applies, first_camera gives ok = 0, no tile has
                     a list; "walk": wf_first_applies is false (a root that is a leaf), the engine keeps the old first pass
    frame_integrators(key)      the integrators a case's frames are rendered under

The base scene: filler(120, seed=5) -- an area emitter, so that a path_mis frame tells a filler triangle from the wall behind it and
the wall is lit -- plus a two-triangle back wall at z = -2; frame 48 x 32 (3 x 2 tiles); camera L = lookat((0.3, 0.2, 4), 0, up), fov 45.
Cameras over it (M = upper 3 x 3 of to_world, any invertible matrix: camera_sample_ray sends M normalize(d), not a unit vector):
fov 2 and 150, L Rz(37 deg), L diag(3, 3, 3), L diag(1, 2, 0.5), L with a shear m01 = 0.7, L diag(-1, 1, 1) (det < 0), a far camera at
fov 0.6, clip planes that cut through the filler; L diag(1, 1, 1e-7) has kappa >= 1e6 and must get no lists.  Then the scene at
1e-3 and 1e3 of its size, frames of 17 x 33, 100 x 60, 16 x 16 and 1 x 1 pixels, a root that is a leaf, slivers and numerically
collinear triangles (unbounded boxes, which no plane test may cull), and coplanar duplicates of distinct radiance, each a mesh of its
own, in both mesh orders: the radiance a path_mats camera ray returns names the triangle that won the tie."""
from __future__ import annotations

import functools

import numpy as np

from nori_amd.scene import Bsdf, Camera, Integrator, Mesh, RFilter, Scene
from tests import scenes

BASE_SIZE = (48, 32)
BASE_ORIGIN = (0.3, 0.2, 4.0)
MOVED_BY = (0.37, -0.21, 0.15)      # the stale-list test moves every filler vertex by this


def tri_mesh(tris, name="t", radiance=None):
    v = np.asarray(tris, dtype=np.float32).reshape(-1, 3)
    f = np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)
    return Mesh(v, f, bsdf=Bsdf("diffuse"), radiance=radiance, name=name)


def tiny_scene(meshes, origin=(0, 0, 4), target=(0, 0, 0), size=(32, 32), fov=45.0, near=1e-4, far=1e4):
    cam = Camera(size[0], size[1], fov, near_clip=near, far_clip=far, to_world=scenes.lookat(origin, target, (0, 1, 0)))
    return Scene(meshes, cam, RFilter(), Integrator("normals"), 1)


def filler(n=40, seed=3, radiance=None):
    """small triangles spread over the view, so that the tree has inner nodes to cull"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.5, 1.5, (n, 1, 3))
    return tri_mesh((c + rng.uniform(-0.2, 0.2, (n, 3, 3))).astype(np.float32), "filler", radiance)


# ------------------------------------------------------------------------------------------------ the adversarial scenes of the CPU file
def edge_in_a_side_plane():
    """a triangle edge on the plane x = 0, which for this camera (on the z axis, 32 pixels wide) is the side plane between the two
    tile columns -- and one on y = 0, between the rows"""
    a = [[0, -1, 0], [0, 1, 0], [1.5, 0, 0]]
    b = [[0, -1, -1], [0, 1, -1], [-1.5, 0, -1]]
    c = [[-1, 0, 0.5], [1, 0, 0.5], [0, 1.2, 0.5]]
    return tiny_scene([tri_mesh([a, b, c]), filler()])


def through_the_camera_plane():
    big = [[-0.5, -0.6, -3], [0.5, -0.6, -3], [0, 0.4, 9]]      # from in front of the camera (z = 4) to behind it
    return tiny_scene([tri_mesh([big]), filler()])


def camera_inside_boxes():
    """the camera inside the scene's box and inside leaf boxes: a shell of triangles around it"""
    p, f, _ = scenes.icosphere(1, 1.0, (0, 0, 4))
    shell = Mesh(p, f, bsdf=Bsdf("diffuse"), name="shell")
    near_tri = [[-0.3, -0.3, 3.9], [0.3, -0.3, 3.9], [0, 0.3, 4.3]]      # its box holds the camera
    return tiny_scene([shell, tri_mesh([near_tri]), filler()])


def flat_boxes():
    """axis-aligned triangles: zero-thickness boxes in x, y and z"""
    t = [[[-1, -1, 0], [1, -1, 0], [0, 1, 0]], [[0.25, -1, -1], [0.25, 1, -1], [0.25, 0, 1]], [[-1, -0.25, -1], [1, -0.25, -1], [0, -0.25, 1]]]
    return tiny_scene([tri_mesh(t), filler()])      # (the filler gives the tree inner nodes: a root that is a leaf gets no lists)


_CLIP_TRIS = [[[-0.05, -0.05, 3.95], [0.05, -0.05, 3.95], [0, 0.05, 3.95]],      # 0.05 from the camera, near = 0.5
              [[-9, -9, -8], [9, -9, -8], [0, 9, -8]],                            # 12 away, far = 10
              [[-1, -1, 0], [1, -1, 0], [0, 1, 0]]]


def near_and_far_clip():
    """one triangle in front of the near clip, one beyond the far clip, one between: only the last is ever hit"""
    return tiny_scene([tri_mesh(_CLIP_TRIS), filler(12)], near=0.5, far=10.0)


def only_clipped():
    """the first two alone: both are clipped for every ray.  (No case of cases(): whether the root of two triangles is a leaf is the builder's choice.)"""
    return tiny_scene([tri_mesh(_CLIP_TRIS[:2])], near=0.5, far=10.0)


def split_duplicates():
    """long thin diagonal triangles among small ones: the device builders split them, so leaves hold duplicated references (more
    pair slots than triangles); duplicates give identical candidates"""
    long_ones = [[[-1.8, -1.8, -1], [-1.7, -1.8, -1], [1.8, 1.8, 1]], [[-1.8, 1.8, 0.5], [-1.8, 1.7, 0.5], [1.8, -1.8, -0.5]]]
    return tiny_scene([tri_mesh(long_ones, "long"), filler(200, seed=9)])


def axis_aligned():
    """The exactly representable case: camera at (0, 0, 4) looking down -z with fov 90 (the tile borders of a 32 x 32 frame are the
    planes x = 0 and y = 0, slopes 0 and +-1), triangles with small-integer coordinates."""
    t = [[[-8, -8, 0], [8, -8, 0], [-8, 8, 0]], [[8, 8, 0], [-8, 8, 0], [8, -8, 0]],
         [[0, 0, 1], [1, 0, 1], [0, 1, 1]], [[0, 0, 2], [-1, 0, 2], [0, -1, 2]], [[-1, 1, 1], [0, 1, 1], [-1, 0, 1]]]
    return tiny_scene([tri_mesh(t)], fov=90.0)


# ------------------------------------------------------------------------------------------------ the base scene and what varies over it
def wall(z=-2.0, half=4.0):
    return tri_mesh([[[-half, -half, z], [half, -half, z], [half, half, z]], [[-half, -half, z], [half, half, z], [-half, half, z]]], "wall")


def base_meshes(n=120, seed=5, moved=False):
    f = filler(n, seed, radiance=(3.0, 2.0, 1.0))
    if moved:
        f.positions = (f.positions + np.float32(MOVED_BY)).astype(np.float32)
    return [f, wall()]


def base_to_world():
    return scenes.lookat(BASE_ORIGIN, (0, 0, 0), (0, 1, 0))


def _lin(m3):
    m = np.eye(4)
    m[:3, :3] = np.asarray(m3, np.float64)
    return m


def base_scene(size=BASE_SIZE, fov=45.0, post=None, to_world=None, near=1e-4, far=1e4, meshes=None, scale=1.0):
    """the base scene under to_world = L post (or the to_world given); scale multiplies the geometry, the camera's translation, near, far"""
    tw = base_to_world().astype(np.float64) if to_world is None else np.asarray(to_world, np.float64)
    if post is not None:
        tw = tw @ _lin(post)
    meshes = base_meshes() if meshes is None else meshes
    if scale != 1.0:
        tw = tw.copy()
        tw[:3, 3] *= scale
        for m in meshes:
            m.positions = (m.positions.astype(np.float64) * scale).astype(np.float32)
    cam = Camera(size[0], size[1], fov, near_clip=near * scale, far_clip=far * scale, to_world=tw.astype(np.float32))
    return Scene(meshes, cam, RFilter(), Integrator("normals"), 1)


def _rz(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return [[c, -s, 0], [s, c, 0], [0, 0, 1]]


def slivers(per_level=8, seed=13):
    """the construction of tests/tree_cases.py (_slivers): needles a, a + d, a + d / 2 + off with sin ~ 3e-3 (a wider pad), 3e-4 (much
    wider) and 2e-5 (numerically collinear: an unbounded box), in view over the wall, with a filler for inner nodes"""
    rng = np.random.default_rng(seed)
    n = 3 * per_level
    a = rng.uniform(-1, 1, (n, 3)); d = rng.normal(size=(n, 3)) * 0.4
    off = rng.normal(size=(n, 3)) * 0.4 * np.repeat([3e-3, 3e-4, 2e-5], per_level)[:, None]
    sl = np.stack([a, a + d, a + 0.5 * d + off], 1)
    col = np.float32([[[0, 0, 0], [1, 1, 1], [2, 2, 2.0000002]], [[-1, 0.5, 0.25], [-0.5, 0.5, 0.25], [0.75, 0.5, 0.25]]])
    return base_scene(meshes=[filler(60, seed=5, radiance=(3.0, 2.0, 1.0)), tri_mesh(sl, "slivers"), tri_mesh(col, "collinear"), wall()])


def at_the_near_plane(near=2.0, cells=4):
    """A patch of 2 cells^2 triangles IN the near-clip plane of a rigid camera on the z axis (depth = near exactly: whether a ray's
    t passes mint = fl(near / d.z) is decided by the roundings, and about half do), in front of a small filler.  The scene is kept
    small against the near distance: the leaf boxes' own pad, kBoxPadRel x the scene's diagonal (~3), must stay below near eps_z, or
    it hides a near-clip cull that has lost its margin."""
    z, g = 4.0 - near, np.linspace(-0.75, 0.75, cells + 1)
    t = []
    for i in range(cells):
        for j in range(cells):
            a, b, c, d = (g[i], g[j], z), (g[i + 1], g[j], z), (g[i + 1], g[j + 1], z), (g[i], g[j + 1], z)
            t += [[a, b, c], [a, c, d]]
    fill = filler()
    fill.positions = (fill.positions * np.float32(0.5)).astype(np.float32)
    return tiny_scene([tri_mesh(t, "patch"), fill], near=near)


def ties(reverse=False):
    """fuzz_intersect's "dups" (ten triangles, three coplanar copies of each), every copy a mesh of its own and an emitter of its own
    radiance; the larger global triangle id wins a tie, so the mesh order decides which copy a ray sees"""
    from tests.fuzz_intersect import make_meshes
    v = np.concatenate([m.positions for m in make_meshes(np.random.default_rng(41), "dups", 30, 1.0)]).reshape(-1, 3, 3)
    assert v.shape[0] == 30 and (v[:10] == v[10:20]).all() and (v[:10] == v[20:]).all()
    meshes = [tri_mesh(v[k:k + 1], f"copy{k // 10}-of-{k % 10}", radiance=(1.0 + k, 40.0 - k, 1.0 + (k * 7) % 30)) for k in range(30)]
    sc = base_scene(meshes=meshes[::-1] if reverse else meshes)
    sc.rfilter = RFilter("box")
    sc.integrator = Integrator("path_mats")
    return sc


OLD_KEYS = ("edge-in-a-side-plane", "through-the-camera-plane", "camera-inside-boxes", "flat-boxes", "near-and-far-clip", "split-duplicates", "axis-aligned")
TIE_KEYS = ("ties", "ties-reversed")


@functools.lru_cache(maxsize=None)
def cases():
    """((key, Scene, expect), ...) -- treat the scenes as read-only (copy before changing one)"""
    far_cam = scenes.lookat((30, 20, 500), (0, 0, 0), (0, 1, 0))
    small = lambda: base_meshes(24)
    out = [
        ("edge-in-a-side-plane", edge_in_a_side_plane(), "lists"), ("through-the-camera-plane", through_the_camera_plane(), "lists"),
        ("camera-inside-boxes", camera_inside_boxes(), "lists"), ("flat-boxes", flat_boxes(), "lists"), ("near-and-far-clip", near_and_far_clip(), "lists"),
        ("split-duplicates", split_duplicates(), "lists"), ("axis-aligned", axis_aligned(), "lists"),
        # cameras over the base scene
        ("base", base_scene(), "lists"),
        ("fov-2", base_scene(fov=2.0), "lists"),
        ("fov-150", base_scene(fov=150.0), "lists"),
        ("rolled-37", base_scene(post=_rz(37.0)), "lists"),
        ("scaled-3", base_scene(post=np.diag([3.0, 3.0, 3.0])), "lists"),
        ("stretched", base_scene(post=np.diag([1.0, 2.0, 0.5])), "lists"),
        ("sheared", base_scene(post=[[1, 0.7, 0], [0, 1, 0], [0, 0, 1]]), "lists"),
        ("mirrored", base_scene(post=np.diag([-1.0, 1.0, 1.0])), "lists"),
        ("far-narrow", base_scene(fov=0.6, to_world=far_cam), "lists"),
        ("clipped", base_scene(near=3.5, far=5.0), "lists"),
        ("at-the-near-plane", at_the_near_plane(), "lists"),
        ("ill-conditioned", base_scene(post=np.diag([1.0, 1.0, 1e-7])), "all-overflow"),
        ("scale-1e-3", base_scene(scale=1e-3), "lists"),
        ("scale-1e3", base_scene(scale=1e3), "lists"),
        ("frame-17x33", base_scene(size=(17, 33)), "lists"),
        ("frame-100x60", base_scene(size=(100, 60)), "lists"),
        ("frame-16x16", base_scene(size=(16, 16), meshes=small()), "lists"),
        ("frame-1x1", base_scene(size=(1, 1), meshes=small()), "lists"),
        ("leaf-root", base_scene(meshes=[wall()]), "walk"),
        ("slivers", slivers(), "lists"),
        ("ties", ties(False), "lists"),
        ("ties-reversed", ties(True), "lists"),
    ]
    assert all(sum(m.indices.shape[0] for m in sc.meshes) <= 250 for _, sc, _ in out)
    return tuple(out)


KEYS = tuple(c[0] for c in cases())
NEW_KEYS = tuple(k for k in KEYS if k not in OLD_KEYS)
EXPECT = {c[0]: c[2] for c in cases()}


def case(key):
    return next(c[1] for c in cases() if c[0] == key)


def n_tiles(key):
    cam = case(key).camera
    return ((cam.width + 15) // 16) * ((cam.height + 15) // 16)


def frame_integrators(key):
    return ("path_mats",) if key in TIE_KEYS else ("normals", "path_mis")
