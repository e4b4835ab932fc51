"""The grids, rays and scenes on which tests/test_gpu_grid_medium.py holds the device to tests/grid_medium_ref.py, and on which
tests/test_grid_medium_cpu.py shows -- without a GPU -- that these inputs reach every branch of the walk (grid_medium_ref.BRANCHES)
and that a wrong walk would change the radiance of the scenes' paths (grid_medium_ref.MUTATIONS).  Everything here is computed on
the CPU, once."""
from __future__ import annotations

import functools

import numpy as np

from nori_amd.scene import GridMedium
from tests import grid_medium_ref as gr, light_cases as lc, path_cases as pc
from tests.backends import Oracle

F = np.float32
INF = F(np.inf)
XI_MAX = F(1.0 - 2.0 ** -24)
CAP = pc.CAP
SAMPLES = (0, 3)
PATHS = pc.PATHS


def _rho(shape, seed, zeros):
    r = np.random.default_rng(seed)
    rho = r.uniform(0.5, 2.0, shape).astype(F)
    rho[r.uniform(size=shape) < zeros] = 0
    return rho


def _g16():
    rho = _rho((16, 16, 16), 3, 0.1)
    rho[4:9, 6:12, 2:7] = 0      # a block of zeros
    return rho


# name -> GridMedium.  Boxes and cell sizes: "g1" and "g16" have cubic cells of a power of two (crossings of several axes tie
# exactly), "g235" has cells 1, 0.5 and 0.4 (the last not a float), "g64" is a row of 64 voxels.
GRIDS = {
    "g1": lambda: GridMedium(np.ones((1, 1, 1), F), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 0.75, (0.9, 0.8, 0.7), 0.6),
    "g235": lambda: GridMedium(_rho((5, 3, 2), 1, 0.25), (-1.0, 0.0, -1.0), (1.0, 1.5, 1.0), 1.5, (0.9, 0.8, 0.7), 0.6),
    "g16": lambda: GridMedium(_g16(), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 3.0, (0.9, 0.8, 0.7), 0.0),
    "g64": lambda: GridMedium(_rho((1, 1, 64), 2, 0.2), (-2.0, -0.25, 0.5), (2.0, 0.25, 1.0), 2.0, (1.0, 1.0, 1.0), -0.4),
    # 2 x 2 x 2 unit cells with ONE voxel that is not empty: where the ORDER of a tie shows (tie_rays below)
    "gtie_x": lambda: GridMedium(_one_voxel(1, 0, 0), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 1.0),
    "gtie_y": lambda: GridMedium(_one_voxel(0, 1, 0), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 1.0),
}
TIE_GRIDS = ("gtie_x", "gtie_y")


def _one_voxel(x, y, z):
    rho = np.zeros((2, 2, 2), F)
    rho[z, y, x] = 1
    return rho


def tie_rays(name):
    """Rays on which the order of a tie decides the result.  They start in the empty voxel (0, 0, 0) of a gtie grid with xi = 0 --
    tau_stop = 0, so the first voxel that is not empty gives an event at the point where it is entered, even over a length of
    zero -- and reach the planes of two or three axes at the same t exactly (direction components of exactly 1 from a point at
    equal, representable distances).  Stepping x, then y, then z visits, over a length of zero, the voxel across the FIRST tying
    axis: in gtie_x that is the one voxel with density, (1, 0, 0), for ties of x with y, with z and with both, and the event lies at
    the tie; any order that steps another axis first passes through empty voxels only and finds no event at all.  In gtie_y the
    voxel is (0, 1, 0) and the ties are of y with z: it is reached iff y steps before z."""
    r = np.random.default_rng(5)
    fam = {"gtie_x": ((1, 1, 0), (1, 0, 1), (1, 1, 1)), "gtie_y": ((0, 1, 1),)}[name]
    O, D = [], []
    for tie in fam:
        for k in range(16):
            a = float(2.0 ** -r.integers(1, 4)) * float(r.integers(1, 4)) / 4.0      # k / 2^m: exact
            d = np.array([1.0 if t else float(r.uniform(0.05, 0.3)) for t in tie])
            o = np.array([-a if t else -0.5 for t in tie])
            O.append(o); D.append(d)
    n = len(O)
    return np.array(O, F), np.array(D, F), np.full(n, INF, F), np.zeros(n, F)


@functools.lru_cache(maxsize=None)
def grid(name):
    return GRIDS[name]()


@functools.lru_cache(maxsize=None)
def rays(name):
    """(o, d, tmax, xi) of about 1000 queries of the grid: the adversarial families below, then random ones"""
    g = gr.as_grid(grid(name))
    r = np.random.default_rng(sum(map(ord, name)))
    lo, hi = g.bmin.astype(np.float64), g.bmax.astype(np.float64)
    ext, mid = hi - lo, (hi + lo) / 2
    n = g.n
    O, D, T, X = [], [], [], []

    def add(o, d, tmax=None, xi=None):
        o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
        k = o.shape[0]
        O.append(o.astype(F)); D.append(d.astype(F))
        T.append(np.full(k, INF, F) if tmax is None else np.broadcast_to(np.asarray(tmax, F), (k,)))
        X.append(r.uniform(0, 1, k).astype(F) if xi is None else np.broadcast_to(np.asarray(xi, F), (k,)))

    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def lattice(k):
        """k lattice corners, exactly as the walk forms a plane: bmin + (float) i cell"""
        i = np.stack([r.integers(0, n[a] + 1, k) for a in range(3)], 1)
        return (g.bmin + (i.astype(F) * g.cell).astype(F)).astype(F), i

    inside = lambda k: lo + ext * r.uniform(0.02, 0.98, (k, 3))
    sphere = lambda k: mid + unit(r.normal(size=(k, 3))) * np.linalg.norm(ext) * 1.5
    # misses: from outside, pointing away; and past a corner
    o = sphere(48)
    add(o, unit(o - mid))
    add(sphere(16), unit(r.normal(size=(16, 3))))
    # from outside, aimed at a point inside; xi random, 0 and the largest; a finite tmax that ends inside; dist = inf
    o = sphere(160)
    d = unit(inside(160) - o)
    add(o[:96], d[:96])
    add(o[96:112], d[96:112], xi=0.0)
    add(o[112:128], d[112:128], xi=XI_MAX)
    add(o[128:], d[128:], tmax=np.linalg.norm(o[128:] - mid, axis=1))
    # from inside; a tmax shorter than a cell; unnormalised directions
    o = inside(160)
    d = unit(r.normal(size=(160, 3)))
    add(o[:64], d[:64])
    add(o[64:80], d[64:80], xi=0.0)
    add(o[80:96], d[80:96], xi=XI_MAX)
    add(o[96:128], d[96:128], tmax=r.uniform(0.05, 0.9, 32) * float(g.cell.min()))
    add(o[128:], d[128:] * r.uniform(0.3, 3.0, (32, 1)))
    # ties: from a lattice corner along a cell's diagonal in two axes (and something in the third), and along its space diagonal
    for k_axes in (2, 3):
        o, _ = lattice(48)
        sign = r.choice([-1.0, 1.0], (48, 3))
        d = sign * g.cell.astype(np.float64)
        if k_axes == 2:
            a = r.integers(0, 3, 48)
            d[np.arange(48), a] *= r.uniform(0.1, 0.7, 48)
        add(o, d)
        add(o - d * 0.5, d)      # ... and from half a diagonal before it (outside the box for corners on its faces)
    # parallel axes: a component that is +0, -0 or below 2^-40, the origin inside its slab, on its planes, and outside
    for val in (0.0, -0.0, 5e-13, -9e-13):
        o = inside(24)
        d = unit(r.normal(size=(24, 3)))
        a = r.integers(0, 3, 24)
        d[np.arange(24), a] = val
        add(o, d)                                   # inside the slab
        o2 = o.copy()
        o2[np.arange(24), a] = np.where(r.uniform(size=24) < 0.5, lo[a] - r.uniform(0.01, 1, 24), hi[a] + r.uniform(0.01, 1, 24))
        o2[:4, :] = o[:4]
        o2[np.arange(4), a[:4]] = hi[a[:4]]         # exactly on bmax: outside
        o2[4:8, :] = o[4:8]
        o2[np.arange(4, 8), a[4:8]] = lo[a[4:8]]    # exactly on bmin: inside
        add(o2, d)
    add(inside(8), np.zeros((8, 3)))                # no direction at all: a miss
    # origins exactly on planes, edges and corners of the lattice, random directions (both signs of every component)
    o, _ = lattice(96)
    o[:32, 0] = inside(32)[:, 0].astype(F)          # on an edge (two planes)
    o[32:64, :2] = inside(32)[:, :2].astype(F)      # on a plane
    add(o, unit(r.normal(size=(96, 3))))
    # the event in the last voxel: xi a little below what the whole walk would need
    o = sphere(96)
    d = unit(inside(96) - o)
    tau, _ = gr.optical_depth(g, o.astype(F), d.astype(F), INF)
    xi = (1.0 - np.exp(-tau.astype(np.float64) * r.uniform(0.97, 0.9999, 96))).astype(F)
    add(o, d, xi=np.minimum(xi, XI_MAX))
    # random ones
    o = mid + r.uniform(-1.2, 1.2, (200, 3)) * ext
    add(o, unit(r.normal(size=(200, 3))), tmax=np.where(r.uniform(size=200) < 0.5, INF, r.uniform(0, 4, 200)))
    if name in TIE_GRIDS:
        for lst, a in zip((O, D, T, X), tie_rays(name)):
            lst.append(a)
    out = tuple(np.ascontiguousarray(np.concatenate(x)) for x in (O, D, T, X))
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ scenes for whole paths
def _bbox(sc):
    pts = np.concatenate([m.positions for m in sc.meshes])
    return pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)


def box_grid(g=0.6):
    """2 x 3 x 5 voxels, a quarter of them empty, partly inside path_cases.box (x, z in -1 .. 1, y in 0 .. 2, open at z = 1, the
    camera at z = 1.6): it sticks out through the right wall and through the opening, and leaves the left third of the room, the
    floor and the ceiling in vacuum -- rays miss it, start in it, end in it, and leave the scene through it"""
    return GridMedium(_rho((5, 3, 2), 5, 0.25), (-0.4, 0.15, -0.7), (1.4, 1.45, 1.3), 2.0, (0.9, 0.8, 0.7), g)


def box(integrator, g=0.6, lights=(), light_normals=True):
    """path_cases.box with a microfacet and a glass sphere, a mirror for its left wall and the textured back wall, in box_grid"""
    sc = pc.box(integrator, [pc.ROUGH, pc.GLASS])
    for m in sc.meshes:
        if m.name == "left":
            m.bsdf = pc.MIRROR
        if m.name == "light" and not light_normals:
            m.normals = None
    sc.medium = box_grid(g)
    sc.lights = list(lights)
    return sc


def many_lights(integrator, lights=()):
    """path_cases.lights("R3"): emitter tables that do not fit the LDS; the grid covers the middle of the scene's bounds"""
    sc = pc.lights("R3", integrator)
    assert not lc.fits(lc.table_counts(sc))
    lo, hi = _bbox(sc)
    mid, ext = (lo + hi) / 2, np.maximum(hi - lo, 0.5)
    sc.medium = GridMedium(_rho((5, 3, 2), 6, 0.25), tuple(mid - 0.3 * ext), tuple(mid + 0.3 * ext), 1.5 / float(ext.max()), (0.9, 0.8, 0.7), 0.6)
    sc.lights = list(lights)
    return sc


def _delta():
    from tests import delta_light_cases as dc
    return [dc.INSIDE, dc.SPOT, dc.SUN]      # one point, one spot and one directional light


CASES = {
    "box_g06": lambda i: box(i, 0.6),
    "box_g0": lambda i: box(i, 0.0),
    "box_lit": lambda i: box(i, 0.6, _delta()),
    "r3": lambda i: many_lights(i),
    "r3_lit": lambda i: many_lights(i, _delta()),
}


def integrators(case):
    return ("path_ems", "path_mis") if case.endswith("_lit") else PATHS


@functools.lru_cache(maxsize=None)
def scene_of(case, integrator):
    return CASES[case](integrator)


@functools.lru_cache(maxsize=None)
def oracle_of(case):
    return Oracle(scene_of(case, "path_mis"), use_bvh=True)      # (neither the integrator, the lights nor the medium enter intersect)


@functools.lru_cache(maxsize=None)
def inputs(case, s):
    return pc.inputs_of(scene_of(case, "path_mis"), s)


def walk(case, integrator, s, from_start=False, mutate=None):
    sc = scene_of(case, integrator)
    _, _, f, rays_ = inputs(case, s)
    return gr.walk(oracle_of(case), sc, integrator, rays_, f if from_start else f[:, 4:], max_vertices=CAP, mutate=mutate)


@functools.lru_cache(maxsize=None)
def reference(case, integrator, s, from_start=False):
    out = walk(case, integrator, s, from_start)
    out[0].setflags(write=False)
    return out
