"""Scenes with many area lights of uneven triangle CDFs, and a numpy statement of the emitter pick (numpy only).

Emitter sampling (rt_path.h: emitter_pick, cdf_sample, emitter_point, sample_direct) picks an emitter uniformly, a triangle of it
by area (DiscretePDF::sample, include/nori/dpdf.h: std::lower_bound on the CDF) and a point by uniform barycentrics.  The other
procedural scenes have one light of two equal triangles, where 1/nE, x/nE and x*(1/nE) are one float and the binary search has no
uneven branch.  `many_lights` builds Cornell boxes with any number of lights of any triangle counts, sizes spread over decades,
zero-area triangles among them; REGIMES names the five scenes the tests use, one per way the kernels read the small tables
(shade_tables.h's fit test) and per shape of the tables' last 16-byte quad.
"""
from __future__ import annotations

import numpy as np

from nori_amd.scene import Bsdf, Integrator, Mesh, RFilter, Scene
from tests import scenes

# shade_tables.h: shade_tables_fit / shade_tables_to_lds -- kShadeMeshWords / (sizeof(MeshRec) / 4), kShadeEmitterWords, kShadeCdfWords
FIT_MAX_MESHES = 32
FIT_MAX_EMITTERS = 64        # never the binding limit: there are no more emitters than meshes
FIT_MAX_CDF = 960

LIGHT_Y = 1.98               # the plane of the light triangles, under the ceiling (y = 2)
SIZE_DECADES = 1.7           # edge lengths are drawn log-uniformly over this many decades: areas over twice as many
U24 = np.float32(2.0 ** -24)
ONE_MINUS = np.float32(1.0) - U24        # the largest float32 below 1


def _zero_area_lights(counts):
    """Indices into counts of the lights that get zero-area triangles: every second of those with more than two triangles."""
    big = [i for i, n in enumerate(counts) if n > 2]
    return set(big[::2])


def many_lights(counts, integrator="path_mis", width=48, height=32, spp=4, extra_meshes=0, with_normals_light=False, seed=1, rfilter=None, overlapping=False):
    """The Cornell box of tests/scenes.py without its light (walls, a microfacet and a diffuse sphere), plus one emitter mesh per
    entry of `counts` with that many triangles: black diffuse, a drawn radiance of its own.  Every light triangle lies in a cell
    of its own of a grid on the plane y = LIGHT_Y inside the box, facing down, so NO TWO LIGHT TRIANGLES OVERLAP (overlapping
    coplanar emitters are counted twice by emitter sampling and once by BSDF sampling: tests/test_light_cases_cpu.py measures it).
    Edge lengths are drawn over SIZE_DECADES decades.  In every second light with more than two triangles, triangles 0, 3, 6, ...
    have zero area (two equal vertices) -- triangle 0 among them, the only zero-area triangle std::lower_bound can return (for
    xiT = 0; a repeated CDF entry elsewhere resolves to the triangle before it).
    with_normals_light: one more light, a small icosphere with vertex normals (emitter_point's interpolated-normal branch).
    extra_meshes: that many small non-emitting quads on the floor, to raise the mesh count.
    overlapping: all triangles of a light in ONE cell, on top of each other -- only for measuring what the disjointness is for."""
    rng = np.random.default_rng(seed)
    sb = [Bsdf("microfacet", (0.2, 0.3, 0.1), 0.2), Bsdf("diffuse", (0.5, 0.5, 0.5))]
    base = scenes.cornell_box(width, height, spp, integrator, sphere_subdiv=1, sphere_bsdfs=sb, rfilter=rfilter)
    meshes = [m for m in base.meshes if m.radiance is None]
    total = int(sum(counts))
    g = max(4, int(np.ceil(np.sqrt(total))))
    cell = 1.9 / g
    cells = rng.permutation(g * g)[:total]
    zero_lights = _zero_area_lights(counts)
    black = Bsdf("diffuse", (0.0, 0.0, 0.0))
    k = 0
    for li, n in enumerate(counts):
        v = np.zeros((n, 3, 3), np.float64)
        for t in range(n):
            ck = cells[k - t] if overlapping else cells[k]; k += 1
            cx, cz = -0.95 + cell * (ck % g), -0.95 + cell * (ck // g)
            s = 0.9 * cell * 10.0 ** (-SIZE_DECADES * rng.uniform())
            a, b, c = s * rng.uniform(0.5, 1.0), s * rng.uniform(0.0, 1.0), s * rng.uniform(0.5, 1.0)
            v[t] = [(cx, LIGHT_Y, cz), (cx + a, LIGHT_Y, cz), (cx + b, LIGHT_Y, cz + c)]      # normal (0, -a c, 0): down
            if li in zero_lights and t % 3 == 0:
                v[t, 2] = v[t, 1]
        rad = tuple(float(x) for x in rng.uniform(5.0, 40.0, 3).astype(np.float32))
        meshes.append(Mesh(v.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3), bsdf=black, radiance=rad, name=f"light{li}"))
    if with_normals_light:
        p, f, nrm = scenes.icosphere(0, 0.08, (0.0, 1.55, 0.1))
        meshes.append(Mesh(p, f, nrm, bsdf=black, radiance=(30.0, 25.0, 20.0), name="light_normals"))
    for e in range(extra_meshes):
        x, z = -0.9 + 0.075 * (e % 24), 0.55 + 0.1 * (e // 24)
        v, f = scenes.quad((x, 0.01, z), (x, 0.01, z + 0.05), (x + 0.05, 0.01, z + 0.05), (x + 0.05, 0.01, z))
        meshes.append(Mesh(v, f, bsdf=Bsdf("diffuse", (0.3, 0.5, 0.7)), name=f"extra{e}"))
    return Scene(meshes, base.camera, rfilter or RFilter(), Integrator(integrator), spp)


def table_counts(scene):
    """(n_meshes, n_emitters, n_cdf) of the scene's small tables; n_cdf = sum of n_triangles + 1 over the emitters."""
    em = [m for m in scene.meshes if m.radiance is not None]
    return len(scene.meshes), len(em), int(sum(m.indices.shape[0] + 1 for m in em))


def fits(counts):
    """shade_tables.h's fit test on (n_meshes, n_emitters, n_cdf): the tables are read from LDS."""
    nm, ne, nc = counts
    return nm <= FIT_MAX_MESHES and ne <= FIT_MAX_EMITTERS and nc <= FIT_MAX_CDF


# 24 lights of 1 .. 90 triangles; the 25th brings the sum to 935 = 960 - 25
_R2_HEAD = (1, 1, 1, 2, 3, 4, 5, 7, 9, 11, 13, 16, 19, 23, 29, 31, 37, 41, 47, 53, 61, 71, 83, 90)
_R2 = _R2_HEAD + (935 - sum(_R2_HEAD),)
_R3 = _R2[:-1] + (_R2[-1] + 1,)

# name -> (many_lights arguments, expected (n_meshes, n_emitters, n_cdf), expected fit): 7 meshes are the box and the spheres
REGIMES = {
    "R1": (dict(counts=(1, 7, 40), seed=11), (10, 3, 51), True),                                          # n_cdf = 3 mod 4
    "R2": (dict(counts=_R2, seed=12), (32, 25, 960), True),                                               # both limits, exactly
    "R3": (dict(counts=_R3, seed=12), (32, 25, 961), False),                                              # one CDF entry too many
    "R4": (dict(counts=(2, 5, 3, 9), extra_meshes=22, seed=14), (33, 4, 23), False),                      # one mesh too many
    "R5": (dict(counts=(1, 4, 12, 6, 28), with_normals_light=True, seed=15), (13, 6, 77), True),          # 1 mod 4, 2 mod 4
}


def regime(name, integrator="path_mis", **kw):
    """The scene of regime `name`; its table counts and fit decision are asserted to be the stated ones."""
    args, counts, fit = REGIMES[name]
    sc = many_lights(integrator=integrator, **args, **kw)
    assert table_counts(sc) == counts, (name, table_counts(sc), counts)
    assert fits(counts) == fit, name
    return sc


def li_inputs(backend, scene, n, seed):
    """n camera rays through random film positions, with random seeds and sequences."""
    rng = np.random.default_rng(seed)
    ps = (rng.random((n, 2)) * [scene.camera.width, scene.camera.height]).astype(np.float32)
    return backend.sample_rays(ps), rng.integers(0, 2 ** 63, n, dtype=np.uint64), rng.integers(0, 2 ** 63, n, dtype=np.uint64)


# ------------------------------------------------------------------ the pick, stated in numpy, float32 operation by operation
def pick_reference(scene, tables, samples):
    """(mesh, tri, p) for samples [n, 4] = (xiE, xiT, xi1, xi2) over `tables` (Renderer.emitter_tables / Emu.emitter_tables: the
    CDF as the device holds it) and the scene's vertices:
        ei  = min(uint32(xiE * float32(nE)), nE - 1)
        tri = std::lower_bound over the emitter's n + 1 CDF entries, minus one, floored at 0, capped at n - 1   (dpdf.h)
        su = sqrt(1 - xi1), alpha = 1 - su, beta = xi2 su, gamma = 1 - alpha - beta, p = (alpha p0 + beta p1) + gamma p2."""
    x = np.ascontiguousarray(samples, np.float32).reshape(-1, 4)
    nE = tables["n_emitters"]
    one = np.float32(1.0)
    ei = np.minimum((x[:, 0] * np.float32(nE)).astype(np.int64), nE - 1)
    mesh = tables["emitters"][ei].astype(np.uint32)
    tri = np.zeros(x.shape[0], np.uint32)
    p0, p1, p2 = (np.zeros((x.shape[0], 3), np.float32) for _ in range(3))
    for mi in np.unique(mesh):
        sel = np.nonzero(mesh == mi)[0]
        first, n = int(tables["cdf_offset"][mi]), int(tables["n_triangles"][mi])
        cdf = tables["cdf"][first:first + n + 1]
        t = np.clip(np.searchsorted(cdf, x[sel, 1], side="left").astype(np.int64) - 1, 0, n - 1)
        tri[sel] = t
        m = scene.meshes[int(mi)]
        v = m.positions[m.indices[t].astype(np.int64)]      # [k, 3 corners, 3]
        p0[sel], p1[sel], p2[sel] = v[:, 0], v[:, 1], v[:, 2]
    su = np.sqrt(one - x[:, 2])
    alpha = one - su
    beta = x[:, 3] * su
    gamma = (one - alpha) - beta
    p = (alpha[:, None] * p0 + beta[:, None] * p1) + gamma[:, None] * p2
    assert su.dtype == np.float32 and p.dtype == np.float32
    return mesh, tri, p


def _neighbours(v):
    """v with both float32 neighbours of every element, kept to [0, 1]."""
    v = np.asarray(v, np.float32)
    a = np.concatenate([v, np.nextafter(v, np.float32(-1.0)), np.nextafter(v, np.float32(2.0))])
    return a[(a >= 0) & (a <= 1)].astype(np.float32)


def edge_samples(tables, n_uniform=100000, seed=5):
    """The samples the pick is compared on, [n, 4] float32 in [0, 1]:
      * n_uniform uniform samples;
      * per emitter: xiT at every entry of its CDF and at both float32 neighbours of every entry, and xiT in
        {0, 2^-24, 1 - 2^-24, 1};
      * xiE at k / nE for every k in 0 .. nE with both neighbours, and 0, 1 - 2^-24, 1;
      * per emitter: xi1 in {0, 1 - 2^-24, 1} x xi2 in {0, 1 - 2^-24}.
    The components a row does not sweep are uniform draws."""
    rng = np.random.default_rng(seed)
    nE = tables["n_emitters"]
    rows = [rng.random((n_uniform, 4), dtype=np.float32)]

    def block(xiE=None, xiT=None, xi1=None, xi2=None, n=None):
        n = n or max(np.size(a) for a in (xiE, xiT, xi1, xi2) if a is not None)
        b = rng.random((n, 4), dtype=np.float32)
        for col, a in enumerate((xiE, xiT, xi1, xi2)):
            if a is not None:
                b[:, col] = a
        rows.append(b)

    ends = np.array([0.0, U24, ONE_MINUS, 1.0], np.float32)
    for k in range(nE):
        mi = int(tables["emitters"][k])
        first, n = int(tables["cdf_offset"][mi]), int(tables["n_triangles"][mi])
        mid = np.float32((k + 0.5) / nE)      # well inside emitter k's share of xiE
        block(xiE=mid, xiT=np.concatenate([_neighbours(tables["cdf"][first:first + n + 1]), ends]))
        a, b = np.meshgrid(np.array([0.0, ONE_MINUS, 1.0], np.float32), np.array([0.0, ONE_MINUS], np.float32))
        block(xiE=mid, xi1=a.ravel(), xi2=b.ravel())
        block(xiE=mid, xiT=ends, xi1=np.float32(1.0))
    steps = np.arange(nE + 1, dtype=np.float32) / np.float32(nE)
    block(xiE=np.concatenate([_neighbours(steps), np.array([0.0, ONE_MINUS, 1.0], np.float32)]))
    out = np.concatenate(rows).astype(np.float32)
    assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0
    return out


def edge_counts(tables, samples, mesh, tri):
    """(samples whose xiT is exactly an entry of the picked emitter's CDF, samples whose picked triangle has zero area -- equal
    CDF entries at its two ends)."""
    x = np.ascontiguousarray(samples, np.float32).reshape(-1, 4)
    on_entry = zero_area = 0
    for mi in np.unique(mesh):
        sel = mesh == mi
        first, n = int(tables["cdf_offset"][mi]), int(tables["n_triangles"][mi])
        cdf = tables["cdf"][first:first + n + 1]
        on_entry += int(np.isin(x[sel, 1], cdf).sum())
        t = tri[sel].astype(np.int64)
        zero_area += int((cdf[t] == cdf[t + 1]).sum())
    return on_entry, zero_area


# ------------------------------------------------------------------ the CDF as uploaded
def mesh_areas_f32(mesh):
    """Per-triangle areas as scene_prep.cpp computes them: 0.5 * sqrt(|cross(p1 - p0, p2 - p0)|^2) in float32, no FMA."""
    v = mesh.positions[mesh.indices.astype(np.int64)]
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    d = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    a = np.float32(0.5) * np.sqrt(d)
    assert a.dtype == np.float32
    return a


def cdf_check(scene, tables):
    """Per emitter: the CDF starts at 0.0, ends at exactly 1.0 and never decreases (asserted).  Returns two worst ratios over the
    entries 1 <= k <= n of all emitters, the cumulative float32 triangle areas A_k summed in binary64:
      * of |cdf[k] - A_k / S| / (A_k / S) to (k + 2) 2^-24, S the float32 total the table is normalised by: entry k has gone
        through k float32 additions (the first of them exact) and the scaling by 1 / S, a reciprocal and a product -- the total is
        the given normaliser here, which is what makes this bound follow from those k additions and the scaling;
      * of |cdf[k] - A_k / A_n| / (A_k / A_n) to (k + n) 2^-24: against the binary64 total, so the n - 1 float32 additions behind S
        count as well.
    S is the sequential float32 sum of the areas; that it is the device's is asserted through the table's inv_area = 1 / S."""
    worst_table, worst_exact = 0.0, 0.0
    for mi in tables["emitters"]:
        mi = int(mi)
        first, n = int(tables["cdf_offset"][mi]), int(tables["n_triangles"][mi])
        cdf = tables["cdf"][first:first + n + 1]
        assert cdf[0] == 0.0 and cdf[-1] == 1.0 and (np.diff(cdf) >= 0).all(), mi
        areas = mesh_areas_f32(scene.meshes[mi])
        S = np.cumsum(areas, dtype=np.float32)[-1]      # (cumsum adds in sequence, as scene_prep.cpp does)
        assert np.float32(1.0) / S == tables["inv_area"][mi], mi
        cum = np.cumsum(areas.astype(np.float64))
        k = np.arange(1, n + 1)
        ok = cum > 0
        assert (cdf[1:][~ok] == 0).all(), mi
        for which, F, allowed in (("table", cum / float(S), k + 2), ("exact", cum / cum[-1], k + n)):
            ratio = np.abs(cdf[1:].astype(np.float64) - F)[ok] / F[ok] / (allowed[ok] * 2.0 ** -24)
            if which == "table":
                worst_table = max(worst_table, float(ratio.max()))
            else:
                worst_exact = max(worst_exact, float(ratio.max()))
    return worst_table, worst_exact
