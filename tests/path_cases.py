"""The scenes and inputs on which tests/test_gpu_paths.py holds the device to tests/path_ref.py, and on which
tests/test_path_ref_cpu.py shows -- without a GPU -- that these inputs reach every branch under test (path_ref.EVENTS) and that
a wrong branch would change their radiance (path_ref.MUTATIONS).  Everything here is computed on the CPU, once per case."""
from __future__ import annotations

import functools

import numpy as np

from nori_amd.scene import Bsdf, Environment, Medium, RFilter, Texture
from tests import envmap_ref as er, lens_ref as lr, light_cases as lc, path_ref as pr, scenes
from tests.backends import Oracle

F = np.float32
W, H = 32, 32
N_PATHS = W * H
S = 3                      # the sample index the frames are rendered at (spp_begin = S != 0, spp_count = 1)
PATHS = ("path_mats", "path_ems", "path_mis")

# Russian roulette (from depth 3 on) keeps a path with probability min(max3(T) eta^2, 0.99): 0.99 at most per vertex, and that
# only along chains of specular bounces and inside the glass (eta^2 = 2.26) -- a diffuse wall leaves max3(T) <= 0.725, the fog
# 0.9.  The inputs are fixed (pcg32 seeded with the pixel index and S), so the longest path is a property of the cases below:
# tests/test_path_ref_cpu.py walks every case -- under each integrator, the frame's paths and nori_hip_li's -- and asserts that
# none takes more than LONGEST vertices, half the cap; the walker asserts that no path is alive after CAP vertices: the reference
# alone ends every path, with as many vertices again to spare.
LONGEST = 127
CAP = 256

FOG = Medium(0.8, (0.9, 0.8, 0.7), 0.6)      # a mean free path of 1.25: the box is 2 wide, a sphere 0.7
THIN_FOG = Medium(0.3, (0.9, 0.8, 0.7), 0.6)


def _sky(seed=7):
    return Environment(er.make_map(16, "contrast"), (2.0, 2.0, 2.5), er.rotation(seed))


def box(integrator, spheres, medium=None, env=None, lens=None):
    """The Cornell box of tests/scenes.py, open towards the camera, seen from just outside the opening: two spheres with vertex
    normals, an image texture on the back wall, and its one area light with vertex normals that lean outwards at the corners (the
    interpolated normal of a light sample or of a light hit is not the geometric one)."""
    sc = scenes.cornell_box(W, H, 1, integrator, sphere_bsdfs=spheres, rfilter=RFilter("box"))
    by_name = {m.name: m for m in sc.meshes}
    sc.textures = [Texture("image", np.random.default_rng(11).uniform(0.05, 0.95, (7, 9, 3)).astype(F), "bilinear", "repeat", 4.0, 4.0)]
    by_name["back"].albedo_texture = 0
    light = by_name["light"]
    lean = np.array([(-0.4, -1, -0.4), (0.4, -1, -0.4), (0.4, -1, 0.4), (-0.4, -1, 0.4)], np.float64)
    light.normals = (lean / np.linalg.norm(lean, axis=1, keepdims=True)).astype(F)
    light.positions[:, [0, 2]] *= F(2.4)      # 1.2 x 1.2: large enough that phase- and BSDF-sampled rays of a small frame hit it
    sc.camera.fov = 58.0
    sc.camera.to_world = scenes.lookat((0.0, 0.85, 1.6), (0.0, 0.45, 0.0), (0.0, 1.0, 0.0))
    sc.medium, sc.environment = medium, env
    if lens is not None:
        sc.camera.aperture_radius, sc.camera.focus_distance = lens
    assert all(by_name[k].normals is not None for k in ("sphere1", "sphere2", "light"))
    return sc


def lights(name, integrator, medium=None, env=None):
    """light_cases.regime(name): many lights whose tables do not fit the LDS.  Its light triangles span 1.7 decades of edge length
    below their grid cell's, so small that a BSDF- or phase-sampled ray of a 1024-path frame all but never hits one; here every
    triangle is grown about its first vertex, an edge e to E (e / E)^(1/8) with E = 0.9 cells: still uneven, still one triangle
    per cell (no two overlap), the zero-area triangles still zero, the table counts the regime's own."""
    sc = lc.regime(name, integrator, width=W, height=H, spp=1, rfilter=RFilter("box"))
    counts = lc.table_counts(sc)
    em = [m for m in sc.meshes if m.radiance is not None]
    E = 0.9 * 1.9 / max(4, int(np.ceil(np.sqrt(sum(m.indices.shape[0] for m in em)))))      # (the grid of light_cases.many_lights)
    for m in em:
        assert m.indices.tobytes() == np.arange(m.positions.shape[0], dtype=np.uint32).tobytes()
        v = m.positions.astype(np.float64).reshape(-1, 3, 3)
        e = np.abs(v[:, 1:] - v[:, :1]).max(axis=(1, 2))
        assert (e > 0).all() and (e <= E * (1 + 1e-6)).all()
        m.positions[:] = (v[:, :1] + (v - v[:, :1]) * ((E / e) ** 0.875)[:, None, None]).reshape(-1, 3).astype(F)
    assert lc.table_counts(sc) == counts and not lc.fits(counts)
    sc.medium, sc.environment = medium, env
    return sc


GLASS, MIRROR, ROUGH = Bsdf("dielectric"), Bsdf("mirror"), Bsdf("microfacet", (0.2, 0.3, 0.1), 0.2)

# name -> (scene(integrator), builder)
CASES = {
    "fog_box": (lambda i: box(i, [MIRROR, GLASS], medium=FOG), 2),
    "sky_box": (lambda i: box(i, [ROUGH, GLASS], env=_sky()), 0),
    "fog_r3": (lambda i: lights("R3", i, medium=THIN_FOG), 0),
    "sky_r4": (lambda i: lights("R4", i, env=_sky(3)), 0),
    "sky_box_lens": (lambda i: box(i, [ROUGH, GLASS], env=_sky(), lens=(0.06, 2.0)), 0),
}
OUTSIDE_LDS = ("fog_r3", "sky_r4")
# mutation -> the cases on which tests/test_path_ref_cpu.py requires it to change at least 8 paths under path_mis: the boxes that
# have the branch, and the OUTSIDE_LDS cases (the LDSTAB = false kernels) for the branches that read the emitter tables there.
# (medium_vertex_keeps_discrete is not asked of fog_r3: it shows only where a phase-sampled ray hits a light, a handful of paths
# under that scene's many small lights.)
SHOWN_ON = {"roulette_without_eta": ("fog_box", "sky_box"), "emitter_hit_pdf_without_env_in_count": ("sky_box", "sky_r4"),
            "medium_vertex_keeps_discrete": ("fog_box",), "env_escape_weighted_after_discrete": ("sky_box",),
            "no_tr_at_surface_nee": ("fog_box", "fog_r3"), "texture_not_in_nee": ("fog_box", "sky_box"),
            "no_nee_at_microfacet": ("sky_box", "fog_r3", "sky_r4"), "geometric_normal_on_emitters": ("fog_box", "sky_box")}


# the counters these cases are about: path_ref.EVENTS without the ones that tests/path_fuzz.py's rounds are there to reach
COUNTERS = tuple(k for k in pr.EVENTS if k not in pr.FUZZ_EVENTS)


def applicable(sc, integrator):
    """The counters of path_ref.EVENTS whose branch exists in the scene under the integrator, from what the scene holds: a fog or
    a sky, the BSDF types, area lights, vertex normals on surfaces and on lights, a texture.  tests/test_path_ref_cpu.py requires
    each of them on at least 8 paths of the case."""
    ems, mis = integrator != "path_mats", integrator == "path_mis"
    fog, sky = sc.medium is not None, sc.environment is not None
    types = {m.bsdf.type for m in sc.meshes}
    glass, discrete, rough = "dielectric" in types, bool(types & {"mirror", "dielectric"}), "microfacet" in types
    area = any(m.radiance is not None for m in sc.meshes)
    has = {
        "rr_eta": glass,
        "medium_vertex_prev_discrete": fog,      # (the camera ray is discrete)
        "medium_vertex_after_specular": fog and discrete,
        "medium_vertex_inside_glass": fog and glass,
        "env_escape_after_discrete": sky and discrete,
        "env_escape_weighted": sky and bool(types & {"diffuse", "microfacet"}),
        "emitter_hit_env_count": sky and mis and area,
        "nee_microfacet_area": ems and rough and area,
        "nee_microfacet_env": ems and rough and sky,
        "nee_textured": ems and any(m.albedo_texture is not None for m in sc.meshes),
        "hit_vertex_normals": any(m.normals is not None for m in sc.meshes),
        "pick_light_normals": ems and any(m.normals is not None and m.radiance is not None for m in sc.meshes),
        "shadow_tr_surface": ems and fog and area,
    }
    assert set(has) == set(COUNTERS)
    return tuple(k for k in COUNTERS if has[k])


@functools.lru_cache(maxsize=None)
def scene_of(case, integrator):
    return CASES[case][0](integrator)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(idx, seq, floats [n, 4 + CAP * 8], rays): the streams pcg32(pixel index, S) and the camera rays of sample S of every pixel --
    the oracle's camera, or tests/lens_ref.py's thin lens"""
    return inputs_of(scene_of(case, "path_mis"), S)


def inputs_of(sc, s):
    """inputs() of any scene's frame at sample index s (tests/path_fuzz.py's rounds too)"""
    w, h = sc.camera.width, sc.camera.height
    idx = np.arange(w * h, dtype=np.uint64)
    seq = np.full(idx.shape, s, np.uint64)
    f = Oracle.pcg32_floats(idx, seq, 4 + CAP * pr.DRAWS_PER_VERTEX)
    ps, ap = lr.camera_samples(w, h, s)
    assert ps.tobytes() == np.stack([(idx % w).astype(F) + f[:, 0], (idx // w).astype(F) + f[:, 1]], 1).tobytes() and ap.tobytes() == f[:, 2:4].tobytes()
    cam = sc.camera
    if cam.aperture_radius > 0:
        rays = lr.as_rays(lr.lens_rays(sc, ps, ap, cam.aperture_radius, cam.focus_distance))
    else:
        rays = Oracle(sc).sample_rays(ps)
    for a in (f, rays):
        a.setflags(write=False)
    return idx, seq, f, rays


@functools.lru_cache(maxsize=None)
def oracle_of(case):
    return Oracle(scene_of(case, "path_mis"), use_bvh=True)      # (the integrator does not enter intersect)


def walk(case, integrator, from_start=False, mutate=None):
    """path_ref.walk on the case's inputs: the frame's paths (the stream after the camera sample's four draws), or with
    from_start Li of the same rays with the stream drawn from the start, as nori_hip_li draws it"""
    return walk_scene(scene_of(case, integrator), oracle_of(case), inputs(case), integrator, from_start, mutate)


def walk_scene(sc, oracle, inp, integrator, from_start=False, mutate=None):
    """path_ref.walk of any scene on its inputs_of()"""
    _, _, f, rays = inp
    return pr.walk(oracle, sc, integrator, rays, f if from_start else f[:, 4:], medium=sc.medium, env=sc.environment, max_vertices=CAP, mutate=mutate)


@functools.lru_cache(maxsize=None)
def reference(case, integrator, from_start=False):
    """walk(), computed once and shared read-only"""
    L, nc, ns, ev = walk(case, integrator, from_start)
    L.setflags(write=False)
    return L, nc, ns, ev
