"""The scenes, light sets and inputs on which tests/test_gpu_delta_lights.py holds the device to tests/delta_lights_ref.py, and on
which tests/test_delta_lights_cpu.py shows -- without a GPU -- that these inputs reach every new branch (delta_lights_ref.EVENTS)
and that a wrong branch would change their radiance (delta_lights_ref.MUTATIONS).  Everything here is computed on the CPU, once.
The box's cases are 48 x 32; the OUTSIDE_LDS cases are path_cases.lights' 32 x 32 (size_of)."""
from __future__ import annotations

import functools

import numpy as np

from nori_amd.scene import Bsdf, Camera, Integrator, Light, Mesh, RFilter, Scene
from tests import delta_lights_ref as dl, light_cases as lc, path_cases as pc, scenes
from tests.backends import Oracle

F = np.float32
W, H = 48, 32                     # the box's frame; the OUTSIDE_LDS cases keep path_cases.lights' own 32 x 32: size_of(case)
SAMPLES = (0, 1, 2, 3)            # the frames: four single-sample frames under the box filter -- a pixel is Li of its path
N_LI = 4096                       # paths of nori_hip_li: the first 1024 pixels of each of the four samples
INTEGRATORS = ("path_ems", "path_mis")
CAP = pc.CAP                      # the walker's cap in vertices (it asserts that no path is alive there); the streams hold its draws
LONGEST = 192                     # ... and no path of any case takes more than this: the mirror wall and the glass sphere make chains
                                  # that Russian roulette keeps with probability 0.99 (the longest, in the fog, has 129 vertices)


def cos_deg(a):
    return float(np.cos(np.radians(a)))


# (a): one light of each type.  The point light lies 5e-5 ABOVE the ceiling (y = 2): a shadow ray towards it meets the ceiling
# 5e-5 / cos(theta) before the light, inside the kEpsilon its maxt leaves out for cos(theta) > 0.5 and outside it for the rest --
# maxt = dist would darken what maxt = dist - kEpsilon lights.  The spot looks down at the microfacet sphere, its band 15 degrees
# wide; the sun comes in through the box's open front.
POINT = Light("point", position=(0.8, 2.00005, 0.5), intensity=(2.0, 1.8, 1.5))
SPOT = Light("spot", position=(0.1, 1.7, 0.7), direction=(-0.55, -1.35, -1.0), intensity=(6.0, 6.0, 5.0), cos_inner=cos_deg(20), cos_outer=cos_deg(35))
SUN = Light("directional", direction=(0.2, -0.6, -0.8), intensity=(1.5, 1.4, 1.2))
INSIDE = Light("point", position=(-0.3, 1.2, 0.4), intensity=(1.0, 1.1, 1.3))


def many(n=257, seed=4):
    """n lights inside the box: points and spots, every 16th a sun; the last one is a spot"""
    r = np.random.default_rng(seed)
    out = []
    for k in range(n):
        pos = tuple(float(x) for x in r.uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9)))
        dirn = tuple(float(x) for x in r.normal(size=3) + (0, -1.5, 0))
        inten = tuple(float(x) for x in r.uniform(0.2, 1.5, 3))
        if k % 16 == 7:
            out.append(Light("directional", direction=(dirn[0], dirn[1], -abs(dirn[2]) - 0.5), intensity=inten))
        elif k % 2 or k == n - 1:
            out.append(Light("spot", pos, dirn, inten, cos_deg(25), cos_deg(60)))
        else:
            out.append(Light("point", pos, intensity=inten))
    return out


def box(integrator, lights, medium=None, env=None, area=True, light_normals=True):
    """path_cases.box with a microfacet and a glass sphere and a mirror for its left wall: mirror, glass, microfacet, a textured
    back wall and one area emitter (area=False: none -- the delta lights are the only lights but the environment).  The area
    emitter has path_cases.box's vertex normals, which lean outwards; light_normals=False: none -- the geometric normal (an emitter
    sample converts area to solid angle with the SHADING normal's cosine, a BSDF-sampled hit needs no conversion: with normals that
    are not the geometric one path_ems and path_mis estimate different integrals, whatever the lights)"""
    sc = pc.box(integrator, [pc.ROUGH, pc.GLASS], medium=medium, env=env)
    sc.camera.width, sc.camera.height = W, H
    sc = scenes_resized(sc)
    for m in sc.meshes:
        if m.name == "left":
            m.bsdf = pc.MIRROR
        if m.name == "light" and not light_normals:
            m.normals = None
    if not area:
        sc.meshes = [m for m in sc.meshes if m.radiance is None]
    sc.lights = list(lights)
    return sc


def scenes_resized(sc):
    """the same scene with the camera of W x H (the camera record is derived from width and height at upload)"""
    sc.camera = Camera(W, H, sc.camera.fov, to_world=sc.camera.to_world)
    return sc


def outside_lds(name, integrator, lights, medium=None, env=None):
    """path_cases.lights(name) -- many area lights, grown so that sampled rays hit them, whose tables do NOT fit the LDS -- with the
    delta lights `lights`: wf_shade<..., LDSTAB = false, ...> of the three delta-light sets, and the megakernel and li_kernel on
    unredirected table pointers.  emitter_pick reads a table of emitters + lights (+ 1) entries from global memory there."""
    sc = pc.lights(name, integrator, medium=medium, env=env)
    assert not lc.fits(lc.table_counts(sc))
    sc.lights = list(lights)
    return sc


CASES = {
    "a_each_type": lambda i: box(i, [POINT, SPOT, SUN]),
    "b_257": lambda i: box(i, many()),
    "c_each_type_sky": lambda i: box(i, [POINT, SPOT, SUN], env=pc._sky()),
    "d_fog": lambda i: box(i, [INSIDE, SPOT], medium=pc.FOG),
    "e_lights_only": lambda i: box(i, [INSIDE, SPOT, SUN], area=False),
    "f_lights_only_sky": lambda i: box(i, [INSIDE, SPOT, SUN], env=pc._sky(), area=False),
    "g_fog_r3": lambda i: outside_lds("R3", i, [INSIDE, SPOT], medium=pc.THIN_FOG),
    "h_sky_r4": lambda i: outside_lds("R4", i, [POINT, SPOT, SUN], env=pc._sky(3)),
    "i_r3": lambda i: outside_lds("R3", i, [POINT, SPOT, SUN]),
}
OUTSIDE_LDS = ("g_fog_r3", "h_sky_r4", "i_r3")      # one per delta-light set (with a medium, with an environment, alone)
# the light sets of (a) and (c) on the box whose area emitter has its geometric normal: what path_ems and path_mis are compared on
STAT_CASES = {
    "a_each_type": lambda i: box(i, [POINT, SPOT, SUN], light_normals=False),
    "c_each_type_sky": lambda i: box(i, [POINT, SPOT, SUN], env=pc._sky(), light_normals=False),
}
# mutation -> the cases on which tests/test_delta_lights_cpu.py requires it to change at least 8 paths under path_mis
SHOWN_ON = {
    "emitter_hit_pdf_without_lights_in_count": ("a_each_type", "b_257") + OUTSIDE_LDS,
    "env_at_unshifted_index": ("c_each_type_sky", "f_lights_only_sky", "h_sky_r4"),
    "mis_weight_from_quotient": ("a_each_type", "e_lights_only"),
    "no_falloff": ("a_each_type", "d_fog"),
    "no_tr_on_delta": ("d_fog", "g_fog_r3"),
    "maxt_is_dist": ("a_each_type",),
}


def applicable(sc, integrator):
    """the counters of delta_lights_ref.EVENTS whose branch exists in the case"""
    types = {l.type for l in sc.lights}
    fog, sky = sc.medium is not None, sc.environment is not None
    area = any(m.radiance is not None for m in sc.meshes)
    has = {
        "pick_point": "point" in types, "pick_spot": "spot" in types, "pick_directional": "directional" in types,
        "emitter_hit_lights_count": area and integrator == "path_mis",
        "env_pick_shifted": sky,
        "delta_at_medium_vertex": fog,
        "spot_in_band": "spot" in types,
        "delta_sample_mis": integrator == "path_mis",
        "delta_shadow": bool(types & {"point", "spot"}),
        "delta_tr": fog,
    }
    assert set(has) == set(dl.EVENTS)
    return tuple(k for k in dl.EVENTS if has[k])


@functools.lru_cache(maxsize=None)
def scene_of(case, integrator):
    return CASES[case](integrator)


def size_of(case):
    """(width, height) of the case's frame"""
    cam = scene_of(case, "path_mis").camera
    return cam.width, cam.height


@functools.lru_cache(maxsize=None)
def oracle_of(case):
    return Oracle(scene_of(case, "path_mis"), use_bvh=True)      # (neither the integrator nor the lights enter intersect)


@functools.lru_cache(maxsize=None)
def inputs(case, s):
    """path_cases.inputs_of at sample s: (idx, seq, floats, rays)"""
    return pc.inputs_of(scene_of(case, "path_mis"), s)


def walk(case, integrator, s, from_start=False, mutate=None, first=None):
    """delta_lights_ref.walk on the case's inputs of sample s: the frame's paths (the stream after the camera sample's four draws),
    or with from_start Li of the same rays with the stream drawn from the start, as nori_hip_li draws it; first: that many paths"""
    sc = scene_of(case, integrator)
    _, _, f, rays = inputs(case, s)
    f, rays = (f if from_start else f[:, 4:])[:first], rays[:first]
    return dl.walk(oracle_of(case), sc, integrator, rays, f, medium=sc.medium, env=sc.environment, max_vertices=CAP, mutate=mutate)


@functools.lru_cache(maxsize=None)
def reference(case, integrator, s, from_start=False, first=None):
    L, nc, ns, ev = walk(case, integrator, s, from_start, first=first)
    L.setflags(write=False)
    return L, nc, ns, ev


# ------------------------------------------------------------------ one diffuse quad under one point light
RHO = (0.6, 0.5, 0.4)
QUAD_LIGHT = Light("point", position=(0.3, 1.5, -0.2), intensity=(5.0, 4.0, 3.0))


def quad_scene(integrator, occluder=False):
    """a diffuse quad of albedo RHO in the plane y = 0 under QUAD_LIGHT, seen from above; the occluder is a small quad at y = 1
    between the light and the middle of the quad"""
    v, f = scenes.quad((-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2))
    m = [Mesh(v, f, bsdf=Bsdf("diffuse", RHO), name="quad")]
    if occluder:
        v, f = scenes.quad((0.0, 1.0, -0.5), (0.0, 1.0, 0.1), (0.6, 1.0, 0.1), (0.6, 1.0, -0.5))
        m.append(Mesh(v, f, bsdf=Bsdf("diffuse", (0.0, 0.0, 0.0)), name="occluder"))
    cam = Camera(64, 64, 50.0, to_world=scenes.lookat((0.2, 4.0, 0.3), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0)))
    sc = Scene(m, cam, RFilter("box"), Integrator(integrator), 1)
    sc.lights = [QUAD_LIGHT]
    return sc
