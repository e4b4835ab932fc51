"""Random rounds for tests/test_gpu_path_fuzz.py, which holds li_kernel and both engines to tests/path_ref.py byte for byte on
them, and for tests/test_path_fuzz_cpu.py, which shows without a GPU what the committed rounds (SEEDS) reach.  Where
tests/path_cases.py has five hand-made scenes, a round here DRAWS its scene: a closed or half-open box, icospheres, a triangle
soup, area lights (leaning normals, a reflecting BSDF, facing away from the camera), the four BSDFs at the ends of their
parameters, textures with and without per-vertex texcoords, a fog or a sky or neither, a thin lens, a camera inside a glass body,
the tree builder, a ragged frame, the sample index and the wavefront knobs.

    python tests/path_fuzz.py [--seconds 60] [--seed 1000] [--lit]

runs rounds from any seed on a GPU (a long manual run; not part of the suite).

What keeps a round's paths short (tests/test_path_fuzz_cpu.py asserts LONGEST): Russian roulette keeps a path with probability
min(max3(T) eta^2, 0.99) per vertex, so a chain of vertices that leave max3(T) at 1 -- specular bounces, or a fog whose albedo has
a 1 -- ends only with probability 0.01 per vertex.  The generator therefore bounds what can chain: diffuse albedos, microfacet kd
and texels stay <= 0.8; at most one wall is a mirror; a fog with a 1 in its albedo fills a CLOSED box and has a mean free path of
at least the box's size, so that most of its paths' vertices are on surfaces (outside a half-open box such a fog has no surface
to end a path at).  It bounds nothing per path: a round whose longest path still exceeds
LONGEST is listed in SKIPPED with that length, whole.

A LIT round (LIT_SEEDS, lit_scene_of) is the round of its seed with drawn delta lights under path_ems or path_mis, held to
tests/delta_lights_ref.py: 1 to 4096 point, spot and directional lights -- in a wall's plane, half a kEpsilon off a wall on either
side, at a mesh vertex, inside a body, at the eye, behind the ceiling; black ones; hard-edged, full-sphere and hair-thin cones.
The draws of the plain rounds are untouched: the lights come from a generator of their own."""
from __future__ import annotations

import argparse
import functools
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nori_amd.scene import Bsdf, Camera, Environment, Integrator, Medium, Mesh, RFilter, Scene, Texture  # noqa: E402
from tests import envmap_ref as er, path_cases as pc, scenes  # noqa: E402

F = np.float32
BASE = 20264
PATHS = pc.PATHS
SAMPLE_INDICES = (0, 1, 5, 1 << 31, (1 << 32) - 1)
INT_IORS, EXT_IORS = (1.33, 1.5046, 2.4), (1.000277, 1.33)
ALPHAS = (0.01, 0.05, 0.2, 0.6, 1.0)
IMAGE_SHAPES = ((1, 1), (5, 12), (10, 3), (7, 9))
FREE_PATHS = (0.05, 0.5, 2.0, 20.0)      # mean free path / scene size
FOG_ALBEDOS = (0.0, 0.5, 0.9, 1.0)
GS = (-0.99, -0.5, 0.0, 5e-4, 1e-3, 0.6, 0.95, 0.99)
MAP_SIZES = (1, 2, 7, 16)
MAP_KINDS = ("random", "zeros", "range", "contrast")      # ("zeros": a third of the texels black)
APERTURES = (0.02, 0.1, 0.3)
SIZE = 2.0                               # the box is 2 wide, high and deep
KINDS = ("fog", "sky", "neither")
BRIGHTEST = 0.8                          # of a diffuse albedo, a kd, a texel

# The committed rounds: a run of consecutive seeds without the ones whose reference holds a path longer than LONGEST -- seed ->
# that round's longest path in vertices (frame stream, from-start stream), as tests/test_path_fuzz_cpu.py measures and asserts it.
LONGEST = 128
SKIPPED = {}
SEEDS = tuple(s for s in range(0, 36) if s not in SKIPPED)

# The lit rounds: scene_of(seed) with drawn delta lights (point, spot, directional; lit_scene_of) under path_ems or path_mis, held to
# tests/delta_lights_ref.py -- a run of consecutive seeds of their own, skipped for the same one reason.
LIT_SKIPPED = {}
LIT_SEEDS = tuple(s for s in range(36, 60) if s not in LIT_SKIPPED)
LIGHT_COUNTS = (1, 2, 3, 17, 256, 4096)      # (4096 is NORI_MAX_LIGHTS)
POSITION_CLASSES = ("anywhere", "in_a_wall_plane", "just_inside_a_wall", "just_outside_a_wall", "at_a_sphere_vertex", "at_a_sphere_centroid",
                    "at_the_eye", "above_the_box")
OFF_THE_WALL = 5e-5                          # half of kEpsilon: a shadow ray's maxt = dist - kEpsilon ends before or after the wall
CONES = ((20.0, 35.0), (30.0, 30.0), (0.0, 180.0), (10.0, 10.01), (60.0, 89.0))      # (inner, outer) in degrees; (0, 180) is cos 1 / -1


# ------------------------------------------------------------------ the draws (tests/fuzz_engines.py --features calls them too)
def draw_texture(rng):
    kind = "image" if rng.random() < 0.7 else "checkerboard"
    sign = lambda: 1.0 if rng.random() < 0.5 else -1.0
    t = Texture(kind, None, ("nearest", "bilinear")[int(rng.integers(2))], ("repeat", "clamp")[int(rng.integers(2))],
                sign() * float(rng.uniform(0.5, 6.0)), sign() * float(rng.uniform(0.5, 6.0)), float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)),
                tuple(rng.uniform(0.05, BRIGHTEST, 3)), tuple(rng.uniform(0.05, BRIGHTEST, 3)))
    if kind == "image":
        h, w = IMAGE_SHAPES[int(rng.integers(len(IMAGE_SHAPES)))]
        t.texels = rng.uniform(0.05, BRIGHTEST, (h, w, 3)).astype(F)
    return t


def draw_texcoords(rng, mesh, centre=None):
    """per-vertex texcoords that differ at the three corners of every triangle (asserted): a sphere's from the spherical
    coordinates of its vertices about `centre`, any other mesh's from its two widest axes -- either with a drawn affine map"""
    p = mesh.positions.astype(np.float64)
    if centre is not None:
        q = p - np.asarray(centre, np.float64)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        uv = np.stack([np.arctan2(q[:, 2], q[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(q[:, 1], -1, 1)) / np.pi], 1)
    else:
        ext = p.max(axis=0) - p.min(axis=0)
        a, b = np.argsort(-ext)[:2]
        uv = np.stack([(p[:, a] - p[:, a].min()) / ext[a], (p[:, b] - p[:, b].min()) / ext[b]], 1)
    ang = rng.uniform(0, 2 * np.pi)
    m = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]) * rng.uniform(0.6, 1.6)
    uv = (uv @ m.T + rng.uniform(-0.5, 0.5, 2)).astype(F)
    c = uv[mesh.indices.astype(np.int64)]
    for i, j in ((0, 1), (1, 2), (2, 0)):
        assert (c[:, i] != c[:, j]).any(axis=1).all()
    return uv


def draw_medium(rng, g=None, closed=True):
    ratio = FREE_PATHS[int(rng.integers(len(FREE_PATHS)))]
    allowed = FOG_ALBEDOS if closed and ratio >= 1.0 else FOG_ALBEDOS[:-1]      # (a 1 only where surfaces end the paths: the module's docstring)
    while True:
        albedo = tuple(float(allowed[int(k)]) for k in rng.integers(0, len(allowed), 3))
        if max(albedo) > 0:
            break
    if g is None:
        g = GS[int(rng.integers(len(GS)))]
    return Medium(1.0 / (ratio * SIZE), albedo, float(g))


def draw_environment(rng):
    n, kind = MAP_SIZES[int(rng.integers(len(MAP_SIZES)))], MAP_KINDS[int(rng.integers(len(MAP_KINDS)))]
    return Environment(er.make_map(n, kind, int(rng.integers(1 << 16))), tuple(rng.uniform(0.3, 2.5, 3)), er.rotation(int(rng.integers(1 << 30))))


def draw_lens(rng):
    """(aperture_radius, focus_distance), or None: a pinhole with probability two thirds"""
    if rng.random() < 2.0 / 3.0:
        return None
    return APERTURES[int(rng.integers(len(APERTURES)))], float(rng.uniform(1.0, 3.0))


def draw_bsdf(rng, kinds=("diffuse", "mirror", "dielectric", "microfacet")):
    k = kinds[int(rng.integers(len(kinds)))]
    if k == "diffuse":
        return Bsdf("diffuse", tuple(rng.uniform(0.1, BRIGHTEST, 3)))
    if k == "mirror":
        return Bsdf("mirror")
    if k == "dielectric":
        return Bsdf("dielectric", int_ior=INT_IORS[int(rng.integers(3))], ext_ior=EXT_IORS[int(rng.integers(2))])
    return Bsdf("microfacet", tuple(rng.uniform(0.05, BRIGHTEST, 3)), ALPHAS[int(rng.integers(len(ALPHAS)))])


def _light(rng, k, eye):
    """area light k: a quad under the ceiling that faces down, or one that stands in the box and faces the back wall, away from
    the camera; its normals may lean outwards at the corners (path_cases.box) and its BSDF may reflect"""
    s = float(rng.uniform(0.1, 0.5))
    away = rng.random() < (0.3 if k else 0.1)
    if away:
        c = np.array([rng.uniform(-0.5, 0.5), rng.uniform(0.5, 1.4), rng.uniform(-0.6, min(0.2, eye[2] - 0.5))])
        v, f = scenes.quad(c + [-s, -s, 0], c + [-s, s, 0], c + [s, s, 0], c + [s, -s, 0])      # faces -z
        lean = np.array([(-0.4, -0.4, -1), (-0.4, 0.4, -1), (0.4, 0.4, -1), (0.4, -0.4, -1)], np.float64)
    else:
        c = np.array([rng.uniform(-0.5, 0.5), 1.98 - 0.03 * k, rng.uniform(-0.5, 0.5)])
        v, f = scenes.quad(c + [-s, 0, -s], c + [s, 0, -s], c + [s, 0, s], c + [-s, 0, s])      # faces -y
        lean = np.array([(-0.4, -1, -0.4), (0.4, -1, -0.4), (0.4, -1, 0.4), (-0.4, -1, 0.4)], np.float64)
    normals = (lean / np.linalg.norm(lean, axis=1, keepdims=True)).astype(F) if rng.random() < 0.4 else None
    albedo = tuple(rng.uniform(0.2, 0.7, 3)) if rng.random() < 0.4 else (0.0, 0.0, 0.0)
    return Mesh(v, f, normals, bsdf=Bsdf("diffuse", albedo), radiance=tuple(rng.uniform(2.0, 20.0, 3) / (4 * s * s) * 0.25), name="light_away" if away else "light")


def kind_of(seed):
    """fog, sky or neither: in turn, and a fog's g through GS in turn -- any 24 consecutive seeds hold all of GS.  Everything else
    of a round is drawn from np.random.default_rng([BASE, seed])."""
    return KINDS[seed % 3], GS[(seed // 3) % len(GS)]


@functools.lru_cache(maxsize=None)
def scene_of(seed):
    """(Scene, builder, knobs) of round `seed`; knobs: S (the sample index the frame is rendered at), wavefront_paths,
    wavefront_samples, env (the wavefront engine's environment knobs) and, for the record, kind / closed / inside_glass"""
    rng = np.random.default_rng([BASE, seed])
    kind, g = kind_of(seed)
    while True:
        w, h = int(rng.integers(9, 41)), int(rng.integers(9, 41))
        if w % 16 or h % 16:
            break
    integrator = PATHS[int(rng.integers(3))]
    s_index = SAMPLE_INDICES[int(rng.integers(len(SAMPLE_INDICES)))]
    n_lights = int(rng.integers(0, 4))
    if kind == "sky":
        n_lights = 0 if rng.random() < 1.0 / 3.0 else max(n_lights, 1)
    else:
        n_lights = max(n_lights, 1)
    closed = rng.random() < (0.25 if kind == "sky" else 0.5) and not (kind == "sky" and n_lights == 0)      # (a sky that nothing sees lights nothing)
    eye = np.array([rng.uniform(-0.3, 0.3), rng.uniform(0.6, 1.4), rng.uniform(0.75, 0.95) if closed else rng.uniform(0.9, 1.8)])

    meshes, textures, can_texture = [], [], []
    walls = {"floor": ((-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1)), "ceiling": ((-1, 2, -1), (1, 2, -1), (1, 2, 1), (-1, 2, 1)),
             "back": ((-1, 0, -1), (1, 0, -1), (1, 2, -1), (-1, 2, -1)), "left": ((-1, 0, -1), (-1, 2, -1), (-1, 2, 1), (-1, 0, 1)),
             "right": ((1, 0, -1), (1, 0, 1), (1, 2, 1), (1, 2, -1))}
    if closed:
        walls["front"] = ((-1, 0, 1), (-1, 2, 1), (1, 2, 1), (1, 0, 1))
    mirror_wall = list(walls)[int(rng.integers(len(walls)))] if rng.random() < 0.2 else None
    for name, q in walls.items():
        v, f = scenes.quad(*q)
        bsdf = Bsdf("mirror") if name == mirror_wall else draw_bsdf(rng, ("diffuse", "diffuse", "diffuse", "microfacet"))
        meshes.append(Mesh(v, f, bsdf=bsdf, name=name))
        can_texture.append((len(meshes) - 1, None))
    budget = 2                                                               # subdivision 2 (320 triangles) for one sphere at most
    for k in range(int(rng.integers(1, 4))):
        sub = int(rng.integers(0, budget + 1))
        budget = 1 if sub == 2 else budget
        r = float(rng.uniform(0.2, 0.4))
        c = (float(rng.uniform(-0.6, 0.6)), float(rng.uniform(r, 1.4)), float(rng.uniform(-0.6, 0.6)))
        p, f, n = scenes.icosphere(sub, r, c, bool(rng.random() < 0.6))
        meshes.append(Mesh(p, f, n, bsdf=draw_bsdf(rng), name=f"sphere{k}"))
        can_texture.append((len(meshes) - 1, c))
    if rng.random() < 0.4:
        v, f = scenes.triangle_soup(int(rng.integers(1, 201)), int(rng.integers(1 << 30)), 0.8, float(rng.uniform(0.05, 0.3)))
        meshes.append(Mesh(v + np.array([0, 1, 0], F), f, bsdf=draw_bsdf(rng), name="soup"))
    inside_glass = rng.random() < 0.125
    if inside_glass:
        p, f, n = scenes.icosphere(1, 0.4, tuple(eye), bool(rng.random() < 0.5))
        meshes.append(Mesh(p, f, n, bsdf=draw_bsdf(rng, ("dielectric",)), name="glass_about_the_camera"))

    # textures: on some of the diffuse walls and spheres, every other one of them (the first included) with texcoords of its own
    k = 0
    for mi, centre in can_texture:
        m = meshes[mi]
        if m.bsdf.type != "diffuse" or not rng.random() < (0.6 if centre is not None else 0.4):
            continue
        textures.append(draw_texture(rng))
        m.albedo_texture = len(textures) - 1
        if k % 2 == 0:
            m.texcoords = draw_texcoords(rng, m, centre)
        k += 1

    for k in range(n_lights):
        meshes.append(_light(rng, k, eye))

    cam = Camera(w, h, float(rng.uniform(40, 75)), to_world=scenes.lookat(tuple(eye), (float(rng.uniform(-0.2, 0.2)), float(rng.uniform(0.6, 1.0)), -0.5), (0, 1, 0)))
    lens = draw_lens(rng)
    if lens is not None:
        cam.aperture_radius, cam.focus_distance = lens
    sc = Scene(meshes, cam, RFilter("box"), Integrator(integrator), 1, textures)
    sc.medium = draw_medium(rng, g, closed) if kind == "fog" else None
    sc.environment = draw_environment(rng) if kind == "sky" else None
    assert sc.n_triangles <= 800

    builder = int(rng.integers(0, 3))
    quarter = -(-(w * h) // 4)
    pools = (256, -(-quarter // 256) * 256, 1 << 14)
    knobs = {"S": s_index, "wavefront_paths": int(pools[int(rng.integers(3))]), "wavefront_samples": int(pools[int(rng.integers(3))]),
             "env": {"NORI_HIP_WF_FINISH_PATHS": str(int(rng.choice([256, 4096, 1 << 19]))), "NORI_HIP_WF_SYNC_EVERY": str(int(rng.choice([1, 2, 6])))},
             "kind": kind, "closed": bool(closed), "inside_glass": bool(inside_glass)}
    return sc, builder, knobs


def light_count_of(seed):
    """the number of delta lights of lit round `seed`: LIGHT_COUNTS in turn, shifted by two per kind, so that any 18 consecutive
    seeds hold every count under every kind (seed // 3 advances once per fog / sky / neither triple)"""
    return LIGHT_COUNTS[(seed // 3 + 2 * (seed % 3)) % len(LIGHT_COUNTS)]


def cone_cosines(inner, outer):
    return (1.0, -1.0) if (inner, outer) == (0.0, 180.0) else (float(np.cos(np.radians(inner))), float(np.cos(np.radians(outer))))


def draw_lights(rng, sc, closed, n, seed):
    """(lights, classes, cones): n delta lights for the scene sc of scene_of(seed), from a generator of their own.
    Types: every fifth light is directional, never in a fog (the setter refuses it); the others are points or spots by a draw.
    Positions: POSITION_CLASSES in turn over the lights that have a position, beginning at class `seed`; classes[k] is the
    class' index, -1 for a directional light.  cones[k] is the index into CONES of a spot, -1 otherwise."""
    from nori_amd.scene import Light
    eye = sc.camera.to_world[:3, 3].astype(np.float64)
    spheres = [m for m in sc.meshes if m.name.startswith("sphere")]
    walls = [("floor", 1, 0.0, 1.0), ("ceiling", 1, 2.0, -1.0), ("back", 2, -1.0, 1.0), ("left", 0, -1.0, 1.0), ("right", 0, 1.0, -1.0)]      # (name, axis, plane, inward)
    if closed:
        walls.append(("front", 2, 1.0, -1.0))
    in_box = lambda: np.array([rng.uniform(-0.95, 0.95), rng.uniform(0.05, 1.95), rng.uniform(-0.95, 0.95)])
    lights, classes, cones = [], [], []
    placed = 0
    for k in range(n):
        u = rng.random()
        inten = rng.uniform(0.2, 6.0, 3)
        if u < 0.1:                                   # a tenth are black: no radiance, and the shadow ray is traced all the same
            inten[:] = 0.0
        elif u < 0.1 + 1.0 / 7.0:                     # a further seventh have one channel at zero
            inten[int(rng.integers(3))] = 0.0
        inten = tuple(float(x) for x in inten)
        target = in_box()
        if sc.medium is None and (k + seed) % 5 == 4:
            d = target - np.array([rng.uniform(-3, 3), rng.uniform(2.5, 6.0), rng.uniform(-1.0, 5.0)])      # from above and mostly from the front
            lights.append(Light("directional", direction=tuple(float(x) for x in d), intensity=inten))
            classes.append(-1)
            cones.append(-1)
            continue
        c = (placed + seed) % len(POSITION_CLASSES)
        placed += 1
        name = POSITION_CLASSES[c]
        if name == "anywhere":
            pos = in_box()
        elif name == "in_a_wall_plane":               # the ceiling's or a side wall's plane, exactly
            _, axis, plane, _ = walls[(1, 3, 4)[int(rng.integers(3))]]
            pos = in_box()
            pos[axis] = plane
        elif name in ("just_inside_a_wall", "just_outside_a_wall"):
            _, axis, plane, inward = walls[int(rng.integers(len(walls)))]
            pos = in_box()
            pos[axis] = plane + (OFF_THE_WALL if name == "just_inside_a_wall" else -OFF_THE_WALL) * inward
        elif name == "at_a_sphere_vertex":            # the float32 coordinates themselves
            m = spheres[int(rng.integers(len(spheres)))]
            pos = m.positions[int(rng.integers(m.positions.shape[0]))].astype(np.float64)
        elif name == "at_a_sphere_centroid":          # inside the body: lit through glass, dark inside an opaque one
            m = spheres[int(rng.integers(len(spheres)))]
            pos = m.positions.astype(np.float64).mean(axis=0)
        elif name == "at_the_eye":
            pos = eye.copy()
        else:                                         # 3 units above the box: behind the ceiling from everywhere inside
            pos = np.array([rng.uniform(-0.95, 0.95), 5.0, rng.uniform(-0.95, 0.95)])
        pos = tuple(float(x) for x in np.asarray(pos, F))
        classes.append(c)
        if rng.random() < 0.5:
            lights.append(Light("point", pos, intensity=inten))
            cones.append(-1)
        else:
            ci = int(rng.integers(len(CONES)))
            axis_ = target - np.asarray(pos, np.float64)
            if not np.abs(axis_).max() > 1e-3:
                axis_ = np.array([0.0, -1.0, 0.0])
            cin, cout = cone_cosines(*CONES[ci])
            lights.append(Light("spot", pos, tuple(float(x) for x in axis_), inten, cin, cout))
            cones.append(ci)
    return lights, classes, cones


@functools.lru_cache(maxsize=None)
def lit_scene_of(seed):
    """(Scene, builder, knobs) of LIT round `seed`: scene_of(seed) -- its geometry, materials, textures, kind, lens, camera, builder, S
    and knobs -- with path_ems (even seeds) or path_mis (odd) for its integrator and light_count_of(seed) delta lights drawn from
    np.random.default_rng([BASE, seed, 1]); knobs gains light_classes and light_cones (draw_lights)."""
    import dataclasses
    sc, builder, kn = scene_of(seed)
    rng = np.random.default_rng([BASE, seed, 1])
    lights, classes, cones = draw_lights(rng, sc, kn["closed"], light_count_of(seed), seed)
    lit = dataclasses.replace(sc, integrator=Integrator(("path_ems", "path_mis")[seed % 2]), lights=lights)
    return lit, builder, dict(kn, light_classes=tuple(classes), light_cones=tuple(cones))


def round_of(seed, lit=False):
    return lit_scene_of(seed) if lit else scene_of(seed)


def describe(seed, lit=False):
    """the drawn configuration in one line"""
    sc, builder, kn = round_of(seed, lit)
    cam = sc.camera
    what = [f"seed {seed}: {sc.integrator.type} {cam.width}x{cam.height} S={kn['S']} builder {builder}", "closed" if kn["closed"] else "half-open"]
    if sc.medium is not None:
        what.append(f"fog sigma_t={sc.medium.sigma_t:g} albedo={sc.medium.albedo} g={sc.medium.g:g}")
    if sc.environment is not None:
        what.append(f"sky n={sc.environment.texels.shape[0]} black texels={int((sc.environment.texels == 0).all(axis=2).sum())}")
    if cam.aperture_radius > 0:
        what.append(f"lens r={cam.aperture_radius:g} f={cam.focus_distance:.3g}")
    if kn["inside_glass"]:
        what.append("camera inside glass")
    for m in sc.meshes:
        b = m.bsdf
        tag = {"diffuse": "d", "mirror": "m", "dielectric": f"g{b.int_ior:g}/{b.ext_ior:g}", "microfacet": f"r{b.alpha:g}"}[b.type]
        if m.albedo_texture is not None:
            t = sc.textures[m.albedo_texture]
            tag += f"[{t.kind[:3]} {t.filter[:3]} {t.wrap[:3]}{' uv' if m.texcoords is not None else ''}]"
        if m.radiance is not None:
            tag += "*" + ("n" if m.normals is not None else "") + ("r" if any(x > 0 for x in b.albedo) else "")
        what.append(f"{m.name}:{tag}:{m.indices.shape[0]}")
    if sc.lights:
        types = [l.type for l in sc.lights]
        held = sorted(set(kn["light_classes"]) - {-1})
        what.append(f"{len(sc.lights)} delta lights: " + " ".join(f"{types.count(t)} {t}" for t in ("point", "spot", "directional") if t in types)
                    + "; positions " + (" ".join(POSITION_CLASSES[c] for c in held) if len(held) < len(POSITION_CLASSES) else "of every class")
                    + "; cones " + " ".join("%g/%g" % CONES[c] for c in sorted(set(kn["light_cones"]) - {-1})))
    what.append(f"pool {kn['wavefront_paths']} batch {kn['wavefront_samples']} {' '.join(kn['env'].values())}")
    return ", ".join(what)


# ------------------------------------------------------------------ inputs and reference, as tests/path_cases.py has them per case
@functools.lru_cache(maxsize=None)
def inputs(seed):
    sc, _, kn = scene_of(seed)
    return pc.inputs_of(sc, kn["S"])


@functools.lru_cache(maxsize=None)
def oracle_of(seed):
    from tests.backends import Oracle
    return Oracle(scene_of(seed)[0], use_bvh=True)


def walk(seed, from_start=False, mutate=None, lit=False):
    """path_ref.walk of the round's frame under the round's integrator (from_start: of nori_hip_li's stream); of a lit round
    delta_lights_ref.walk -- on the same inputs and oracle: neither the integrator nor the lights enter them"""
    sc = round_of(seed, lit)[0]
    if not lit:
        return pc.walk_scene(sc, oracle_of(seed), inputs(seed), sc.integrator.type, from_start, mutate)
    from tests import delta_lights_ref as dl
    _, _, f, rays = inputs(seed)
    return dl.walk(oracle_of(seed), sc, sc.integrator.type, rays, f if from_start else f[:, 4:], medium=sc.medium, env=sc.environment, max_vertices=pc.CAP, mutate=mutate)


@functools.lru_cache(maxsize=None)
def reference(seed, from_start=False, lit=False):
    """walk(), computed once and shared read-only"""
    L, nc, ns, ev = walk(seed, from_start, lit=lit)
    L.setflags(write=False)
    return L, nc, ns, ev


def longest_path(seed, lit=False):
    """the vertices of the round's longest path: of the frame's stream and, for a pinhole round, of nori_hip_li's"""
    streams = (False,) if scene_of(seed)[0].camera.aperture_radius > 0 else (False, True)
    return max(int(reference(seed, fs, lit)[3]["vertices"].max()) for fs in streams)


# ------------------------------------------------------------------ one round on a GPU
def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=1).sum())


def one_round(seed, make_renderer, lit=False):
    """The three parts of tests/test_gpu_paths.py on round `seed` (lit: on lit round `seed`), every comparison an equality of bytes;
    make_renderer(scene, builder=...) gives the uploaded renderer.  Prints the seed, the configuration and the differing paths of
    every part before it asserts.  Returns the rays traced."""
    sc, builder, kn = round_of(seed, lit)
    what = describe(seed, lit)
    print(what)
    r = make_renderer(sc, builder=builder)
    if builder == 1:      # (the radix tree, which assert_built_where_asked does not know)
        assert r.accel_info()["built_on_device"] == 1, (what, r.accel_info())
    else:
        from tests.test_gpu_parity import assert_built_where_asked
        assert_built_where_asked(r, builder)
    assert (r.medium is not None) == (sc.medium is not None) and (r.environment_size > 0) == (sc.environment is not None), what
    assert len(r.lights) == len(sc.lights) and bool(sc.lights) == lit, what
    idx, seq, f, rays = inputs(seed)
    cam = sc.camera
    w, h, n = cam.width, cam.height, cam.width * cam.height
    integrator = sc.integrator.type
    # 1. Li of the stated rays; through a lens the rays themselves
    if cam.aperture_radius > 0:
        assert r.lens == (float(F(cam.aperture_radius)), float(F(cam.focus_distance))), what
        got = r.sample_rays_lens(np.stack([(idx % w).astype(F) + f[:, 0], (idx // w).astype(F) + f[:, 1]], 1), f[:, 2:4])
        print(f"seed {seed} lens rays:", int((got.view(np.uint32).reshape(n, -1) != rays.view(np.uint32).reshape(n, -1)).any(axis=1).sum()), "of", n, "differ")
        assert got.tobytes() == rays.tobytes(), what
    else:
        want_li = reference(seed, True, lit)[0]
        got_li = r.li(rays, idx, seq)
        print(f"seed {seed} li:", differing(got_li, want_li), "of", n, "paths differ")
        assert got_li.tobytes() == want_li.tobytes(), (what, differing(got_li, want_li))
    # 2. both engines' frames of sample S under the box filter: a pixel is Li of its path
    want, nc, ns, _ = reference(seed, False, lit)
    frames = {}
    for e, engine in enumerate(("megakernel", "wavefront")):
        r.set_option("engine", engine)
        frame, st = r.render_host(spp_count=1, spp_begin=kn["S"])
        assert st["engine"] == e and st["n_camera_samples"] == n, what
        assert frame.shape == (h, w, 4) and (frame[..., 3] == 1).all(), what
        got = frame[..., :3].reshape(-1, 3)
        print(f"seed {seed} {engine}:", differing(got, want), "of", n, "paths differ; rays", st["n_closest_rays"], st["n_shadow_rays"], "want", nc, ns)
        assert got.tobytes() == want.tobytes(), (what, engine, differing(got, want))
        assert (st["n_closest_rays"], st["n_shadow_rays"]) == (nc, ns), (what, engine)
        assert st["n_invalid"] == 0, what
        if engine == "wavefront" and (lit or sc.medium is not None or sc.environment is not None):
            assert st["wf_record"] == "full", what      # a fog, a sky or delta lights: a general variant, on the full record
        frames[engine] = frame
    # 3. the drawn pool, batch and finish knobs: regeneration, many passes, wf_finish early or never
    r.set_option("wavefront_paths", kn["wavefront_paths"])
    r.set_option("wavefront_samples", kn["wavefront_samples"])
    old = {k: os.environ.get(k) for k in kn["env"]}
    os.environ.update(kn["env"])
    try:
        small, st = r.render_host(spp_count=1, spp_begin=kn["S"])
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    print(f"seed {seed} wavefront under its knobs:", differing(small[..., :3].reshape(-1, 3), want), "of", n, "paths differ")
    assert st["engine"] == 1 and st["n_invalid"] == 0 and (st["n_closest_rays"], st["n_shadow_rays"]) == (nc, ns), what
    assert small.tobytes() == frames["wavefront"].tobytes(), (what, differing(small[..., :3].reshape(-1, 3), want))
    return nc + ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--lit", action="store_true", help="the rounds with drawn delta lights")
    a = ap.parse_args()
    from nori_amd.render import Renderer
    t0, n, rays, skipped = time.time(), 0, 0, []
    while time.time() - t0 < a.seconds:
        seed = a.seed + n
        n += 1
        try:
            longest = longest_path(seed, a.lit)
        except AssertionError:      # (the walker's: a path alive at path_cases.CAP)
            longest = pc.CAP + 1
        if longest > LONGEST:      # (the walker has ended every path within path_cases.CAP; the suite's rounds stay under half of it)
            skipped.append((seed, longest))
            continue
        made = []

        def make(scene, **kw):
            made.append(Renderer(0).upload(scene, **kw))
            return made[-1]
        try:
            rays += one_round(seed, make, a.lit)
        finally:
            for r in made:
                r.close()
    print(f"path_fuzz: {n - len(skipped)} rounds from seed {a.seed}, {rays} rays, li and both engines equal the CPU walker byte for byte; skipped (seed, longest path): {skipped}")


if __name__ == "__main__":
    main()
