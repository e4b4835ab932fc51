"""The compact path record of all-diffuse scenes (nori_amd/csrc/device/wf_records.h: derived pcg32 state, (T, pdf_mat) quad with a
12-byte L, Lsum in the place of Ld; wf_shade / wf_finish of wavefront.hip) against the full 100-byte record it replaces there: the
same draws and the same additions per path, so EVERY BIT of the bordered RGBW frame, the count of rejected samples and the ray
counts must be equal.

NORI_HIP_WF_RECORD=full (read once per process) forces the full record and the kernels of before for every scene, so the old frames
come from one child process that renders every case of this file with the switch set; this process renders the same cases with
the switch unset.  Both go through render_cases() below.  nori_render_stats.wf_record says which record a render used: eligible
scenes must say "compact" here and "full" in the child, scenes with a mirror or a dielectric "full" in both."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nori_amd.scene import Bsdf, Camera, Integrator, Mesh, RFilter, Scene, Texture
from tests import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_KEYS = ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid")
W, H, SPP = 45, 37, 40                # 3 x 3 tiles, clipped edge tiles
BATCH_SAMPLES = 9 * 256 * 7           # 40 samples per pixel of 9 tiles in six batches: tails beside the next batch (wf_tail_copy)
INTEGRATORS = ("path_mats", "path_ems", "path_mis")


def diffuse(integrator="path_mis", spp=SPP):
    """the Cornell box, every BSDF diffuse"""
    return scenes.cornell_box(W, H, spp, integrator, rfilter=RFilter("gaussian"))


def textured(integrator="path_mis"):
    sc = diffuse(integrator)
    img = np.random.default_rng(11).uniform(0.05, 0.95, (7, 9, 3)).astype(np.float32)
    sc.textures = [Texture("image", img, "bilinear", "repeat", 4.0, 4.0),
                   Texture("checkerboard", uscale=4.0, vscale=4.0, color0=(0.85, 0.3, 0.2), color1=(0.1, 0.5, 0.75))]
    by_name = {m.name: m for m in sc.meshes}
    by_name["floor"].albedo_texture = 0
    by_name["back"].albedo_texture = 1
    return sc


def no_emitter(integrator):
    sc = diffuse(integrator)
    sc.meshes = [m for m in sc.meshes if m.radiance is None]
    return sc


def white_box(integrator="path_mis", spp=8):
    """A closed box of albedo 0.99 around the camera and a small light: Russian roulette keeps a path with p ~ 0.99^depth, so many
    paths live for a hundred vertices and more -- past the 32 depths of wf_shade's table of skip pairs."""
    white = Bsdf("diffuse", (0.99, 0.99, 0.99))
    faces = [((-1, 0, -1), (-1, 0, 5), (1, 0, 5), (1, 0, -1)), ((-1, 2, -1), (1, 2, -1), (1, 2, 5), (-1, 2, 5)),
             ((-1, 0, -1), (1, 0, -1), (1, 2, -1), (-1, 2, -1)), ((-1, 0, 5), (-1, 2, 5), (1, 2, 5), (1, 0, 5)),
             ((-1, 0, -1), (-1, 2, -1), (-1, 2, 5), (-1, 0, 5)), ((1, 0, -1), (1, 0, 5), (1, 2, 5), (1, 2, -1))]
    m = []
    for k, q in enumerate(faces):
        v, f = scenes.quad(*q)
        m.append(Mesh(v, f, bsdf=white, name=f"wall{k}"))
    v, f = scenes.quad((-0.25, 1.98, -0.25), (0.25, 1.98, -0.25), (0.25, 1.98, 0.25), (-0.25, 1.98, 0.25))
    m.append(Mesh(v, f, bsdf=Bsdf("diffuse", (0, 0, 0)), radiance=(20.0, 20.0, 20.0), name="light"))
    cam = Camera(W, H, 40.0, to_world=scenes.lookat((0, 1, 4.2), (0, 1, 0), (0, 1, 0)))
    return Scene(m, cam, RFilter("gaussian"), Integrator(integrator), spp)


def with_sphere(bsdf):
    return scenes.cornell_box(W, H, SPP, "path_mis", sphere_bsdfs=[bsdf, Bsdf("diffuse")], rfilter=RFilter("gaussian"))


NO_FINISH, SHORT_FINISH, MIXED = {"NORI_HIP_WF_FINISH": "0"}, {"NORI_HIP_WF_FINISH_PATHS": "256"}, {"NORI_HIP_WF_FORCE_MIXED": "1"}


def cases():
    """[(key, scene, options, environment, render_host's keywords or {"tiles": [...]}, the record expected without the switch)]"""
    out = []
    for integ in INTEGRATORS:
        out.append((f"plain-{integ}", diffuse(integ), {}, {}, {}, "compact"))
        # every pass by wf_shade (stored rounds at every depth the paths reach) / wf_finish once 256 paths are left
        out.append((f"no-finish-{integ}", diffuse(integ), {}, NO_FINISH, {}, "compact"))
    out.append(("short-finish", diffuse(), {}, SHORT_FINISH, {}, "compact"))
    out.append(("spp-begin", diffuse(), {}, NO_FINISH, {"spp_begin": 7, "spp_count": 13}, "compact"))
    for rem in range(3):
        out.append((f"share-{rem}", diffuse(), {}, NO_FINISH, {"tile_mod": 3, "tile_rem": rem}, "compact"))
    out.append(("tile-list", diffuse(), {}, NO_FINISH, {"tiles": [1, 2, 5, 6, 8], "spp_begin": 3, "spp_count": 20}, "compact"))
    out.append(("tile-list-finish", diffuse(), {}, {}, {"tiles": [0, 4, 7]}, "compact"))
    out.append(("batches", diffuse(), {"wavefront_samples": BATCH_SAMPLES}, {}, {}, "compact"))
    out.append(("batches-short-finish", diffuse("path_ems"), {"wavefront_samples": BATCH_SAMPLES}, SHORT_FINISH, {}, "compact"))
    # regeneration: a pool of 2048 paths under a batch of the whole frame, every pass a mixed one -- depths differ per lane
    out.append(("mixed-pool", diffuse(), {"wavefront_paths": 2048, "wavefront_samples": 1 << 30}, dict(MIXED, **NO_FINISH), {}, "compact"))
    out.append(("mixed-pool-finish", diffuse("path_mats"), {"wavefront_paths": 2048, "wavefront_samples": 1 << 30}, MIXED, {}, "compact"))
    for integ in INTEGRATORS:
        out.append((f"white-box-{integ}", white_box(integ), {}, NO_FINISH, {}, "compact"))
    out.append(("white-box-finish", white_box(), {}, {}, {}, "compact"))
    out.append(("textured", textured(), {}, NO_FINISH, {}, "compact"))
    out.append(("textured-finish", textured("path_ems"), {}, {}, {}, "compact"))
    for integ in INTEGRATORS:
        out.append((f"no-emitter-{integ}", no_emitter(integ), {}, NO_FINISH, {}, "compact"))
    out.append(("mirror", with_sphere(Bsdf("mirror")), {}, NO_FINISH, {}, "full"))
    out.append(("dielectric", with_sphere(Bsdf("dielectric")), {}, {}, {}, "full"))
    return out


KEYS = [c[0] for c in cases()]
EXPECTED = {c[0]: c[5] for c in cases()}


def render_cases(out_dir):
    """Every case through the wavefront engine: <key>.npy and stats.json in out_dir."""
    from nori_amd.render import Renderer
    stats = {}
    for key, scene, options, env, kw, _ in cases():
        r = Renderer(0).upload(scene)
        r.set_option("engine", "wavefront")
        for k, v in options.items():
            r.set_option(k, v)
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            if "tiles" in kw:
                F, _, st = r.render_tiles_host(kw["tiles"], **{k: v for k, v in kw.items() if k != "tiles"})
            else:
                F, st = r.render_host(**kw)
        finally:
            for k, v in saved.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        r.close()
        np.save(os.path.join(out_dir, key + ".npy"), F)
        stats[key] = dict({k: int(st[k]) for k in STAT_KEYS + ("engine", "tail_cus")}, wf_record=st["wf_record"])
    with open(os.path.join(out_dir, "stats.json"), "w") as f:
        json.dump(stats, f)


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
assert os.environ.get("NORI_HIP_WF_RECORD") == "full"
from tests.test_gpu_records_compact import render_cases
render_cases(sys.argv[2])
"""


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """key -> (full-record frame, its stats, this process's frame, its stats)"""
    assert os.environ.get("NORI_HIP_WF_RECORD") is None, "this process must use the record the library picks"
    old_dir, new_dir = tmp_path_factory.mktemp("record_full"), tmp_path_factory.mktemp("record_picked")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(old_dir)], env=dict(os.environ, NORI_HIP_WF_RECORD="full"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    render_cases(str(new_dir))
    old, new = json.load(open(old_dir / "stats.json")), json.load(open(new_dir / "stats.json"))
    assert set(old) == set(new) == set(KEYS)
    return {k: (np.load(old_dir / (k + ".npy")), old[k], np.load(new_dir / (k + ".npy")), new[k]) for k in old}


@pytest.mark.parametrize("key", KEYS)
def test_same_bits_as_the_full_record(frames, key):
    A, sa, B, sb = frames[key]
    assert sa["engine"] == sb["engine"] == 1, (key, sa, sb)
    assert sa["wf_record"] == "full" and sb["wf_record"] == EXPECTED[key], (key, sa["wf_record"], sb["wf_record"])
    for k in STAT_KEYS:
        assert sa[k] == sb[k], (key, k, sa[k], sb[k])
    assert sb["n_camera_samples"] > 0 and sb["n_closest_rays"] >= sb["n_camera_samples"], (key, sb)
    assert A.dtype == B.dtype == np.float32 and A.shape == B.shape and A.shape[2] == 4, key
    assert (B[..., 3] > 0).any(), key
    diff = A.view(np.uint32) != B.view(np.uint32)
    assert not diff.any(), f"{key}: {int(diff.sum())} of {A.size} floats differ, max {np.abs(A - B).max():.3e}, first at {tuple(np.argwhere(diff)[0])}"
    if key.startswith("no-emitter"):        # nothing shines: the ray counts carry the check
        assert not B[..., :3].any() and sb["n_shadow_rays"] == 0 and sb["n_closest_rays"] > sb["n_camera_samples"]
    elif not key.startswith("tile-list"):
        assert B[..., :3].any(), key
    if key.startswith("batches"):
        assert sb["tail_cus"] > 0 and sa["tail_cus"] > 0, (key, sa, sb)      # the tails ran on the side copy
    if key.startswith("plain") or key.startswith("no-finish"):
        assert sb["n_camera_samples"] == W * H * SPP
