"""The compact path record of all-diffuse scenes (nori_amd/csrc/device/wf_records.h, rt_sampling.h) on the CPU, bit for bit, through
tests/records_compact/harness.cpp -- a stand-alone program built here with g++, once plain and once with
-fsanitize=address,undefined, and run as a process of its own:

1. closed form: rng_state_derived against rng_seed + n draws, for the draw counts of the three path integrators at depths 0 .. 5
   (Russian roulette starts at 3), the last depth of the kernels' table of skip pairs, the first past it and a few hundred beyond,
   with the seed of pixel (4095, 4095) of a 4096 x 4096 frame and streams next to 2^31;
2. lock-step walk: every path of a scene walked at once through vertex_pack / vertex_unpack with a carried pcg32 state and through
   vertex_pack_diffuse / vertex_unpack_diffuse with the derived state and Lsum; after every stored vertex the rng state, T, L,
   pdf_mat, eta, flags and both rays must be equal, at the end the radiance.  Scenes: the Cornell box (all diffuse), the same
   without its emitter, a closed box of albedo 0.99 (paths outlive the table).  A record with F_END_AFTER_B cannot arise from
   diffuse BSDFs alone (bsdf_sample and bsdf_eval vanish together), so the harness packs every vertex that has a shadow ray once
   more with end_after_shadow set and takes it through the consuming pass in both forms ("forced")."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from nori_amd import _capi as capi
from tests import scenes
from tests.test_gpu_records_compact import no_emitter, white_box

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "records_compact", "harness.cpp")
PREP = os.path.join(os.path.dirname(HERE), "nori_amd", "csrc", "device", "scene_prep.cpp")
CXXFLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-comment", "-Wno-unused-function", "-Wno-misleading-indentation"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]}
INTEGRATORS = ("path_mats", "path_ems", "path_mis")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = {}
    d = tmp_path_factory.mktemp("records_compact")
    procs = {name: subprocess.Popen(["g++"] + CXXFLAGS + flags + ["-o", str(d / name), SRC, PREP], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for name, flags in BUILDS.items()}
    for name, p in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, log
        out[name] = str(d / name)
    return out


def write_scene(path, sc):
    """the file harness.cpp's read_scene reads; every BSDF diffuse"""
    cam = sc.camera
    with open(path, "wb") as f:
        f.write(b"RCS1")
        f.write(struct.pack("<3i", capi.INTEGRATOR_NAMES[sc.integrator.type], cam.width, cam.height))
        f.write(struct.pack("<3f", cam.fov, cam.near_clip, cam.far_clip))
        f.write(np.asarray(cam.to_world, dtype="<f4").reshape(16).tobytes())
        f.write(struct.pack("<I", len(sc.meshes)))
        for m in sc.meshes:
            assert m.bsdf.type == "diffuse" and m.albedo_texture is None
            f.write(struct.pack("<3I", m.positions.shape[0], m.indices.shape[0], 0 if m.normals is None else 1))
            f.write(struct.pack("<3f", *m.bsdf.albedo))
            f.write(struct.pack("<i", 0 if m.radiance is None else 1))
            f.write(struct.pack("<3f", *(m.radiance or (0, 0, 0))))
            f.write(m.positions.astype("<f4").tobytes())
            if m.normals is not None:
                f.write(m.normals.astype("<f4").tobytes())
            f.write(m.indices.astype("<u4").tobytes())


def run(program, *args):
    # (a process of its own; the sanitizers' runtime is linked into the program statically)
    p = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    return {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", p.stdout)}


@pytest.mark.parametrize("build", list(BUILDS))
def test_closed_form_equals_drawing(programs, build):
    out = run(programs[build], "closed-form")
    assert out["failures"] == 0 and out["cases"] == 3 * 12 * 5 * 8


def cornell(integrator):
    return scenes.cornell_box(24, 20, 1, integrator, sphere_subdiv=1)


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_lock_step_on_the_cornell_box(programs, tmp_path, integrator):
    write_scene(tmp_path / "scene", cornell(integrator))
    out = run(programs["plain"], "walk", tmp_path / "scene", 6)
    assert out["failures"] == 0 and out["paths"] == 24 * 20 * 6 and out["stored"] > out["paths"] and out["max_depth"] >= 4
    if integrator == "path_mats":
        assert out["shadow"] == 0
    else:
        assert 0 < out["lit"] < out["shadow"] and out["forced"] == out["shadow"]
    # streams next to 2^31 (spp_begin): the same checks
    out = run(programs["plain"], "walk", tmp_path / "scene", 2, 2 ** 31 - 2)
    assert out["failures"] == 0 and out["stored"] > 0


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_lock_step_without_an_emitter(programs, tmp_path, integrator):
    sc = no_emitter(integrator)
    sc.camera.width, sc.camera.height = 24, 20
    write_scene(tmp_path / "scene", sc)
    out = run(programs["plain"], "walk", tmp_path / "scene", 4)
    # sample_direct draws its four numbers and asks for no shadow ray
    assert out["failures"] == 0 and out["shadow"] == 0 and out["stored"] > out["paths"]


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_lock_step_past_the_table(programs, tmp_path, integrator):
    sc = white_box(integrator)
    sc.camera.width, sc.camera.height = 12, 10
    write_scene(tmp_path / "scene", sc)
    out = run(programs["plain"], "walk", tmp_path / "scene", 2)
    assert out["failures"] == 0 and out["past_table"] > 0 and out["max_depth"] > 100, out


def test_lock_step_under_the_sanitizers(programs, tmp_path):
    write_scene(tmp_path / "cornell", cornell("path_mis"))
    out = run(programs["sanitized"], "walk", tmp_path / "cornell", 2)
    assert out["failures"] == 0 and out["stored"] > 0 and out["forced"] > 0
    sc = white_box("path_ems")
    sc.camera.width, sc.camera.height = 6, 5
    write_scene(tmp_path / "box", sc)
    out = run(programs["sanitized"], "walk", tmp_path / "box", 1)
    assert out["failures"] == 0 and out["past_table"] > 0
