"""Albedo textures without a GPU: the descriptor and its defaults, the fixtures' digests, .npz round trips, the load-time
checks of prepare_scene (through the CPU emulation, which shares that code with the library), and the register budget of the
kernels compiled for textured scenes."""
from __future__ import annotations

import glob
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi as capi
from nori_amd.scene import Bsdf, Scene, Texture
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_zero_initialised_descriptors_carry_no_texture():
    assert capi.MeshDesc().albedo_texture == 0
    s = capi.SceneDesc()
    assert s.n_textures == 0 and not s.textures
    assert capi.HIP_ABI_VERSION == 8
    desc, keep = scenes.cornell_box(8, 8, 1).c_desc()
    assert desc.n_textures == 0 and not desc.textures
    assert all(desc.meshes[i].albedo_texture == 0 for i in range(desc.n_meshes))


def test_c_desc_marshals_textures_one_based():
    sc = scenes.cornell_box(8, 8, 1)
    img = np.arange(2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3)
    sc.textures = [Texture("checkerboard", color0=(1, 0, 0), color1=(0, 0, 1), uscale=3.0), Texture("image", img, "nearest", "clamp")]
    sc.meshes[2].albedo_texture = 1
    desc, keep = sc.c_desc()
    assert desc.n_textures == 2
    t = desc.textures[1]
    assert (t.type, t.width, t.height, t.filter, t.wrap) == (0, 3, 2, 0, 1)
    assert np.array_equal(np.ctypeslib.as_array(t.texels, (2 * 3 * 3,)), img.reshape(-1))
    assert desc.textures[0].type == 1 and desc.textures[0].uscale == 3.0 and list(desc.textures[0].color1) == [0, 0, 1]
    assert [desc.meshes[i].albedo_texture for i in range(desc.n_meshes)] == [0, 0, 2, 0, 0, 0, 0, 0]


def _old_digest(sc):
    """geometry_digest as it was before scenes had textures"""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(sc.camera.to_world, dtype=np.float32).tobytes())
    for m in sc.meshes:
        for a in (m.positions, m.indices, m.normals, m.texcoords):
            h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_geometry_digest_of_the_fixtures_is_unchanged():
    paths = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
    n = 0
    for p in paths:
        z = np.load(p)
        if "meta" not in z.files:
            continue
        sc = Scene.load_npz(p)       # (variant fixtures assert their stored digest of the base's arrays on load)
        assert not sc.textures
        assert sc.geometry_digest() == _old_digest(sc), p
        n += 1
    assert n >= 5


def test_textured_scene_round_trips_through_npz(tmp_path):
    sc = scenes.cornell_box(8, 8, 1)
    rng = np.random.default_rng(1)
    sc.textures = [Texture("image", rng.uniform(0, 1, (4, 5, 3)), "nearest", "clamp", 2.0, 3.0, 0.5, -0.5),
                   Texture("checkerboard", color0=(0.1, 0.2, 0.3), color1=(0.4, 0.5, 0.6), uscale=8.0)]
    sc.meshes[0].albedo_texture, sc.meshes[2].albedo_texture = 1, 0
    p = str(tmp_path / "t.npz")
    sc.save_npz(p)
    back = Scene.load_npz(p)
    assert [m.albedo_texture for m in back.meshes] == [m.albedo_texture for m in sc.meshes]
    assert len(back.textures) == 2
    for a, b in zip(sc.textures, back.textures):
        assert a.params() == b.params()
        assert (a.texels is None and b.texels is None) or np.array_equal(a.texels, b.texels)
    assert back.geometry_digest() == sc.geometry_digest() != _old_digest(sc)


def test_load_time_checks_reject_bad_textures():
    """prepare_scene (shared by the library and the CPU emulation) refuses what nori_hip_upload_scene documents; the messages
    are checked on the GPU (tests/test_gpu_textures.py)."""
    from tests.backends import Emu

    def make(mutate):
        sc = scenes.cornell_box(8, 8, 1)
        sc.textures = [Texture("image", np.ones((2, 2, 3), np.float32))]
        sc.meshes[0].albedo_texture = 0
        mutate(sc)
        return sc

    Emu(make(lambda sc: None)).close()
    bad = [lambda sc: setattr(sc.meshes[0], "albedo_texture", 1),
           lambda sc: (setattr(sc.meshes[1], "bsdf", Bsdf("dielectric")), setattr(sc.meshes[1], "albedo_texture", 0)),
           lambda sc: setattr(sc.textures[0], "texels", np.ones((2, 0, 3), np.float32)),
           lambda sc: setattr(sc.textures[0], "texels", np.ones((16385, 1, 3), np.float32)),
           lambda sc: setattr(sc.textures[0], "texels", None)]
    for mutate in bad:
        with pytest.raises(AssertionError, match="create failed"):
            Emu(make(mutate))


@pytest.fixture(scope="module")
def wavefront_kernels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as ge
    from kernel_resources import kernels
    out = tmp_path_factory.mktemp("asm") / "wavefront.s"
    flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    p = subprocess.run([ge.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(ge.DEV, "wavefront.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return {r["demangled"].replace("(anonymous namespace)::", ""): r for r in kernels(str(out))}


def _one(rows, prefix):
    hit = [r for name, r in rows.items() if name.startswith("void " + prefix)]
    assert len(hit) == 1, (prefix, len(hit))
    return hit[0]


def test_textured_shading_kernels_keep_the_budget(wavefront_kernels):
    rows = wavefront_kernels
    textured = 15 | 16      # kAnyBsdf | kTextured (rt_path.h)
    for integ in range(3, 7):
        for mode in (0, 1, 2):
            for lds_tables in ("true", "false"):
                k = _one(rows, f"wf_shade<{integ}, {mode}, {lds_tables}, {textured}>")
                assert k["vgpr"] <= 128 and k["scratch"] == 0, k
                for matset in (1, 7, 15):      # the names the existing guard looks up still name one kernel each
                    _one(rows, f"wf_shade<{integ}, {mode}, {lds_tables}, {matset}>")
        tail, plain = _one(rows, f"wf_finish<{integ}, {textured}>"), _one(rows, f"wf_finish<{integ}, 15>")
        # (wf_finish keeps its LDS stack's spill words in scratch with or without textures)
        assert tail["vgpr"] <= 128 and tail["scratch"] <= plain["scratch"] and tail["lds"] == plain["lds"], (tail, plain)
    # integrators that never ask a BSDF have no textured kernel
    assert not [n for n in rows if n.startswith("void wf_shade<") and n.split(",")[0].endswith(("<0", "<1", "<2")) and f", {textured}>" in n]
    assert len([n for n in rows if n.startswith("void wf_shade<")]) == 90 + 24
