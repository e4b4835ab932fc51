"""film_gather_strips_kernel (nori_amd/csrc/device/film.hip: the fast film's gather for border 1 and 2, one thread per vertical
strip of outputs) against film_gather_kernel, the gather it replaces there: the same terms in the same order, so EVERY BIT of
the bordered RGBW frame, the count of rejected samples and the ray counts must be equal.

NORI_HIP_FILM_GATHER=rounds (read once per process) forces film_gather_kernel for every border, so the old frames come from
one child process that renders every case of this file with the switch set; this process renders the same cases with the
switch unset.  Both go through render_cases() below."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nori_amd.scene import RFilter
from tests import film_cases
from tests.test_gpu_film import ENGINE_ID, ENGINES, NEGATIVE_LIGHT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_KEYS = ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid", "engine")

# rows of film_cases.ROWS                                what they reach in the gather
ROW_NAMES = ["a-one-past-a-chunk", "b-two-chunks-and-6",      # border 2, 45 x 37: clipped edge tiles
             "c-tent-one-chunk",                              # border 1, 33 x 17
             "h-one-pixel",                                   # one live lane per tile
             "k-1spp", "k-3spp",                              # fewer samples than n_parts: empty parts
             "f-border8", "j-box"]                            # borders that keep film_gather_kernel
BATCH_SAMPLES = 9 * 256 * 7      # 40 samples per pixel of 9 tiles in six batches (tests/test_gpu_film.py: test_wavefront_film_in_several_batches)


def plain(integrator="path_mis", radiance=None):
    return film_cases.cornell(45, 37, 40, RFilter("gaussian"), integrator, radiance)


def case_groups():
    """[(scene, [(key, engine, options, render_host's keywords)])]: one upload per scene."""
    groups = [(film_cases.row_scene(name), [(f"row-{name}-{engine}", engine, {}, {}) for engine in ENGINES]) for name in ROW_NAMES]
    groups.append((plain(), [("batches", "wavefront", {"wavefront_samples": BATCH_SAMPLES}, {})]))
    groups.append((plain(), [(f"share-{rem}", "wavefront", {}, {"tile_mod": 3, "tile_rem": rem}) for rem in range(3)]))
    for integrator in ("path_mis", "path_mats"):
        groups.append((plain(integrator, NEGATIVE_LIGHT), [(f"rejected-{integrator}-{engine}", engine, {}, {}) for engine in ENGINES]))
    return groups


def render_cases(out_dir):
    """Every case with film_order = fast: <key>.npy and stats.json in out_dir."""
    from nori_amd.render import Renderer
    stats = {}
    for scene, cases in case_groups():
        r = Renderer(0).upload(scene)
        r.set_option("film_order", "fast")
        for key, engine, options, kw in cases:
            r.set_option("engine", engine)
            for k, v in options.items():
                r.set_option(k, v)
            F, st = r.render_host(**kw)
            np.save(os.path.join(out_dir, key + ".npy"), F)
            stats[key] = {k: int(st[k]) for k in STAT_KEYS + ("tail_cus",)}
        r.close()
    with open(os.path.join(out_dir, "stats.json"), "w") as f:
        json.dump(stats, f)


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
assert os.environ.get("NORI_HIP_FILM_GATHER") == "rounds"
from tests.test_gpu_film_gather_strips import render_cases
render_cases(sys.argv[2])
"""


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """key -> (old frame, old stats, new frame, new stats)"""
    assert os.environ.get("NORI_HIP_FILM_GATHER") != "rounds", "this process must run the gather the library picks"
    old_dir, new_dir = tmp_path_factory.mktemp("gather_rounds"), tmp_path_factory.mktemp("gather_strips")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(old_dir)], env=dict(os.environ, NORI_HIP_FILM_GATHER="rounds"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    render_cases(str(new_dir))
    old, new = json.load(open(old_dir / "stats.json")), json.load(open(new_dir / "stats.json"))
    assert set(old) == set(new)
    return {k: (np.load(old_dir / (k + ".npy")), old[k], np.load(new_dir / (k + ".npy")), new[k]) for k in old}


def assert_equal_bits(frames, key, engine):
    A, sa, B, sb = frames[key]
    assert sa["engine"] == sb["engine"] == ENGINE_ID[engine], (key, sa, sb)
    for k in STAT_KEYS:
        assert sa[k] == sb[k], (key, k, sa[k], sb[k])
    assert A.dtype == B.dtype == np.float32 and A.shape == B.shape and A.shape[2] == 4, key
    assert sb["n_camera_samples"] > 0 and (B[..., 3] > 0).any(), key
    diff = A.view(np.uint32) != B.view(np.uint32)
    assert not diff.any(), f"{key}: {int(diff.sum())} of {A.size} floats differ, max {np.abs(A - B).max():.3e}, first at {tuple(np.argwhere(diff)[0])}"
    return sb


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ROW_NAMES)
def test_same_bits_as_the_rounds_kernel(frames, name, engine):
    st = assert_equal_bits(frames, f"row-{name}-{engine}", engine)
    w, h, _, spp = film_cases.ROWS[name]
    assert st["n_camera_samples"] == w * h * spp


def test_same_bits_in_several_batches(frames):
    """wavefront_samples bounds a batch: the film is gathered six times, the tile accumulators carried from batch to batch."""
    st = assert_equal_bits(frames, "batches", "wavefront")
    assert st["tail_cus"] > 0 and st["n_camera_samples"] == 45 * 37 * 40


@pytest.mark.parametrize("rem", range(3))
def test_same_bits_of_a_tile_share(frames, rem):
    st = assert_equal_bits(frames, f"share-{rem}", "wavefront")
    assert 0 < st["n_camera_samples"] < 45 * 37 * 40


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("integrator", ["path_mis", "path_mats"])
def test_same_bits_with_rejected_samples(frames, integrator, engine):
    """A light with a negative channel (tests/test_gpu_film.py: test_samples_the_guard_rejects): rejected samples are staged with
    weight 0 and radiance 0 by both kernels."""
    st = assert_equal_bits(frames, f"rejected-{integrator}-{engine}", engine)
    assert 0 < st["n_invalid"] < st["n_camera_samples"]
