"""The film kernels (nori_amd/csrc/device/film.hip) where the rest of the suite does not reach: more samples per pixel than
one staging chunk of the reference-order kernel, filters of 11 to 17 taps, frames smaller than the filter's border,
samples the isValid() guard rejects, the film in several launches / batches / tile shares.

Two checks, on the whole bordered RGBW frame:
  * film_order = reference: every bit equals the single-threaded oracle's frame;
  * the fast film (film_gather + film_resolve, what the benchmark runs): every pixel and channel within the first-order
    summation bound of the oracle's binary64 film -- tests/test_gpu_parity.py: assert_within_summation_bound.
The oracle's frame and binary64 film of a configuration are computed once (tests/film_cases.py) and never written to."""
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from nori_amd.scene import RFilter
from tests import film_cases
from tests.film_cases import ROWS, FilmReference, row_reference
from tests.test_gpu_parity import assert_built_where_asked, assert_within_summation_bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINES = ("megakernel", "wavefront")
ENGINE_ID = {"megakernel": 0, "wavefront": 1}


@pytest.fixture(scope="module")
def row_renderer(renderer_factory):
    """One renderer per (row, builder), shared by the tests of this file (options are set by each test)."""
    made = {}

    def get(name, builder=0):
        if (name, builder) not in made:
            made[name, builder] = renderer_factory(film_cases.row_scene(name), builder=builder)
            assert_built_where_asked(made[name, builder], builder)
        return made[name, builder]

    return get


def render(r, engine, film_order, what="", **kw):
    r.set_option("engine", engine)
    r.set_option("film_order", film_order)
    t0 = time.perf_counter()
    F, st = r.render_host(**kw)
    print(f"[film time] {what} {engine} {film_order}: {1e3 * (time.perf_counter() - t0):.1f} ms wall, {st['kernel_ms']:.2f} ms on the device")
    assert st["engine"] == ENGINE_ID[engine]
    return F, st


def assert_same_bits(ref: FilmReference, F, st, what):
    for k in ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid"):
        assert st[k] == ref.stats[k], (what, k, st[k], ref.stats[k])
    A = ref.frame
    assert F.shape == A.shape, what
    diff = F.view(np.uint32) != A.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {A.size} floats differ, max {np.abs(A - F).max():.3e}, first at {tuple(np.argwhere(diff)[0])}"


# ------------------------------------------------------------------------------------------------ reference order
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", list(ROWS))
def test_reference_order_has_the_oracles_bits(row_renderer, name, engine):
    ref = row_reference(name)
    for builder in (0, 2) if name[0] in "bf" else (0,):
        F, st = render(row_renderer(name, builder), engine, "reference", f"{name} builder {builder}")
        assert_same_bits(ref, F, st, f"{name} {engine} builder {builder}")


@pytest.mark.parametrize("engine", ENGINES)
def test_reference_order_with_chunks_of_4_samples(row_renderer, monkeypatch, engine):
    """NORI_HIP_FILM_REF_CHUNK (read per call): 70 samples per pixel as 17 chunks of 4 and one of 2 -- the same bits."""
    name = "b-two-chunks-and-6"
    monkeypatch.setenv("NORI_HIP_FILM_REF_CHUNK", "4")
    F, st = render(row_renderer(name), engine, "reference", name + " chunk 4")
    assert_same_bits(row_reference(name), F, st, f"{name} {engine} chunk 4")


_UNSTAGED_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from nori_amd.render import Renderer
from tests import film_cases
assert os.environ.get("NORI_HIP_FILM_REF_UNSTAGED")
stats = {}
for name in sys.argv[3:]:
    r = Renderer(0).upload(film_cases.row_scene(name))
    r.set_option("film_order", "reference")
    for engine in ("megakernel", "wavefront"):
        r.set_option("engine", engine)
        F, st = r.render_host()
        np.save(os.path.join(sys.argv[2], name + "-" + engine + ".npy"), F)
        stats[name + "-" + engine] = {k: int(st[k]) for k in ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid", "engine")}
    r.close()
json.dump(stats, open(os.path.join(sys.argv[2], "stats.json"), "w"))
"""


def test_reference_order_unstaged_kernel_in_a_fresh_process(tmp_path):
    """NORI_HIP_FILM_REF_UNSTAGED (read once per process) selects film_block_reference_kernel, the first implementation:
    one thread per output pixel.  Same bits, at more than one chunk's worth of samples and at 17 taps."""
    names = ["b-two-chunks-and-6", "f-border8"]
    env = dict(os.environ, NORI_HIP_FILM_REF_UNSTAGED="1")
    p = subprocess.run([sys.executable, "-c", _UNSTAGED_CHILD, ROOT, str(tmp_path)] + names, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    stats = json.load(open(tmp_path / "stats.json"))
    for name in names:
        for engine in ENGINES:
            st = stats[f"{name}-{engine}"]
            assert st["engine"] == ENGINE_ID[engine]
            assert_same_bits(row_reference(name), np.load(tmp_path / f"{name}-{engine}.npy"), st, f"{name} {engine} unstaged")


# ------------------------------------------------------------------------------------------------------ fast film
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", list(ROWS))
def test_fast_film_is_within_the_summation_bound(row_renderer, name, engine):
    ref = row_reference(name)
    F, st = render(row_renderer(name), engine, "fast", name)
    for k in ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid"):
        assert st[k] == ref.stats[k], (k, st[k], ref.stats[k])
    assert_within_summation_bound(F, *ref.film, f"fast film, {name} {engine}")
    if ROWS[name][2].type == "box":      # sums of integers are exact in any order
        assert np.array_equal(F[..., 3], ref.frame[..., 3]) and (F[..., 3] == ROWS[name][3]).all()


SIZES = [(32, 32), (45, 37)]      # one block of 2 x 2 tiles; 2 x 2 blocks of 3 x 3 tiles, clipped


@functools.lru_cache(maxsize=None)
def plain_reference(w, h, spp, integrator="path_mis", radiance=None, tile_mod=1, tile_rem=0) -> FilmReference:
    """The Cornell box under the default filter (gaussian, radius 2)."""
    return FilmReference(film_cases.cornell(w, h, spp, RFilter("gaussian"), integrator, radiance), tile_mod=tile_mod, tile_rem=tile_rem)


def n_tiles(w, h):
    return ((w + 15) // 16) * ((h + 15) // 16)


@pytest.mark.parametrize("w,h", SIZES)
def test_megakernel_film_in_six_launches(renderer_factory, monkeypatch, w, h):
    """NORI_HIP_FILM_SAMPLES caps the sample store: 40 samples per pixel go through it 7 at a time (the last launch 5), the
    tile accumulators carried from launch to launch."""
    import torch
    ref = plain_reference(w, h, 40)
    monkeypatch.setenv("NORI_HIP_FILM_SAMPLES", str(n_tiles(w, h) * 256 * 7))
    r = renderer_factory(ref.scene)
    r.set_option("engine", "megakernel"); r.set_option("film_order", "fast")
    frame = torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    st = r.render_into(frame, time_kernels=True)
    assert st["engine"] == 0 and st["n_trace_launches"] == 6
    for k in ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid"):
        assert st[k] == ref.stats[k], (k, st[k], ref.stats[k])
    assert_within_summation_bound(frame.cpu().numpy(), *ref.film, f"fast film, megakernel in 6 launches, {w} x {h}")


@pytest.mark.parametrize("w,h,spp,samples", [(32, 32, 40, 4 * 256 * 7), (45, 37, 40, 9 * 256 * 7), (45, 37, 3, 1024)])
def test_wavefront_film_in_several_batches(renderer_factory, w, h, spp, samples):
    """wavefront_samples bounds a batch: 40 samples per pixel in six batches of whole frames (7 + ... + 5 samples per pixel), and 3
    samples per pixel in nine batches of 4, 4 and 1 tiles.  With two or more batches the tail of one runs beside the next and
    the sample store alternates between its two halves (stats: tail_cus > 0)."""
    ref = plain_reference(w, h, spp)
    r = renderer_factory(ref.scene)
    r.set_option("wavefront_samples", samples)
    F, st = render(r, "wavefront", "fast", f"{w} x {h} x {spp} in batches of {samples}")
    assert st["tail_cus"] > 0
    for k in ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid"):
        assert st[k] == ref.stats[k], (k, st[k], ref.stats[k])
    assert_within_summation_bound(F, *ref.film, f"fast film, wavefront in batches of {samples} samples, {w} x {h} x {spp}")


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("w,h", SIZES)
def test_tile_shares_are_within_the_bound_of_their_own_film(renderer_factory, w, h, engine):
    """tile_mod = 3: each share of the tiles against the oracle's binary64 film of the same share."""
    r = None
    for rem in range(3):
        ref = plain_reference(w, h, 40, tile_mod=3, tile_rem=rem)
        r = r or renderer_factory(ref.scene)
        F, st = render(r, engine, "fast", f"{w} x {h} tiles {rem} mod 3", tile_mod=3, tile_rem=rem)
        for k in ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid"):
            assert st[k] == ref.stats[k], (rem, k, st[k], ref.stats[k])
        assert 0 < st["n_camera_samples"] < w * h * 40
        assert_within_summation_bound(F, *ref.film, f"fast film, {engine}, tiles {rem} mod 3, {w} x {h}")


# ----------------------------------------------------------------------------------------------- rejected samples
NEGATIVE_LIGHT = (20.0, -1.0, 20.0)      # finite, inside the domain the exact-division sequences are verified on


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("integrator", ["path_mis", "path_mats"])
def test_samples_the_guard_rejects(renderer_factory, integrator, engine):
    """A light with a negative channel: ImageBlock::put's isValid() guard (src/block.cpp:63-67) drops every sample that saw it in
    that channel -- most of path_mis', a few per cent of path_mats'.  The kernels count them and give them weight 0 and
    radiance 0, which must leave every accumulator's bits alone."""
    ref = plain_reference(45, 37, 40, integrator, NEGATIVE_LIGHT)
    print(f"[film invalid] {integrator}: {ref.stats['n_invalid']} of {ref.stats['n_camera_samples']} samples rejected by the oracle")
    assert 0 < ref.stats["n_invalid"] < ref.stats["n_camera_samples"]
    r = renderer_factory(ref.scene)
    F, st = render(r, engine, "reference", "negative light " + integrator)
    assert_same_bits(ref, F, st, f"negative light, {integrator} {engine}")
    G, sg = render(r, engine, "fast", "negative light " + integrator)
    for k in ("n_camera_samples", "n_closest_rays", "n_shadow_rays", "n_invalid"):
        assert sg[k] == ref.stats[k], (k, sg[k], ref.stats[k])
    assert_within_summation_bound(G, *ref.film, f"fast film, negative light, {integrator} {engine}")
    assert (F >= 0).all() and (G >= 0).all()


@pytest.mark.parametrize("engine", ENGINES)
def test_rejected_samples_are_counted_once_over_block_row_shares(renderer_factory, engine):
    """render_block_rows_into with 1, 2 and 3 shares of the frame's 2 block rows (the third share is empty): the shares' counts
    add up to the frame's, the resolved frame has the bits of the one-share frame -- the oracle's."""
    import torch
    from nori_amd import dist as ndist
    ref = plain_reference(45, 37, 40, "path_mis", NEGATIVE_LIGHT)
    r = renderer_factory(ref.scene)
    r.set_option("engine", engine); r.set_option("film_order", "reference")
    assert r.block_rows() == 2
    for world in (1, 2, 3):
        total, invalid, cameras = torch.zeros(r.block_acc_floats(), dtype=torch.float32, device="cuda:0"), 0, 0
        for rank in reversed(range(world)):
            acc = torch.zeros_like(total)
            st = r.render_block_rows_into(acc, *ndist.block_rows(rank, world, r.block_rows()))
            invalid += st["n_invalid"]; cameras += st["n_camera_samples"]
            total += acc
        frame = torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
        r.resolve_blocks(total, frame)
        assert invalid == ref.stats["n_invalid"] and cameras == ref.stats["n_camera_samples"], (world, invalid, cameras)
        assert np.array_equal(frame.cpu().numpy().view(np.uint32), ref.frame.view(np.uint32)), world
