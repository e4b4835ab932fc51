"""nori_hip_li and both engines' frames against tests/path_ref.py, byte for byte, on the DRAWN rounds of tests/path_fuzz.py: where
tests/test_gpu_paths.py pins the general kernels (the kEnvLit / kMedium variants of li_kernel, render_kernel, wf_shade and
wf_finish) on five hand-made scenes, these rounds draw the scene -- texcoords that differ at every corner (hit_uv inside shading),
a fog or a sky or neither with microfacet, mirror and glass at the ends of their parameters, a sky as the only light, lights that
reflect or face away, a thin lens, a camera inside glass, frames of ragged width, all three tree builders, the sample index up to
2^32 - 1, and the wavefront pool, batch and finish knobs.

One test per committed seed, and one per committed LIT seed: a round of its own seed with drawn delta lights, held to
tests/delta_lights_ref.py in the same way.  tests/test_path_fuzz_cpu.py shows without a GPU what these seeds reach and that a wrong branch
changes their bytes.  Every comparison is equality of bytes: no tolerance, no exempted path; a round's line of differing paths
reads 0 for every part."""
from __future__ import annotations

import pytest

from tests import path_fuzz as pf

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", pf.SEEDS)
def test_round_equals_the_reference_bit_for_bit(renderer_factory, seed):
    made = []

    def make(scene, **kw):
        made.append(renderer_factory(scene, **kw))
        return made[-1]
    try:
        pf.one_round(seed, make)
    finally:
        for r in made:      # (now, not when the file is done: a context per round is all that need be alive)
            r.close()


@pytest.mark.parametrize("seed", pf.LIT_SEEDS)
def test_lit_round_equals_the_reference_bit_for_bit(renderer_factory, seed):
    """the same round with drawn delta lights (path_fuzz.lit_scene_of) under path_ems or path_mis, against tests/delta_lights_ref.py:
    the kDeltaLit variants, alone, with kEnvLit and with kMedium -- up to 4096 lights in a wall's plane, a hair off it on either
    side, at a mesh vertex, inside a body, at the eye and behind the ceiling, black ones, hard-edged and hair-thin cones"""
    made = []

    def make(scene, **kw):
        made.append(renderer_factory(scene, **kw))
        return made[-1]
    try:
        pf.one_round(seed, make, lit=True)
    finally:
        for r in made:
            r.close()
