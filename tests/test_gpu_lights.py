"""Emitter sampling on the device, bit for bit: many lights, uneven CDFs, the limits of the shade tables.

tests/light_cases.py has the scenes -- five regimes, one per way the kernels read the small tables (global memory, DevScene
pointers redirected into LDS, LDS instructions) and per shape of the tables' last 16-byte quad -- and the references:
  * radiance: Renderer.li against Oracle.li, path for path (li_kernel: the global reader);
  * frames in film_order = reference against a single-threaded oracle render, every bit of the RGBW frame: megakernel
    (render_kernel: redirected pointers), wavefront as shipped (a small frame's vertices after the first are shaded by wf_finish:
    redirected pointers) and wavefront with NORI_HIP_WF_FINISH_PATHS=256 (wf_shade shades until at most 256 paths live: LdsTables
    where the tables fit, global memory where not);
  * the pick itself (nori_hip_debug_emitter_sample: emitter_pick + emitter_point through each of the three readers) against
    light_cases.pick_reference -- numpy, float32 operation by operation, std::lower_bound -- on uniform samples and on the edges
    no render reaches: xiT on a CDF entry and beside it, repeated entries, 0 and 1, xiE on the emitter boundaries;
  * the tables as uploaded (nori_hip_debug_emitter_tables): counts, the CDF's ends and monotonicity, its rounding error.
"""
import os
import time

import numpy as np
import pytest

from nori_amd import NoriError
from tests import light_cases as lc
from tests import scenes
from tests.backends import Oracle
from tests.test_gpu_parity import assert_built_where_asked

pytestmark = pytest.mark.gpu

N_PATHS = 20000
FRAME = dict(width=48, height=32, spp=4)      # 6144 camera samples; the default filter is the Gaussian (border 2)
CASES = [(r, "path_mis") for r in lc.REGIMES] + [(r, i) for r in ("R2", "R3") for i in ("path_ems", "whitted")]
READERS = ("global", "redirected", "lds")

_scenes, _oracle_frames, _renderers = {}, {}, {}


def _with_env(env, fn):
    """As tests/test_gpu_wavefront.py's: the variables are set around the call only."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _scene(name, integ="path_mis"):
    if (name, integ) not in _scenes:
        _scenes[name, integ] = lc.regime(name, integ, **FRAME)
    return _scenes[name, integ]


def _renderer(renderer_factory, name, integ="path_mis", builder=0):
    """One context per (regime, integrator, builder) for the whole file."""
    key = (name, integ, builder)
    if key not in _renderers:
        _renderers[key] = renderer_factory(_scene(name, integ), builder=builder)
        assert_built_where_asked(_renderers[key], builder)
    return _renderers[key]


def _oracle_frame(name, integ):
    """The single-threaded oracle's frame, computed once and shared (read-only)."""
    if (name, integ) not in _oracle_frames:
        A, st = Oracle(_scene(name, integ), use_bvh=True).render_host(threads=1)
        A.setflags(write=False)
        _oracle_frames[name, integ] = (A, st)
    return _oracle_frames[name, integ]


@pytest.mark.parametrize("name,integ", CASES)
def test_li_equals_the_oracle_path_for_path(renderer_factory, name, integ):
    """Renderer.li == Oracle.li on 20000 camera rays with random seeds and sequences, every bit of every path's radiance."""
    sc = _scene(name, integ)
    r, o = _renderer(renderer_factory, name, integ), Oracle(sc, use_bvh=True)
    rays, ss, sq = lc.li_inputs(o, sc, N_PATHS, seed=3)
    a = o.li(rays, ss, sq)
    t0 = time.perf_counter()
    b = r.li(rays, ss, sq)
    differ = int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum())
    print(f"[lights] li {name} {integ}: {differ} of {N_PATHS} paths differ ({1e3 * (time.perf_counter() - t0):.0f} ms on the device)")
    assert np.isfinite(b).all()
    assert differ == 0


FRAME_CASES = [(n, i, 0) for n, i in CASES] + [(n, i, 2) for n, i in CASES if n in ("R2", "R3")]


@pytest.mark.parametrize("name,integ,builder", FRAME_CASES)
def test_reference_order_frames_equal_the_oracle(renderer_factory, name, integ, builder):
    """film_order = reference, 48 x 32 at 4 spp (the height is one 32-pixel block, the width one and a half; two 16-pixel tile rows):
    the whole RGBW frame and both ray counts equal the single-threaded oracle's, for (a) the megakernel, (b) the wavefront engine
    as shipped and (c) the wavefront engine with NORI_HIP_WF_FINISH_PATHS=256.

    Which kernel shades what in (b) and (c).  The launch count (stats["n_workgroups"] of a wavefront render) does NOT tell them
    apart here -- measured 15 and 15 (whitted: 14 and 14) -- because of what wavefront_render guarantees: while a batch may still
    start camera samples the path count is read back only every sync_every = 6 iterations, so wf_shade runs six
    passes over the paths of such a frame before wf_finish can be chosen at all, as shipped as well as under the knob (measured
    on R1 and R2: 121 and 123 of 6144 paths live at that first readback, fewer than 256; whitted: none).  Six wf_extend and six
    wf_shade launches are 12 of the launches counted, and that is asserted: wf_shade's table reader -- LdsTables where the
    tables fit, global memory where not -- does nearly all of a frame's emitter sampling in (b) and (c), wf_finish (redirected
    pointers) the tail of the longest paths.  (c) is kept: the knob makes wf_shade go on wherever more than 256 paths live at a
    readback, so it can only take as many launches as (b) or more."""
    A, sa = _oracle_frame(name, integ)
    r = _renderer(renderer_factory, name, integ, builder)
    r.set_option("film_order", "reference")
    failures, launches = [], {}
    for label, engine, env in (("a megakernel", "megakernel", {}), ("b wavefront", "wavefront", {}),
                               ("c wavefront wf_shade", "wavefront", {"NORI_HIP_WF_FINISH_PATHS": 256})):
        r.set_option("engine", engine)
        t0 = time.perf_counter()
        B, sb = _with_env(env, lambda: r.render_host())
        ms = 1e3 * (time.perf_counter() - t0)
        differ = int((A.view(np.uint32) != B.view(np.uint32)).sum())
        rays_equal = sa["n_closest_rays"] == sb["n_closest_rays"] and sa["n_shadow_rays"] == sb["n_shadow_rays"]
        print(f"[lights] frame {name} {integ} builder {builder} ({label}): {differ} of {A.size} floats differ, ray counts equal: {rays_equal}, "
              f"{sb['n_workgroups']} launches / workgroups, {ms:.0f} ms")
        assert sb["engine"] == (0 if engine == "megakernel" else 1)
        launches[label[0]] = sb["n_workgroups"]
        if differ or not rays_equal or not np.array_equal(A, B):
            failures.append((label, differ, rays_equal))
    r.set_option("film_order", "fast")
    assert not failures, failures
    assert launches["c"] >= launches["b"] >= 12, launches


@pytest.mark.parametrize("name", list(lc.REGIMES))
def test_table_counts_and_the_lds_reader_is_refused_where_the_tables_do_not_fit(renderer_factory, name):
    sc = _scene(name)
    r = _renderer(renderer_factory, name)
    tb = r.emitter_tables()
    counts = (tb["n_meshes"], tb["n_emitters"], tb["n_cdf"])
    assert counts == lc.table_counts(sc) == lc.REGIMES[name][1]
    em = [i for i, m in enumerate(sc.meshes) if m.radiance is not None]
    assert list(tb["emitters"]) == em
    assert [int(tb["n_triangles"][i]) for i in range(len(sc.meshes))] == [m.indices.shape[0] for m in sc.meshes]
    assert int(sum(tb["n_triangles"][i] + 1 for i in em)) == tb["n_cdf"]
    x = np.full((5, 4), 0.5, np.float32)
    if lc.fits(counts):
        r.emitter_sample(x, "lds")
    else:
        with pytest.raises(NoriError, match="UNSUPPORTED"):
            r.emitter_sample(x, "lds")
    r.emitter_sample(x, "global"); r.emitter_sample(x, "redirected")      # never refused


def test_emitter_sample_refuses_loudly(renderer_factory):
    """An unknown reader and a scene without emitters are errors with a message, not results."""
    r = _renderer(renderer_factory, "R1")
    x = np.full((3, 4), 0.25, np.float32)
    for reader in (-1, 3, 7):
        with pytest.raises(NoriError, match="unknown reader"):
            r.emitter_sample(x, reader)
    dark = renderer_factory(scenes.soup_scene(40))
    for reader in READERS:
        with pytest.raises(NoriError, match="no emitters"):
            dark.emitter_sample(x, reader)
    assert dark.emitter_tables()["n_emitters"] == 0
    m, t, p = r.emitter_sample(np.zeros((0, 4), np.float32))
    assert m.size == 0 and p.shape == (0, 3)


@pytest.mark.parametrize("name", list(lc.REGIMES))
def test_cdf_as_uploaded(renderer_factory, name):
    """Every emitter's CDF in device memory starts at 0.0, ends at exactly 1.0 and never decreases, and entry k is within
    (k + 2) 2^-24 relative of the cumulative area fraction computed in binary64 from the float32 triangle areas: k float32
    additions and the scaling (light_cases.cdf_check; the worst ratio of the error to the bound is printed and must be <= 1).

    The fraction is of the total S the table is normalised by (the float32 sum, tied to the device's table through inv_area =
    1 / S): that is the reference the bound follows for, S being the given normaliser -- k - 1 roundings in entry k's partial
    sum, one in 1 / S, one in the product.  Measured worst ratios, R1 .. R5: 0.283, 0.335, 0.335, 0.260, 0.325.  Against the
    fraction of the BINARY64 total, (k + 2) 2^-24 does not hold and cannot: S itself has n - 1 float32 additions behind it, which
    no entry's k counts (k = 1 of R5's 20-triangle light is off by 3.015 * 2^-24, S by 2.04 * 2^-24; worst ratios 0.240, 0.962,
    0.962, 0.465, 1.005).  That comparison is asserted with the bound that counts them, (k + n) 2^-24: worst ratios 0.064, 0.320,
    0.320, 0.465, 0.176.  The tables are DiscretePDF's arithmetic (append in float, normalise by the float total:
    include/nori/dpdf.h) and the oracle's bits."""
    sc = _scene(name)
    tb = _renderer(renderer_factory, name).emitter_tables()
    worst_table, worst_exact = lc.cdf_check(sc, tb)
    print(f"[lights] cdf {name}: worst error / ((k + 2) 2^-24) against the table's total = {worst_table:.3f}; "
          f"worst error / ((k + n) 2^-24) against the binary64 total = {worst_exact:.3f}")
    assert worst_table <= 1.0
    assert worst_exact <= 1.0


@pytest.mark.parametrize("name", list(lc.REGIMES))
def test_pick_equals_the_numpy_statement_through_every_reader(renderer_factory, name):
    """Mesh, triangle and every bit of the point, for each reader the regime allows, against light_cases.pick_reference applied to
    the device's own CDF, on light_cases.edge_samples (100000 uniform samples plus the edges); and the readers agree with each
    other.  The samples that sit exactly on a CDF entry and those that pick a zero-area triangle are counted: neither edge may
    drop out."""
    sc = _scene(name)
    r = _renderer(renderer_factory, name)
    tb = r.emitter_tables()
    x = lc.edge_samples(tb)
    assert x.shape[0] >= 100000 and x.min() == 0.0 and x.max() == 1.0 and np.isfinite(x).all()
    rm, rt, rp = lc.pick_reference(sc, tb, x)
    on_entry, zero_area = lc.edge_counts(tb, x, rm, rt)
    print(f"[lights] pick {name}: {x.shape[0]} samples, {on_entry} on a CDF entry, {zero_area} on a zero-area triangle")
    assert on_entry > 0 and zero_area > 0
    readers = [rd for rd in READERS if rd != "lds" or lc.fits(lc.table_counts(sc))]
    assert len(readers) == (3 if lc.REGIMES[name][2] else 2)
    got, failures = {}, []
    for rd in readers:
        t0 = time.perf_counter()
        m, t, p = r.emitter_sample(x, rd)
        ms = 1e3 * (time.perf_counter() - t0)
        got[rd] = (m, t, p)
        bad = (m != rm) | (t != rt) | (p.view(np.uint32) != rp.view(np.uint32)).any(axis=1)
        edge_bad = int(bad[100000:].sum())
        print(f"[lights] pick {name} reader {rd}: {int(bad.sum())} of {x.shape[0]} samples differ ({edge_bad} of them edge samples), {ms:.0f} ms")
        if bad.any():
            failures.append((rd, int(bad.sum()), edge_bad))
    assert not failures, failures
    for rd in readers[1:]:
        for u, v in zip(got[readers[0]], got[rd]):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), rd
