"""tests/light_cases.py on the CPU: the five regimes are what they claim to be, the device headers (compiled for the host,
tests/emu) agree with the oracle on them path for path, the numpy statement of the emitter pick is the device header's, and
the specification itself -- emitter sampling, BSDF sampling and their MIS combination -- estimates one integral."""
import numpy as np
import pytest

from nori_amd.scene import RFilter
from tests import light_cases as lc
from tests.backends import Emu, Oracle

N_PATHS = 20000


def test_regimes_have_the_stated_counts_and_fit_decisions():
    """Each regime's (n_meshes, n_emitters, n_cdf) and fit decision (asserted by light_cases.regime as well), the limits they sit
    at, the shapes of the last 16-byte quad, the emitter counts, the spread of the areas and the zero-area triangles."""
    got = {}
    for name, (_, counts, fit) in lc.REGIMES.items():
        sc = lc.regime(name)
        got[name] = lc.table_counts(sc)
        assert got[name] == counts and lc.fits(got[name]) == fit
        tb = Emu(sc).emitter_tables()      # scene_prep.cpp counts the same
        assert (tb["n_meshes"], tb["n_emitters"], tb["n_cdf"]) == counts
        flat = [m for m in sc.meshes if m.radiance is not None and m.normals is None]
        areas = np.concatenate([lc.mesh_areas_f32(m) for m in flat])
        nz = areas[areas > 0]
        assert np.log10(nz.max() / nz.min()) >= 2.5, name
        zero_lights = [m for m in flat if (lc.mesh_areas_f32(m) == 0).any()]
        assert zero_lights and all(lc.mesh_areas_f32(m)[0] == 0 and m.indices.shape[0] > 2 for m in zero_lights), name
    assert got["R1"][2] % 4 == 3
    assert got["R2"][0] == lc.FIT_MAX_MESHES and got["R2"][2] == lc.FIT_MAX_CDF
    assert got["R3"][0] == lc.FIT_MAX_MESHES and got["R3"][2] == lc.FIT_MAX_CDF + 1
    assert got["R4"][0] == lc.FIT_MAX_MESHES + 1 and got["R4"][2] <= lc.FIT_MAX_CDF
    assert got["R5"][2] % 4 == 1 and got["R5"][1] % 4 == 2
    assert lc.fits((32, 64, 960)) and not lc.fits((33, 1, 2)) and not lc.fits((3, 3, 961)) and not lc.fits((32, 65, 100))
    ne = {c[1] for c in got.values()}
    assert {3, 25} <= ne and ne & {2, 4}
    r2 = [m.indices.shape[0] for m in lc.regime("R2").meshes if m.radiance is not None]
    assert min(r2) == 1 and max(r2) >= 90
    assert any(m.normals is not None and m.radiance is not None for m in lc.regime("R5").meshes)


def test_light_triangles_are_disjoint():
    """No two light triangles of a regime share a grid cell: every triangle's bounding square lies inside a cell of its own."""
    for name in lc.REGIMES:
        sc = lc.regime(name)
        tris = np.concatenate([m.positions.reshape(-1, 3, 3) for m in sc.meshes if m.radiance is not None and m.normals is None])
        g = max(4, int(np.ceil(np.sqrt(len(tris)))))
        cell = 1.9 / g
        lo = np.floor((tris[:, :, [0, 2]].min(axis=1) + 0.95) / cell + 1e-4).astype(int)
        hi = np.floor((tris[:, :, [0, 2]].max(axis=1) + 0.95) / cell - 1e-4).astype(int)
        assert (hi <= lo).all(), name                                    # inside one cell
        assert len({tuple(c) for c in lo}) == len(tris), name            # and no cell twice
        assert np.all(tris[:, :, 1] == np.float32(lc.LIGHT_Y))


CASES = [(r, "path_mis") for r in lc.REGIMES] + [(r, i) for r in ("R2", "R3") for i in ("path_ems", "whitted")]


@pytest.mark.parametrize("name,integ", CASES)
def test_emu_li_equals_oracle_li(name, integ):
    """The device headers compiled for the host against the oracle, path for path and bit for bit, on N_PATHS camera rays."""
    sc = lc.regime(name, integ)
    o, e = Oracle(sc, use_bvh=True), Emu(sc)
    rays, ss, sq = lc.li_inputs(o, sc, N_PATHS, seed=3)
    a, b = o.li(rays, ss, sq), e.li(rays, ss, sq)
    differ = int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum())
    print(f"[lights cpu] {name} {integ}: {differ} of {N_PATHS} paths differ; mean {a.mean(axis=0)}")
    assert np.isfinite(a).all() and a.max() > 0
    assert differ == 0


@pytest.mark.parametrize("name", list(lc.REGIMES))
def test_numpy_pick_equals_the_device_header(name):
    """light_cases.pick_reference against emitter_pick + emitter_point (tests/emu: emu_emitter_sample) on the edge samples: mesh,
    triangle and every bit of the point.  The samples must reach the edges they are made for."""
    sc = lc.regime(name)
    e = Emu(sc)
    tb = e.emitter_tables()
    x = lc.edge_samples(tb)
    assert x.shape[0] >= 100000 and x.min() == 0.0 and x.max() == 1.0
    m, t, p = e.emitter_sample(x)
    rm, rt, rp = lc.pick_reference(sc, tb, x)
    bad = (m != rm) | (t != rt) | (p.view(np.uint32) != rp.view(np.uint32)).any(axis=1)
    on_entry, zero_area = lc.edge_counts(tb, x, m, t)
    print(f"[lights cpu] {name}: {int(bad.sum())} of {x.shape[0]} picks differ; {on_entry} on a CDF entry, {zero_area} on a zero-area triangle")
    assert int(bad.sum()) == 0
    assert on_entry > 0 and zero_area > 0
    assert set(np.unique(m)) == set(int(i) for i in tb["emitters"])      # every emitter is picked


@pytest.mark.parametrize("name", list(lc.REGIMES))
def test_cdf_of_the_prepared_tables(name):
    """light_cases.cdf_check on the tables scene_prep.cpp makes (the device is handed a copy of them; tests/test_gpu_lights.py
    reads that copy back): ends, monotonicity, and both rounding bounds."""
    sc = lc.regime(name)
    worst_table, worst_exact = lc.cdf_check(sc, Emu(sc).emitter_tables())
    print(f"[lights cpu] cdf {name}: {worst_table:.3f} of (k + 2) 2^-24 against the table's total, {worst_exact:.3f} of (k + n) 2^-24 against the binary64 total")
    assert worst_table <= 1.0 and worst_exact <= 1.0


STAT_COUNTS = (1, 2, 5, 9, 14, 23, 38, 61, 90)
STAT_PASSES, STAT_SPP = 24, 64


@pytest.mark.slow
def test_the_three_path_integrators_estimate_one_integral():
    """The specification itself, on the oracle: on a scene of nine lights of 1 .. 90 triangles (32 x 24, box filter) the frame means
    under path_mats, path_ems and path_mis agree.  Per integrator STAT_PASSES independent passes of STAT_SPP samples per pixel
    (disjoint spp ranges, so no two passes share a seed); per pair and channel a two-sample Student's t (Welch) on the passes' frame
    means, significance 0.01 corrected for the 9 comparisons as tests/stat_harness.py does (Sidak).  Seeds are fixed: deterministic.

    The condition: NO TWO LIGHT TRIANGLES OVERLAP.  Emitter sampling adds the radiance of every emitter triangle that covers a
    point (each is sampled by its own area), a ray that arrives there sees the nearest one only, so overlapping coplanar light
    triangles make path_ems / path_mis and path_mats estimate different integrals -- a property of such a scene, not an error of
    the oracle.  Measured with this test's procedure on the same nine lights with all triangles of a light stacked in one cell
    (many_lights(overlapping=True)): path_mats 55-65 % below path_ems and path_mis (t = -35 .. -52 per channel), path_ems and
    path_mis 10-16 % apart (t = 7 .. 9).  With disjoint triangles: |t| <= 1.31 for all nine comparisons (p >= 0.2)."""
    from scipy import stats
    names = ("path_mats", "path_ems", "path_mis")
    means = {}
    for i, integ in enumerate(names):
        sc = lc.many_lights(STAT_COUNTS, integ, 32, 24, STAT_SPP, seed=21, rfilter=RFilter("box"))
        o = Oracle(sc, use_bvh=True)
        rows = []
        for k in range(STAT_PASSES):
            f, st = o.render_host(spp_count=STAT_SPP, spp_begin=(i * STAT_PASSES + k) * STAT_SPP)
            assert st["n_invalid"] == 0
            rows.append(f[..., :3].sum(axis=(0, 1)) / f[..., 3].sum())
        means[integ] = np.array(rows, dtype=np.float64)
    pairs = [(a, b) for ia, a in enumerate(names) for b in names[ia + 1:]]
    alpha = 1.0 - (1.0 - 0.01) ** (1.0 / (3 * len(pairs)))
    for a, b in pairs:
        for c in range(3):
            r = stats.ttest_ind(means[a][:, c], means[b][:, c], equal_var=False)
            print(f"[lights stat] {a} vs {b} channel {c}: means {means[a][:, c].mean():.5f} {means[b][:, c].mean():.5f}, t {r.statistic:.2f}, p {r.pvalue:.3f} (alpha {alpha:.5f})")
            assert r.pvalue > alpha, (a, b, c, r)
