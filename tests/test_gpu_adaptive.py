"""Tile-list renders, tile errors, tile selection and the adaptive loop (include/nori_hip.h: nori_hip_render_tiles,
nori_hip_tile_errors, nori_hip_select_tiles, nori_hip_render_adaptive) on the GPU: against the renders of a progression, the
oracle's binary64 film tile by tile, the numpy restatements of tests/adaptive_ref.py (validated by tests/test_adaptive_cpu.py),
and a replay of the loop from outside."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from nori_amd import NoriError, _capi
from nori_amd.scene import Bsdf, Mesh, RFilter
from tests import adaptive_ref as ar, film_cases, moments_ref as mr, scenes
from tests.backends import Oracle
from tests.test_gpu_parity import assert_within_summation_bound

pytestmark = pytest.mark.gpu

SIZES = {"45x37": (45, 37), "72x40": (72, 40)}      # 3 x 3 and 5 x 3 tiles, the right and bottom ones partial
ENGINES = ["megakernel", "wavefront"]
FILTERS = {"box": RFilter("box"), "tent": RFilter("tent"), "gaussian": RFilter("gaussian"),
           "gaussian5.2": RFilter("gaussian", radius=5.2, stddev=1.3), "mitchell4": RFilter("mitchell", radius=4.0)}
RAYS = ("n_camera_samples", "n_closest_rays", "n_shadow_rays")
LISTS = [(0, 4, 8), (5,), (2, 3, 7, 8)]
C = (0.5, 1.25, 3.0)            # the wall's radiance
C2 = (0.25, 1.5625, 9.0)        # its square, exact in float32


def _renderer(renderer_factory, sc, engine=None, **options):
    r = renderer_factory(sc)
    if engine is not None:
        r.set_option("engine", engine)
    for k, v in options.items():
        r.set_option(k, v)
    return r


def _n_tiles(size):
    ty, tx = ar.tile_grid(*size)
    return ty * tx


# ------------------------------------------------------------------ 1. a progression as a list
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("case", [("45x37", n) for n in FILTERS] + [("72x40", "gaussian"), ("72x40", "box")], ids=lambda c: "-".join(c))
def test_a_progression_as_a_list_gives_the_same_bits(renderer_factory, monkeypatch, engine, case):
    size, name = SIZES[case[0]], FILTERS[case[1]]
    n = _n_tiles(size)
    spp = 5
    r = _renderer(renderer_factory, film_cases.cornell(*size, spp, name), engine)

    def both(what):
        for mod, rem in ((1, 0), (2, 1), (4, 3)):
            want = r.render_moments_host(tile_mod=mod, tile_rem=rem)
            got = r.render_tiles_host(list(range(rem, n, mod)))
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]), (case, engine, what, mod, rem)
            assert all(want[2][k] == got[2][k] for k in RAYS + ("n_invalid", "engine")), (want[2], got[2])
            assert got[2]["engine"] == ENGINES.index(engine) and got[0][..., 3].max() > 0

    both("one batch")
    if engine == "wavefront":
        r.set_option("wavefront_samples", 4096)                              # several batches: regeneration, the pending gather beside the next batch
        both("wavefront_samples 4096")
    else:
        monkeypatch.setenv("NORI_HIP_FILM_SAMPLES", "4096")                  # read per call: several launches
        both("NORI_HIP_FILM_SAMPLES 4096")


def test_a_list_without_moments_is_a_plain_render(renderer_factory):
    import torch
    r = _renderer(renderer_factory, film_cases.cornell(45, 37, 3, RFilter("gaussian")))
    want, ws = r.render_host(tile_mod=2, tile_rem=0)
    frame = torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    gs = r.render_tiles_into([0, 2, 4, 6, 8], frame)
    assert np.array_equal(frame.cpu().numpy(), want) and all(ws[k] == gs[k] for k in RAYS)


# ------------------------------------------------------------------ 2. an arbitrary list against the oracle
SPP_ORACLE = 6


@functools.lru_cache(maxsize=None)
def _oracle_tiles(name, wall=False):
    """per tile t of the 45 x 37 frame: Oracle.render_f64(tile_mod = n_tiles, tile_rem = t) -- (total, abs_total, terms, stats)"""
    size = SIZES["45x37"]
    sc = mr.emitter_wall(*size, SPP_ORACLE, FILTERS[name], C2) if wall else film_cases.cornell(*size, SPP_ORACLE, FILTERS[name])
    o = Oracle(sc, use_bvh=True)
    n = _n_tiles(size)
    out = [o.render_f64(tile_mod=n, tile_rem=t, threads=1) for t in range(n)]
    o.close()
    for total, abs_total, terms, _ in out:
        total.setflags(write=False); abs_total.setflags(write=False); terms.setflags(write=False)
    return out


def _oracle_sum(per_tile, tiles):
    total = sum(per_tile[t][0] for t in tiles)
    abs_total = sum(per_tile[t][1] for t in tiles)
    terms = sum(per_tile[t][2].astype(np.uint64) for t in tiles).astype(np.uint32)
    stats = {k: sum(per_tile[t][3][k] for t in tiles) for k in RAYS}
    return total, abs_total, terms, stats


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", list(FILTERS))
def test_an_arbitrary_list_against_the_oracle(renderer_factory, engine, name):
    per_tile = _oracle_tiles(name)
    r = _renderer(renderer_factory, film_cases.cornell(*SIZES["45x37"], SPP_ORACLE, FILTERS[name]), engine)
    for tiles in LISTS:
        total, abs_total, terms, ostats = _oracle_sum(per_tile, tiles)
        rgbw, m2, st = r.render_tiles_host(list(tiles))
        assert_within_summation_bound(rgbw, total, abs_total, terms, f"list {tiles} {name} {engine}")
        assert all(st[k] == ostats[k] for k in RAYS), (st, ostats)
        untouched = terms == 0
        assert untouched.any() and not rgbw[untouched].any() and not m2[untouched].any()      # pixels no listed tile reaches: exactly 0
        assert np.isfinite(m2).all() and (m2[~untouched][:, 3] >= 0).all()


@pytest.mark.parametrize("engine", ENGINES)
def test_box_filter_moments_of_a_list_are_the_sum_of_squares(renderer_factory, engine):
    """As tests/test_gpu_moments.py::test_box_filter_moments_are_the_sum_of_squares, restricted to the listed tiles: under the box filter a
    pixel receives its own samples with weight 1, so m2.rgb is the sum of float32(L_s L_s) over the N samples of a pixel of a listed
    tile -- held to (N + 16) 2^-24 of the binary64 sum -- and exactly 0 in every other pixel."""
    width, height = SIZES["45x37"]
    box = film_cases.cornell(width, height, SPP_ORACLE, RFilter("box"))
    r1 = _renderer(renderer_factory, box, "megakernel")
    assert r1.border == 0
    L = np.stack([r1.render_host(spp_count=1, spp_begin=s)[0][..., :3] for s in range(SPP_ORACLE)])
    sq = (L * L).astype(np.float32).astype(np.float64).sum(0)
    r = _renderer(renderer_factory, box, engine)
    ys, xs = np.mgrid[0:height, 0:width]
    tile_of = (ys // 16) * 3 + xs // 16
    for tiles in LISTS:
        listed = np.isin(tile_of, tiles)
        total = np.concatenate([sq, np.full(sq.shape[:2] + (1,), float(SPP_ORACLE))], -1) * listed[..., None]
        terms = np.where(listed, SPP_ORACLE, 0).astype(np.uint32)
        rgbw, m2, _ = r.render_tiles_host(list(tiles))
        assert_within_summation_bound(m2, total, total, terms, f"box moments of list {tiles} {engine}")
        assert (m2[..., 3] == terms).all() and (rgbw[..., 3] == terms).all()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ["tent", "gaussian"])
def test_wide_filter_moments_of_a_list_against_the_squared_scene(renderer_factory, engine, name):
    """As tests/test_gpu_moments.py::test_wide_filter_moments_against_the_squared_scene: every sample of the wall carries C, whose
    square C2 is exact, so (m2.rgb, rgbw.w) of the listed tiles is the film of the wall with radiance C2 over the listed tiles' samples."""
    per_tile = _oracle_tiles(name, wall=True)
    r = _renderer(renderer_factory, mr.emitter_wall(*SIZES["45x37"], SPP_ORACLE, FILTERS[name], C), engine)
    for tiles in LISTS:
        total, abs_total, terms, _ = _oracle_sum(per_tile, tiles)
        rgbw, m2, _ = r.render_tiles_host(list(tiles))
        assert_within_summation_bound(np.concatenate([m2[..., :3], rgbw[..., 3:]], -1), total, abs_total, terms, f"wall moments of list {tiles} {name} {engine}")


# ------------------------------------------------------------------ 3. refusals and the empty list
@pytest.mark.parametrize("engine", ENGINES)
def test_bad_lists_are_refused_and_the_empty_list_touches_nothing(renderer_factory, engine):
    import torch
    r = _renderer(renderer_factory, film_cases.cornell(*SIZES["45x37"], 2, RFilter("gaussian")), engine)
    for tiles, word in (([0, 9], "out of range"), ([4, 0xffffffff], "out of range"), ([3, 2], "ascending"), ([1, 5, 5, 6], "ascending")):
        with pytest.raises(NoriError, match=rf"NORI_ERR_INVALID_ARGUMENT: .*{word}"):
            r.render_tiles_host(tiles)
    with pytest.raises(NoriError, match=r"NORI_ERR_UNSUPPORTED: \S+"):
        r.render_tiles_host([0, 1], seed_mode=_capi.SEED_NORI_BLOCK)
    a = torch.full(r.frame_shape(), 3.0, dtype=torch.float32, device="cuda:0")
    b = torch.full(r.frame_shape(), 5.0, dtype=torch.float32, device="cuda:0")
    st = r.render_tiles_into([], a, b)
    assert (a == 3.0).all() and (b == 5.0).all() and st["n_camera_samples"] == 0
    import ctypes
    p = r._params(0, 2, 2, 1, False, None)          # the list names the tiles: no progression beside it
    host_frame = np.zeros(r.frame_shape(), np.float32)
    rc = r._lib.nori_hip_render_tiles_host(r._h, ctypes.byref(p), None, 0, _capi.ptr(host_frame), None, None)
    assert _capi.STATUS[rc] == "NORI_ERR_INVALID_ARGUMENT" and b"tile_mod" in r._lib.nori_hip_last_error(r._h) and not host_frame.any()
    rgbw, m2, st = r.render_tiles_host([0, 1])      # and the context still renders
    assert st["n_camera_samples"] == 2 * 256 * 2 and rgbw[..., 3].max() > 0
    r.set_option("film_order", "reference")
    with pytest.raises(NoriError, match=r"NORI_ERR_UNSUPPORTED: \S+"):
        r.render_tiles_host([0, 1])
    with pytest.raises(NoriError, match=r"NORI_ERR_UNSUPPORTED: \S+"):
        r.render_adaptive_host(0.1, pass_spp=1, spp_count=2)


# ------------------------------------------------------------------ 4. tile errors and selection on made-up frames
@pytest.mark.parametrize("size", [(45, 37), (520, 520)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_errors_and_selection_on_made_up_frames(renderer_factory, size):
    """No render.  520 x 520 is 33 x 33 = 1089 tiles: more than one workgroup's width for the selection (five workgroups count and
    scatter, the scan's lanes own a count each or none), the last tile column and row 8 pixels wide."""
    import torch
    width, height = size
    r = _renderer(renderer_factory, mr.emitter_wall(width, height, 1, RFilter("gaussian"), C))
    rgbw, m2 = ar.random_pair(width, height, r.border, seed=width)
    want = ar.tile_errors(rgbw, m2, r.border)
    got = r.tile_errors(rgbw, m2)
    assert got.dtype == np.float32 and got.shape == ar.tile_grid(width, height)
    assert got.tobytes() == want.tobytes()
    assert r.tile_errors(rgbw, m2).tobytes() == got.tobytes()
    on_device = r.tile_errors(torch.from_numpy(rgbw).cuda(), torch.from_numpy(m2).cuda())
    assert on_device.cpu().numpy().tobytes() == got.tobytes()
    assert want[1, 1] == 0 and np.count_nonzero(want) == want.size - 1

    n = want.size
    te = want.copy().reshape(-1)
    te[n // 2] = np.nan
    every = np.arange(n, dtype=np.uint32)
    finite = np.sort(te[np.isfinite(te)])
    targets = [-1.0, 0.0, float(finite[len(finite) // 3]), float(finite[len(finite) // 2]), float(finite[-1]), float(np.inf)]
    for tiles in (every, every[::3], every[n // 2:n // 2 + 1], every[:0]):
        for target in targets:
            ref = ar.select(te, target, tiles)
            out = r.select_tiles(te, target, tiles)
            assert out.dtype == np.uint32 and out.tobytes() == ref.tobytes(), (size, target, len(tiles))
            assert r.select_tiles(te, target, tiles).tobytes() == out.tobytes()
    assert ar.select(te, -1.0, every).size == n                                 # one target keeps all tiles,
    assert ar.select(te, float(np.inf), every).tolist() == [n // 2]             # one keeps none but the NaN tile,
    assert 0 < ar.select(te, targets[3], every).size < n                        # and one splits them
    with pytest.raises(NoriError, match="INVALID_ARGUMENT"):
        r.select_tiles(te, 0.1, [0, n])
    with pytest.raises(NoriError, match="INVALID_ARGUMENT"):
        r.select_tiles(te, 0.1, [2, 1])


def test_selection_of_more_tiles_than_the_scan_has_lanes_for_single_counts(renderer_factory):
    """4112 x 4112 is 257 x 257 = 66049 tiles: 259 workgroups count and scatter, so a lane of the scan owns TWO consecutive counts (the
    form a 16384^2 frame's 2^20 tiles run with 16 per lane) and the last lanes own none.  Made-up tile errors, no frames."""
    r = _renderer(renderer_factory, mr.emitter_wall(4112, 4112, 1, RFilter("box"), C))
    n = 257 * 257
    assert r.tile_grid() == (257, 257)
    rng = np.random.default_rng(5)
    te = rng.uniform(0.0, 1.0, n).astype(np.float32)
    te[[0, 255, 256, 257, 511, 512, 65535, 65536, n - 1]] = np.float32([np.nan, 0.9, 0.1, 0.9, 0.1, 0.9, 0.9, np.nan, 0.9])      # around the seams of the blocks and runs
    every = np.arange(n, dtype=np.uint32)
    for tiles in (every, every[1::2], every[65000:]):
        for target in (-1.0, 0.25, 0.5, 0.999, float(np.inf)):
            ref = ar.select(te, target, tiles)
            out = r.select_tiles(te, target, tiles)
            assert out.tobytes() == ref.tobytes(), (target, len(tiles))
    assert ar.select(te, float(np.inf), every).tolist() == [0, 65536] and 0 < ar.select(te, 0.5, every).size < n


# ------------------------------------------------------------------ 5. the loop, by replay
def wall_and_cornell(width, height, spp, rfilter):
    """The Cornell box of film_cases with a constant emitter (moments_ref.emitter_wall's material: black albedo, every camera sample
    that meets it carries exactly its radiance) half a unit in front of the camera, over the half x >= 0 of the view."""
    sc = film_cases.cornell(width, height, spp, rfilter)
    v, f = scenes.quad((0, -10, 3.7), (10, -10, 3.7), (10, 10, 3.7), (0, 10, 3.7))
    sc.meshes.append(Mesh(v, f, bsdf=Bsdf("diffuse", (0.0, 0.0, 0.0)), radiance=(0.5, 0.5, 0.5), name="wall"))
    return sc


LOOP_E, LOOP_K, LOOP_N = 0.119, 4, 24


@pytest.mark.parametrize("engine", ENGINES)
def test_the_loop_is_its_replay(renderer_factory, engine):
    """render_adaptive(E, K = 4, N = 24) on the 72 x 40 frame (5 x 3 tiles) whose one half sees the constant wall, replayed pass by pass
    with render_tiles of {t : tile_spp[t] > k K} into zeroed frames.

    E = 0.119 is an input, not a tolerance: it lies between tile errors observed on the GPU (MI355X, both engines give the same
    values; tiles 3, 4, 8, 9, 13, 14 see only the wall, tiles 2, 7, 12 its edge).  Tile errors of the active tiles after each pass:
        pass 1 ( 8 spp)  0: .1498  1: .2070  2: .0517  3: 0  4: 0  5: .1726  6: .2815  7: .0582  8: 0  9: 0  10: .1598  11: .3270  12: .0466  13: 0  14: 0
                         -> the nine tiles of the wall and its edge retire (largest .0582), the other six stay (smallest .1498)
        pass 2 (12 spp)  0: .1273  1: .1889  5: .1380  6: .2352  10: .1313  11: .2692       -> all stay
        pass 3 (16 spp)  0: .1142  1: .1701  5: .1240  6: .2066  10: .1143  11: .2521       -> 0 and 10 retire, 5 stays
        pass 4 (20 spp)  1: .1574  5: .1121  6: .1840  11: .2232                            -> 5 retires
        pass 5 (24 spp)  1: .1506  6: .1684  11: .2119                                      -> the budget: three tiles still active
    so tile_spp = 16 24 8 8 8 / 20 24 8 8 8 / 16 24 8 8 8: tiles retire in three different passes.  The nearest errors on either side of
    E are .1143 and .1240 (pass 3); the render is deterministic, so the gap need not cover noise."""
    import torch
    width, height = SIZES["72x40"]
    K, N, E = LOOP_K, LOOP_N, LOOP_E
    r = _renderer(renderer_factory, wall_and_cornell(width, height, N, RFilter("gaussian")), engine)
    zeros = lambda: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    a, b = zeros(), zeros()
    tile_spp_t, summary, stats = r.render_adaptive(a, b, E, pass_spp=K, spp_count=N)
    tile_spp = tile_spp_t.cpu().numpy().astype(np.int64).reshape(-1)
    n = tile_spp.size
    assert n == 15 and summary["n_tiles"] == n
    print(f"[adaptive loop] {engine}: tile_spp {tile_spp.tolist()} summary {summary}")

    ra, rb = zeros(), zeros()
    replay_stats, passes, active_at_end = [], 0, None
    for k in range((N + K - 1) // K):
        active = np.flatnonzero(tile_spp > k * K).astype(np.uint32)
        if active.size == 0:
            break
        count = min(K, N - k * K)
        replay_stats.append(r.render_tiles_into(active, ra, rb, spp_count=count, spp_begin=k * K))
        passes += 1
        nxt = np.flatnonzero(tile_spp > (k + 1) * K).astype(np.uint32)
        if k == 0:
            assert nxt.tolist() == active.tolist()      # the first pass is not evaluated: nothing retires
            continue
        te = r.tile_errors(ra, rb).cpu().numpy().reshape(-1)
        print(f"[adaptive loop] {engine}: after pass {k} tile errors {' '.join(f'{v:.4f}' for v in te)}")
        stay = ar.select(te, E, active)
        if k * K + count < N:
            assert nxt.tolist() == stay.tolist(), (k, te.tolist())      # the tiles that leave: exactly the active ones with tile_err <= E
        active_at_end = stay
    assert torch.equal(a, ra) and torch.equal(b, rb)
    assert summary["passes"] == passes
    pixels = ar.tile_pixels(width, height).reshape(-1)
    assert stats["n_camera_samples"] == int((tile_spp * pixels).sum())
    assert all(stats[key] == sum(s[key] for s in replay_stats) for key in RAYS)
    assert (summary["spp_min"], summary["spp_max"]) == (int(tile_spp.min()), int(tile_spp.max()))
    assert summary["n_unconverged"] == active_at_end.size
    err, frame = r.error_map(a, b, threshold=E)
    assert summary["frame"] == frame
    # the test is not vacuous: tiles retired in at least two different passes, and at least one was still active at the budget
    retired_at = set(tile_spp[tile_spp < N].tolist())
    assert len(retired_at) >= 2, tile_spp.tolist()
    assert 2 * K in retired_at                              # the wall's tiles: retired at the first evaluation
    assert summary["n_unconverged"] >= 1 and (tile_spp == N).any()
    # the host twin returns the same frames, map and counts
    rgbw, m2, emap, spp_host, s2, st2 = r.render_adaptive_host(E, pass_spp=K, spp_count=N)
    assert np.array_equal(rgbw, a.cpu().numpy()) and np.array_equal(m2, b.cpu().numpy()) and np.array_equal(emap, err.cpu().numpy())
    assert spp_host.reshape(-1).tolist() == tile_spp.tolist() and s2 == summary and all(st2[key] == stats[key] for key in RAYS)


# ------------------------------------------------------------------ 6. limits of the loop
@pytest.mark.parametrize("engine", ENGINES)
def test_limits_of_the_loop(renderer_factory, engine):
    import torch
    width, height = SIZES["45x37"]
    K, N = 3, 11
    r = _renderer(renderer_factory, film_cases.cornell(width, height, N, RFilter("gaussian")), engine)
    zeros = lambda: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    # target 0 never retires a tile with an error: the uniform loop's frames, bit for bit
    a, b = zeros(), zeros()
    done, last, ust = r.render_to_error(a, b, 0.0, pass_spp=K, spp_count=N)
    c, d = zeros(), zeros()
    tile_spp, summary, st = r.render_adaptive(c, d, 0.0, pass_spp=K, spp_count=N)
    assert done == N and torch.equal(a, c) and torch.equal(b, d)
    assert (tile_spp == N).all() and summary["passes"] == 4 and summary["n_unconverged"] == 9 and summary["frame"] == last
    assert all(st[k] == ust[k] for k in RAYS)
    # a target above every tile error: two passes, then every tile retires
    c, d = zeros(), zeros()
    tile_spp, summary, st = r.render_adaptive(c, d, 1e9, pass_spp=K, spp_count=N)
    assert (tile_spp == 2 * K).all() and summary["passes"] == 2 and summary["n_unconverged"] == 0
    assert (summary["spp_min"], summary["spp_max"]) == (2 * K, 2 * K) and st["n_camera_samples"] == width * height * 2 * K
    e, f = zeros(), zeros()
    r.render_moments_into(e, f, spp_count=K)
    r.render_moments_into(e, f, spp_count=K, spp_begin=K)
    assert torch.equal(c, e) and torch.equal(d, f)
    # one pass spends the samples: nothing is evaluated for retiring, the summary still describes the frames
    tile_spp, summary, st = r.render_adaptive(zeros(), zeros(), 1e9, pass_spp=8, spp_count=5)
    assert (tile_spp == 5).all() and summary["passes"] == 1 and summary["n_unconverged"] == 0 and summary["frame"]["n_pixels"] == width * height
    for bad in (dict(pass_spp=0), dict(pass_spp=2, target=-0.5), dict(pass_spp=2, target=float("nan"))):
        with pytest.raises(NoriError, match="INVALID_ARGUMENT"):
            r.render_adaptive(zeros(), zeros(), bad.get("target", 0.1), pass_spp=bad["pass_spp"], spp_count=4)
