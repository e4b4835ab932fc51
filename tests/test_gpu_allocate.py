"""Sample levels per tile from a pilot on the GPU (include/nori_hip.h: nori_hip_allocate_tiles, nori_hip_render_allocated): the
classification and the grouping against the restatement of tests/allocate_ref.py (validated by tests/test_allocate_cpu.py) bit for
bit on made-up tile errors, and the loop by a replay from its level log with render_tiles calls in the stated order."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nori_amd import NoriError, _capi, host
from nori_amd.scene import RFilter
from tests import adaptive_ref as ar, allocate_ref as al, film_cases, moments_ref as mr
from tests.exr_reader import read_exr_rgb

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 45, 37                   # 3 x 3 tiles, the right column 13 px wide, the bottom row 5 px high
PILOT, BUDGET = 8, 64           # levels 8, 16, 32, 64
NAMES = ("albedo", "normal", "depth")
RAYS = ("n_camera_samples", "n_closest_rays", "n_shadow_rays")
WALL = (0.5, 1.25, 3.0)


# ------------------------------------------------------------------ 1. classification and grouping on made-up errors, no render
def _random_case(n, J, seed, target):
    rng = np.random.default_rng(seed)
    e = (F(max(target, 0.05)) * np.exp(rng.uniform(-1.0, 3.0, n))).astype(F)      # ratios E / target of 0.37 .. 20: every level is somebody's need
    e[rng.integers(0, n, max(n // 8, 1))] = F(target)                              # equal to the target: done
    special = np.array([np.nan, np.inf, -np.inf, 0.0], F)
    e[rng.choice(n, special.size, replace=False)] = special
    level = rng.integers(0, J + 1, n).astype(np.uint32)                            # every level as the start
    done = (rng.uniform(0, 1, n) < 0.2).astype(np.uint32)                          # tiles already done
    return e, level, done


def _every_pair_case(n, spp, target, headroom):
    """tile t asks for pair t mod n_pairs: need = 0.9 spp_j lies in (spp_(j-1), spp_j], so E = target sqrt(0.9 spp_j / (headroom spp_i)) --
    above the target for a headroom up to 1.8"""
    J = len(spp) - 1
    ps = al.pairs(J)
    level, e = np.zeros(n, np.uint32), np.zeros(n, F)
    for t in range(n):
        i, j = ps[t % len(ps)]
        level[t] = i
        e[t] = F(target) * F(np.sqrt(0.9 * spp[j] / (headroom * spp[i])))
    return e, level, np.zeros(n, np.uint32)


def _check(r, e, target, headroom, spp, level, done, what):
    want = al.allocate(e, target, headroom, spp, level, done)
    got = r.allocate_tiles(e, target, level, done, pilot_spp=spp[0], spp_count=spp[-1], headroom=headroom)
    for w, g, name in zip(want, got, ("level", "done", "tiles", "bucket_begin")):
        assert g.dtype == np.uint32 and g.tobytes() == w.tobytes(), (what, name, int((g != w).sum()) if g.shape == w.shape else (g.shape, w.shape))
    again = r.allocate_tiles(e, target, level, done, pilot_spp=spp[0], spp_count=spp[-1], headroom=headroom)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got)), what      # the same inputs give the same bytes
    return want


@pytest.mark.parametrize("size", [(45, 37), (320, 240), (4112, 4096)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_classification_and_grouping_on_made_up_errors(renderer_factory, size):
    """9 tiles (partial right and bottom tiles); 300 tiles: two count blocks; 65 792 tiles: 257 count blocks, so a lane of the scan owns
    a run of counts that crosses from one bucket into the next (28 x 257 = 7196 counts, 29 per lane).  No render: the big frame only
    uploads a scene with that camera."""
    width, height = size
    r = renderer_factory(mr.emitter_wall(width, height, 1, RFilter("box"), WALL))
    ty, tx = r.tile_grid()
    n = ty * tx
    assert n == {45: 9, 320: 300, 4112: 65792}[width]
    full = al.levels(2, 256)            # J = 7: 28 pairs
    short = al.levels(PILOT, BUDGET)    # J = 3: 6 pairs
    assert len(full) == 8 and len(short) == 4
    for spp in (full, short):
        J = len(spp) - 1
        for target, headroom in ((0.1, 1.0), (0.1, 1.5), (0.0, 1.0)):
            e, level, done = _random_case(n, J, seed=n + J, target=target)
            new_level, new_done, tiles, begin = _check(r, e, target, headroom, spp, level, done, (size, J, target, headroom, "random"))
            live_nan = np.isnan(e) & (done == 0)
            assert (new_level[live_nan] == J).all()
            if target == 0.0:
                with np.errstate(invalid="ignore"):
                    assert (new_level[(done == 0) & ~(e <= 0)] == J).all()
        for headroom in (1.0, 1.5):     # every bucket filled (where the frame has the tiles for it)
            e, level, done = _every_pair_case(n, spp, 0.1, headroom)
            _, _, tiles, begin = _check(r, e, 0.1, headroom, spp, level, done, (size, J, headroom, "every pair"))
            filled = np.diff(begin[:J * (J + 1) // 2 + 1].astype(np.int64)) > 0
            assert filled.sum() == min(n, J * (J + 1) // 2) and tiles.size == n
        # all but one bucket empty: every tile at level 1 asks for the top; and with everything done nothing moves
        e = np.full(n, 50.0, F)
        _, _, tiles, begin = _check(r, e, 0.1, 1.0, spp, np.ones(n, np.uint32), np.zeros(n, np.uint32), (size, J, "one bucket"))
        assert tiles.tolist() == list(range(n)) and (np.diff(begin.astype(np.int64)) > 0).sum() == 1
        _, _, tiles, begin = _check(r, e, 0.1, 1.0, spp, np.ones(n, np.uint32), np.ones(n, np.uint32), (size, J, "all done"))
        assert tiles.size == 0 and not begin.any()
    # one level: nothing can move, every live tile is done
    e, level, done = _random_case(n, 0, seed=1, target=0.1)
    new_level, new_done, tiles, begin = _check(r, e, 0.1, 1.0, [8], level, done, (size, "one level"))
    assert tiles.size == 0 and new_done.all() and not new_level.any()


# ------------------------------------------------------------------ 2. the loop, by replay from its log
def _cornell(renderer_factory, engine=None):
    r = renderer_factory(film_cases.cornell(W, H, BUDGET, RFilter("gaussian")))
    if engine is not None:
        r.set_option("engine", engine)
    return r


def _replay(r, tw, E, rounds, headroom, evaluate):
    """Renders the pilot and then, round by round, the moves read off the twin's level log, pair by pair in ascending (i, j) and
    ascending tile id, into zeroed frames; before each round the restated rule is applied to the replayed frames' tile errors and
    must give the log's next row.  Returns (rgbw, m2, stats of the calls, the restatement's done flags, the final tile errors)."""
    import torch
    spp = al.levels(PILOT, BUDGET)
    J = len(spp) - 1
    log = tw["level_log"]
    n = log.shape[1]
    assert log.shape == (rounds + 1, n) and not log[0].any()
    zeros = lambda: torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0")
    ra, rb = zeros(), zeros()
    calls = [r.render_moments_into(ra, rb, spp_count=spp[0])]
    level, done = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for k in range(1, rounds + 1):
        te = evaluate(ra, rb)
        print(f"[allocate replay] round {k}: tile errors {' '.join(f'{v:.4f}' for v in te)} target {E:.4f}")
        level, done, tiles, begin = al.allocate(te, E, headroom, spp, level, done)
        assert log[k].tolist() == level.tolist(), (k, te.tolist())
        moves = al.moves_of_log(log, k, J)
        assert np.concatenate([t for t, _, _ in moves] + [np.zeros(0, np.uint32)]).tolist() == tiles.tolist()      # the grouping, in its order
        if not moves:
            assert all(log[m].tolist() == level.tolist() for m in range(k, rounds + 1))      # rounds that did not run repeat the levels
            break
        for t, i, j in moves:
            calls.append(r.render_tiles_into(t, ra, rb, spp_count=spp[j] - spp[i], spp_begin=spp[i]))
    return ra, rb, calls, done, evaluate(ra, rb)


def _check_loop(r, tw, ra, rb, calls, te_final, E, frame_summary):
    spp = al.levels(PILOT, BUDGET)
    tile_spp = np.asarray(spp, np.uint32)[tw["level_log"][-1]]
    assert np.array_equal(tw["rgbw"], ra.cpu().numpy()) and np.array_equal(tw["m2"], rb.cpu().numpy())
    assert tw["tile_spp"].reshape(-1).tolist() == tile_spp.tolist()
    s = tw["summary"]
    assert s["passes"] == len(calls) and s["n_tiles"] == tile_spp.size
    assert (s["spp_min"], s["spp_max"]) == (int(tile_spp.min()), int(tile_spp.max()))
    with np.errstate(invalid="ignore"):
        assert s["n_unconverged"] == int((~(te_final <= F(E))).sum())
    assert s["frame"] == frame_summary
    pixels = ar.tile_pixels(W, H).reshape(-1)
    assert tw["stats"]["n_camera_samples"] == int((tile_spp.astype(np.int64) * pixels).sum())
    assert all(tw["stats"][key] == sum(c[key] for c in calls) for key in RAYS)


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("engine", ["megakernel", "wavefront"])
def test_the_loop_is_its_replay(renderer_factory, engine, rounds):
    """The 45 x 37 Cornell box, pilot 8, budget 64.  The target is the median of the pilot's own tile errors: the input of the run, so
    that by construction some tiles stop at level 0 and the others move."""
    r = _cornell(renderer_factory, engine)
    rgbw, m2, _ = r.render_moments_host(spp_count=PILOT)
    pilot_te = r.tile_errors(rgbw, m2).reshape(-1)
    E = float(np.median(pilot_te))
    tw = r.render_allocated_host(E, pilot_spp=PILOT, max_rounds=rounds, spp_count=BUDGET)
    print(f"[allocate loop] {engine} rounds {rounds}: levels {tw['level_log'].tolist()} summary {tw['summary']}")
    evaluate = lambda a, b: r.tile_errors(a, b).cpu().numpy().reshape(-1)
    ra, rb, calls, done, te_final = _replay(r, tw, E, rounds, 1.0, evaluate)
    err, frame = r.error_map(ra, rb, threshold=E)
    _check_loop(r, tw, ra, rb, calls, te_final, E, frame)
    assert tw["err"].tobytes() == err.cpu().numpy().tobytes()
    first = tw["level_log"][1]
    assert (first == 0).any() and (first > 0).any()                  # some tiles stopped on the pilot, some moved
    assert (first[pilot_te <= F(E)] == 0).all() and (first[pilot_te > F(E)] > 0).all()
    assert len(calls) >= 2 and tw["summary"]["spp_min"] == PILOT and tw["summary"]["spp_max"] > PILOT


def test_headroom_is_part_of_the_rule_on_the_device(renderer_factory):
    r = _cornell(renderer_factory)
    rgbw, m2, _ = r.render_moments_host(spp_count=PILOT)
    E = float(np.median(r.tile_errors(rgbw, m2)))
    tw = r.render_allocated_host(E, pilot_spp=PILOT, max_rounds=2, headroom=2.0, spp_count=BUDGET)
    evaluate = lambda a, b: r.tile_errors(a, b).cpu().numpy().reshape(-1)
    ra, rb, calls, done, te_final = _replay(r, tw, E, 2, 2.0, evaluate)
    _check_loop(r, tw, ra, rb, calls, te_final, E, r.error_map(ra, rb, threshold=E)[1])
    plain = r.render_allocated_host(E, pilot_spp=PILOT, max_rounds=2, spp_count=BUDGET)
    assert (tw["level_log"][1] >= plain["level_log"][1]).all()


# ------------------------------------------------------------------ 3. anchors
@pytest.mark.parametrize("engine", ["megakernel", "wavefront"])
def test_anchors(renderer_factory, engine):
    r = _cornell(renderer_factory, engine)
    spp = al.levels(PILOT, BUDGET)
    # a target above every pilot error: the frames are render_moments of pilot_spp
    tw = r.render_allocated_host(1e9, pilot_spp=PILOT, max_rounds=3, spp_count=BUDGET)
    rgbw, m2, st = r.render_moments_host(spp_count=PILOT)
    assert np.array_equal(tw["rgbw"], rgbw) and np.array_equal(tw["m2"], m2) and not tw["level_log"].any() and (tw["tile_spp"] == PILOT).all()
    assert tw["summary"]["passes"] == 1 and tw["summary"]["n_unconverged"] == 0 and all(tw["stats"][k] == st[k] for k in RAYS)
    # target 0: the pilot plus one render_tiles of all tiles over [spp_0, spp_J)
    import torch
    tw = r.render_allocated_host(0.0, pilot_spp=PILOT, max_rounds=3, spp_count=BUDGET)
    a, b = (torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0") for _ in range(2))
    r.render_moments_into(a, b, spp_count=PILOT)
    r.render_tiles_into(np.arange(9, dtype=np.uint32), a, b, spp_count=spp[-1] - spp[0], spp_begin=spp[0])
    assert np.array_equal(tw["rgbw"], a.cpu().numpy()) and np.array_equal(tw["m2"], b.cpu().numpy())
    assert (tw["level_log"][1:] == len(spp) - 1).all() and (tw["tile_spp"] == BUDGET).all()
    assert tw["summary"]["passes"] == 2 and tw["summary"]["n_unconverged"] == 9 and tw["stats"]["n_camera_samples"] == W * H * BUDGET
    # a budget below two levels: the pilot alone, whatever the target
    tw = r.render_allocated_host(0.0, pilot_spp=PILOT, max_rounds=2, spp_count=2 * PILOT - 1)
    assert np.array_equal(tw["rgbw"], rgbw) and tw["summary"]["passes"] == 1 and (tw["tile_spp"] == PILOT).all() and tw["summary"]["n_unconverged"] == 9


# ------------------------------------------------------------------ 4. the denoised metric
@pytest.mark.parametrize("rounds", [1, 3])
def test_the_denoised_loop_is_its_replay(renderer_factory, rounds):
    import torch
    r = _cornell(renderer_factory)
    feats, _ = r.render_features_host(spp_count=PILOT)
    fd = {name: torch.from_numpy(feats[name]).cuda() for name in NAMES}
    params = dict(radius=3, patch=1)

    def outputs(a, b):
        out = (torch.empty((H, W, 3), device="cuda:0"), torch.empty((H, W, 3), device="cuda:0"), torch.empty((H, W), device="cuda:0"))
        r.denoise_var_into(out[0], out[1], a, b, wsum=out[2], **fd, **params)      # the whole frame: the not-done tiles' pixels have these bits
        return out

    evaluate = lambda a, b: r.denoised_tile_errors(*outputs(a, b)).cpu().numpy().reshape(-1)
    a, b = (torch.zeros(r.frame_shape(), dtype=torch.float32, device="cuda:0") for _ in range(2))
    r.render_moments_into(a, b, spp_count=PILOT)
    pilot_te = evaluate(a, b)
    E = float(np.median(pilot_te))
    tw = r.render_allocated_denoised_host(E, **feats, pilot_spp=PILOT, max_rounds=rounds, spp_count=BUDGET, **params)
    print(f"[allocate denoised loop] rounds {rounds}: levels {tw['level_log'].tolist()} summary {tw['summary']}")
    ra, rb, calls, done, te_final = _replay(r, tw, E, rounds, 1.0, evaluate)
    rgb, var, wsum = outputs(ra, rb)
    derr, frame = r.denoised_error_map(rgb, var, wsum, threshold=E)
    _check_loop(r, tw, ra, rb, calls, te_final, E, frame)
    want = r.denoise_var_host(tw["rgbw"], tw["m2"], **feats, **params)      # the outputs: denoise_var of the final frames
    assert all(tw[k].tobytes() == w.tobytes() for k, w in zip(("rgb", "var", "wsum"), want))
    assert tw["err"].tobytes() == derr.cpu().numpy().tobytes()
    first = tw["level_log"][1]
    assert (first == 0).any() and (first > 0).any()
    # without feature frames the loop runs too, and ends in the same final filter
    bare = r.render_allocated_denoised_host(E, pilot_spp=PILOT, max_rounds=1, spp_count=BUDGET)
    want = r.denoise_var_host(bare["rgbw"], bare["m2"])
    assert all(bare[k].tobytes() == w.tobytes() for k, w in zip(("rgb", "var", "wsum"), want))


# ------------------------------------------------------------------ 5. determinism and isolation
def test_two_runs_give_the_same_bytes_and_other_calls_are_untouched(renderer_factory):
    r = _cornell(renderer_factory)
    feats, _ = r.render_features_host(spp_count=PILOT)

    def others():
        plain, _ = r.render_host(spp_count=8)
        ad = r.render_adaptive_host(0.2, pass_spp=4, spp_count=12)
        sel = r.select_tiles(np.linspace(0, 1, 9).astype(F), 0.5, np.arange(9))
        return [plain, ad[0], ad[1], ad[2], ad[3], sel], ad[4]

    before, s_before = others()
    E = 0.12
    raw = r.render_allocated_host(E, pilot_spp=PILOT, max_rounds=3, spp_count=BUDGET)
    den = r.render_allocated_denoised_host(0.03, **feats, pilot_spp=PILOT, max_rounds=2, spp_count=BUDGET)
    assert raw["summary"]["passes"] >= 2 and den["summary"]["passes"] >= 2
    after, s_after = others()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after)) and s_before == s_after
    raw2 = r.render_allocated_host(E, pilot_spp=PILOT, max_rounds=3, spp_count=BUDGET)
    den2 = r.render_allocated_denoised_host(0.03, **feats, pilot_spp=PILOT, max_rounds=2, spp_count=BUDGET)
    assert all(raw2[k].tobytes() == raw[k].tobytes() for k in ("rgbw", "m2", "err", "tile_spp", "level_log")) and raw2["summary"] == raw["summary"]
    assert all(den2[k].tobytes() == den[k].tobytes() for k in ("rgbw", "m2", "rgb", "var", "wsum", "err", "tile_spp", "level_log")) and den2["summary"] == den["summary"]


# ------------------------------------------------------------------ 6. error codes
def test_error_codes(renderer_factory):
    r = _cornell(renderer_factory)
    ok = dict(pilot_spp=PILOT, max_rounds=2, spp_count=BUDGET)
    for bad, word in ((dict(pilot_spp=1), "pilot_spp"), (dict(pilot_spp=0), "pilot_spp"), (dict(max_rounds=0), "max_rounds"), (dict(headroom=0.5), "headroom"),
                      (dict(headroom=float("nan")), "headroom"), (dict(spp_count=PILOT - 1), "spp_count"), (dict(tile_mod=2), "tile_mod")):
        with pytest.raises(NoriError, match=rf"NORI_ERR_INVALID_ARGUMENT: .*{word}"):
            r.render_allocated_host(0.1, **{**ok, **bad})
    for target in (-0.5, float("nan")):
        with pytest.raises(NoriError, match=r"NORI_ERR_INVALID_ARGUMENT: .*target"):
            r.render_allocated_host(target, **ok)
    with pytest.raises(NoriError, match=r"NORI_ERR_INVALID_ARGUMENT: .*1 \.\. 8"):
        r.render_allocated_denoised_host(0.1, radius=9, **ok)
    with pytest.raises(NoriError, match=r"NORI_ERR_INVALID_ARGUMENT: .*metric"):
        r._render_allocated_host(2, 0.1, (None, None, None), PILOT, 2, 1.0, BUDGET, 0, False, _capi.SEED_PER_SAMPLE, 1, {})
    with pytest.raises(NoriError, match=r"NORI_ERR_UNSUPPORTED: \S+"):
        r.render_allocated_host(0.1, seed_mode=_capi.SEED_NORI_BLOCK, **ok)
    te, zero = np.full(9, 0.3, F), np.zeros(9, np.uint32)
    with pytest.raises(NoriError, match=r"NORI_ERR_INVALID_ARGUMENT: .*level"):
        r.allocate_tiles(te, 0.1, np.full(9, 4, np.uint32), zero, pilot_spp=PILOT, spp_count=BUDGET)      # the top level is 3
    for bad in (dict(pilot_spp=1), dict(headroom=0.0), dict(spp_count=4)):
        with pytest.raises(NoriError, match="NORI_ERR_INVALID_ARGUMENT"):
            r.allocate_tiles(te, 0.1, zero, zero, **{**dict(pilot_spp=PILOT, spp_count=BUDGET), **bad})
    with pytest.raises(NoriError, match="NORI_ERR_INVALID_ARGUMENT"):
        r.allocate_tiles(te, -1.0, zero, zero, pilot_spp=PILOT, spp_count=BUDGET)
    p, ap = r._params(0, BUDGET, 1, 0, False, None), _capi.AllocateParams(PILOT, 2, 0.1, 1.0, 0)
    frame = np.zeros(r.frame_shape(), F)
    rc = r._lib.nori_hip_render_allocated_host(r._h, C.byref(p), None, None, _capi.ptr(frame), None, None, None, None, None, None, None, None, None, None, None, None)
    assert _capi.STATUS[rc] == "NORI_ERR_INVALID_ARGUMENT" and not frame.any()
    ap.metric = 1      # metric 1 without a buffer for the denoised frame
    rc = r._lib.nori_hip_render_allocated_host(r._h, C.byref(p), C.byref(ap), None, _capi.ptr(frame), None, None, None, None, None, None, None, None, None, None, None, None)
    assert _capi.STATUS[rc] == "NORI_ERR_INVALID_ARGUMENT" and b"metric 1" in r._lib.nori_hip_last_error(r._h)
    r.set_option("film_order", "reference")
    with pytest.raises(NoriError, match=r"NORI_ERR_UNSUPPORTED: \S+"):
        r.render_allocated_host(0.1, **ok)
    r.set_option("film_order", "fast")
    assert r.render_allocated_host(1e9, **ok)["summary"]["passes"] == 1      # the context still renders


# ------------------------------------------------------------------ 7. the command line
def test_cli_allocate(renderer_factory, tmp_path):
    (tmp_path / "floor.obj").write_text("v -3 0 -3\nv -3 0 3\nv 3 0 3\nv 3 0 -3\nf 1 2 3 4\n")
    (tmp_path / "light.obj").write_text("v -0.5 2 -0.5\nv 0.5 2 -0.5\nv 0.5 2 0.5\nv -0.5 2 0.5\nf 1 2 3 4\n")
    (tmp_path / "s.xml").write_text("""<scene><integrator type="path_mis"/>
      <sampler type="independent"><integer name="sampleCount" value="32"/></sampler>
      <camera type="perspective"><integer name="width" value="40"/><integer name="height" value="24"/><float name="fov" value="50"/>
        <transform name="toWorld"><lookat target="0, 0.5, 0" origin="0, 1, 4" up="0, 1, 0"/></transform></camera>
      <mesh type="obj"><string name="filename" value="floor.obj"/><bsdf type="diffuse"><color name="albedo" value="0.6,0.5,0.4"/></bsdf></mesh>
      <mesh type="obj"><string name="filename" value="light.obj"/><emitter type="area"><color name="radiance" value="8,8,8"/></emitter></mesh>
    </scene>""")
    r = renderer_factory(host.load_xml(str(tmp_path / "s.xml")), builder=2)
    rgbw, m2, _ = r.render_moments_host(spp_count=4)
    E = float(np.median(r.tile_errors(rgbw, m2)))
    want = r.render_allocated_host(E, pilot_spp=4, max_rounds=2)
    exe = os.path.join(_capi.LIB_DIR, "nori")
    p = subprocess.run([exe, str(tmp_path / "s.xml"), "--target-error", repr(E), "--allocate", "--pilot-spp", "4", "--rounds", "2"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    s = want["summary"]
    assert f"Stopped after {s['passes']} render calls (a pilot of 4 samples per pixel, at most 2 rounds)" in p.stdout, p.stdout
    assert f"{s['n_unconverged']} of {s['n_tiles']} tiles above the target" in p.stdout, p.stdout
    spp_map = read_exr_rgb(str(tmp_path / "s.spp.exr"))[1][..., 0]
    assert set(np.unique(spp_map).tolist()) <= {4.0, 8.0, 16.0, 32.0} and len(np.unique(spp_map)) >= 2      # only level values, and not one alone
    assert np.array_equal(spp_map, np.repeat(np.repeat(want["tile_spp"], 16, 0), 16, 1)[:24, :40].astype(F))
    assert np.array_equal(read_exr_rgb(str(tmp_path / "s.error.exr"))[1][..., 0], want["err"])
    from nori_amd.render import develop_host
    assert np.array_equal(read_exr_rgb(str(tmp_path / "s.exr"))[1], develop_host(want["rgbw"], r.border))
