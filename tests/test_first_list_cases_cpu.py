"""The cases of tests/first_list_cases.py that tests/test_first_lists_cpu.py does not already run -- cameras that are no rigid lookat,
an ill-conditioned one, scaled scenes, odd and one-tile frames, a root that is a leaf, slivers, coplanar duplicates -- through the CPU
harness (tests/first_lists/harness.cpp): for every tile with a list, every ray of the harness's deterministic set must find its hit in
the list, and the list must return the walk's (t, u, v, triangle) bit for bit, with every ray also held to the linear scan.

At the largest K a case must not pass by leaving everything out: a "lists" case has a list for at least half its tiles under the
device builders' tree and rays that hit; an "all-overflow" case has no list at all."""
import pytest

from tests import first_list_cases as flc
from tests.test_first_lists_cpu import DEFAULT_K, MAX_K, OVERFLOW, Harness, assert_superset, lib      # noqa: F401 (lib: the fixture)


@pytest.mark.parametrize("builder", [0, 1])
@pytest.mark.parametrize("key", flc.NEW_KEYS)
def test_case_lists_hold_every_hit(lib, key, builder):
    sc, expect = flc.case(key), flc.EXPECT[key]
    n_tiles = flc.n_tiles(key)
    h = Harness(lib, sc, builder=builder)
    try:
        assert h.n_tiles == n_tiles
        for K in (2, DEFAULT_K, MAX_K):
            r = h.check(K, per_pixel=4, scan_every=1)
            assert_superset(r, f"{key} builder {builder} K {K}")
            assert r["list_tiles"] + r["overflow_tiles"] == n_tiles
            if K != MAX_K:
                continue
            if expect == "lists" and builder == 1:
                assert r["list_tiles"] >= (n_tiles + 1) // 2 and r["hits"] > 0, (key, r)
            elif expect == "lists":
                assert r["list_tiles"] > 0, (key, r)
            else:      # "all-overflow": first_camera's ok = 0; "walk": the root is a leaf, which first_camera refuses as well
                assert r["list_tiles"] == 0 and r["rays"] == 0, (key, r)
                assert (h.lists(K)[0] == OVERFLOW).all()
    finally:
        h.close()


@pytest.mark.parametrize("builder", [0, 1])
def test_unbounded_boxes_do_not_widen_the_pad(lib, builder):
    """Numerically collinear triangles get unbounded boxes (h = kBoxHalfInf = 2^59, a finite number).  first_root_diagonal must skip
    them: pad_abs is kBoxPadRel (2e-6) x the diagonal of the FINITE part of the scene -- the wall, 8 x 8, and the filler in front of
    it: less than 20 -- and the tiles' lists are culled as the base scene's are.  (A diagonal of 1e18 gave a pad of 4e12, under which
    every tile listed every pair record of the tree.)"""
    h = Harness(lib, flc.case("slivers"), builder=builder)
    try:
        ok, m = h.margin(0, 0)
        assert ok == 3 and 0.0 < m["pad_abs"] < 2e-6 * 20.0, m
        count, _ = h.lists(MAX_K)
        assert (count != OVERFLOW).all() and (count < h.info()["n_pairs"]).all(), count      # every tile culls something
    finally:
        h.close()


def test_ill_conditioned_camera_is_refused_by_kappa(lib):
    """L diag(1, 1, 1e-7): first_camera computes kappa >= 1e6 and gives ok = 0 (bit 0 of fl_margin's flags), the base camera ok = 1"""
    for key, want in (("ill-conditioned", 0), ("base", 1)):
        h = Harness(lib, flc.case(key))
        try:
            assert h.margin(0, 0)[0] & 1 == want, key
        finally:
            h.close()

