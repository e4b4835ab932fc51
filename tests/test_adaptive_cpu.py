"""Adaptive sampling without a GPU: the numpy restatements of the tile errors and the selection (tests/adaptive_ref.py) on hand-made
frames, the resources of film_tiles.hip's kernels, the bindings and the command line."""
from __future__ import annotations

import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi
from tests import adaptive_ref as ar, moments_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

NEW_ENTRY_POINTS = ["nori_hip_render_tiles", "nori_hip_render_tiles_host", "nori_hip_tile_errors", "nori_hip_tile_errors_host",
                    "nori_hip_select_tiles", "nori_hip_render_adaptive", "nori_hip_render_adaptive_host"]


# ------------------------------------------------------------------ the restatement
def test_tree_sum_is_the_stated_tree():
    """lane t takes lane t + off, off = 128 .. 1: spelt out with Python floats (binary64) for one row, and against the exact sum
    within the bound of any summation order of 256 non-negative terms"""
    rng = np.random.default_rng(3)
    lanes = rng.uniform(0.0, 2.0, 256)
    s = [float(v) for v in lanes]
    off = 128
    while off:
        for t in range(off):
            s[t] = s[t] + s[t + off]
        off //= 2
    assert ar.tree_sum(lanes) == s[0]
    assert abs(s[0] - math.fsum(lanes)) <= 256 * 2.0 ** -53 * math.fsum(lanes)
    # the order matters in the last bits: the tree is not the sequential sum for every input, so a test against it is a test of the order
    seq = 0.0
    differs = False
    for seed in range(20):
        v = np.random.default_rng(seed).uniform(0.0, 2.0, 256)
        seq = 0.0
        for x in v:
            seq += float(x)
        differs |= seq != ar.tree_sum(v)
    assert differs


def test_tile_errors_partial_tiles_and_special_pixels():
    """45 x 37: 3 x 3 tiles, the right column 13 wide, the bottom row 5 high.  The mean is over the pixels inside the frame; the
    special pixels of moments_ref.hand_made_pair (W = 0, W < 0, negative variance, M = 0) contribute their err -- 0 --, and still count."""
    width, height, border = 45, 37, 2
    rgbw, m2 = ar.random_pair(width, height, border, seed=7)
    err, empty = mr.error_map(rgbw, m2, border)
    assert int(empty.sum()) >= 256 + 10                      # the empty tile and the scattered W <= 0 pixels
    te = ar.tile_errors(rgbw, m2, border)
    assert te.shape == (3, 3) and te.dtype == F
    pixels = ar.tile_pixels(width, height)
    assert pixels.tolist() == [[256, 256, 208], [256, 256, 208], [80, 80, 65]]
    for ty in range(3):
        for tx in range(3):
            blk = err[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].astype(np.float64)
            want = math.fsum(blk.reshape(-1)) / blk.size
            assert blk.size == pixels[ty, tx]
            # 256 terms in any order: within 256 2^-53 of the exact sum, then one rounding to float32
            assert abs(float(te[ty, tx]) - want) <= want * (256 * 2.0 ** -53 + 2.0 ** -24), (ty, tx)
    assert te[1, 1] == 0                                     # nothing but empty pixels
    assert (np.delete(te.reshape(-1), 4) > 0).all()
    # the hand-made pair of the error-map tests, 11 x 9: one partial tile
    rgbw, m2 = mr.hand_made_pair(border=2)
    err, empty = mr.error_map(rgbw, m2, 2)
    te = ar.tile_errors(rgbw, m2, 2)
    assert te.shape == (1, 1) and abs(float(te[0, 0]) - math.fsum(err.astype(np.float64).reshape(-1)) / 99) <= float(te[0, 0]) * 2.0 ** -23


def test_selection_keeps_order_and_nans():
    te = np.array([0.5, 0.1, np.nan, 0.3, 0.0, 0.3, np.inf, 0.2], F)
    every = np.arange(8, dtype=np.uint32)
    assert ar.select(te, 0.3, every).tolist() == [0, 2, 6]                 # 0.3 <= 0.3 retires; the NaN stays
    assert ar.select(te, 0.0, every).tolist() == [0, 1, 2, 3, 5, 6, 7]     # a target of 0 retires only an error of exactly 0
    assert ar.select(te, np.inf, every).tolist() == [2]                    # nothing but the NaN is above every target
    assert ar.select(te, 0.25, [1, 3, 7]).tolist() == [3]                  # a sub-list: only its members, in its order
    assert ar.select(te, 0.25, []).tolist() == []
    assert ar.select(te, -1.0, every).tolist() == every.tolist()


# ------------------------------------------------------------------ the new device source
@pytest.fixture(scope="module")
def tile_kernels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as ge
    from kernel_resources import kernels
    assert "film_tiles.hip" in ge.HIP_SOURCES
    out = tmp_path_factory.mktemp("asm") / "film_tiles.s"
    flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    p = subprocess.run([ge.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(ge.DEV, "film_tiles.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return {r["demangled"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: r for r in kernels(str(out))}


def test_tile_kernels_compile_without_scratch(tile_kernels):
    want = {"film_resolve_tiles_kernel", "film_tile_errors_kernel", "film_tile_select_count_kernel", "film_tile_select_scan_kernel",
            "film_tile_select_scatter_kernel", "film_tiles_add_spp_kernel"}
    assert set(tile_kernels) == want, sorted(tile_kernels)
    for name, k in tile_kernels.items():
        assert k["scratch"] == 0, (name, k)
    assert tile_kernels["film_tile_errors_kernel"]["lds"] == 256 * 8      # the 256 binary64 lanes of the tree, nothing else


# ------------------------------------------------------------------ bindings, command line
def test_capi_declares_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "nori_hip.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*|nori_hip_ctx \*)\s*(nori_hip_\w+)\(", header, re.M))
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
    assert declared <= set(_capi.HIP_PROTOTYPES), sorted(declared - set(_capi.HIP_PROTOTYPES))
    # nori_adaptive_summary: five uint32, then nori_error_summary at its 8-byte alignment
    import ctypes
    assert ctypes.sizeof(_capi.AdaptiveSummary) == 24 + ctypes.sizeof(_capi.ErrorSummary) and _capi.AdaptiveSummary.frame.offset == 24
    assert _capi.HIP_ABI_VERSION == 8 and "#define NORI_HIP_ABI_VERSION 8 " in header


def test_cli_rejects_adaptive_without_a_target(tmp_path):
    """before anything is loaded or a device is asked for: the scene file does not even exist"""
    exe = os.path.join(_capi.LIB_DIR, "nori")
    for args in (["--adaptive"], ["--adaptive", "--gpus", "1"]):
        p = subprocess.run([exe, str(tmp_path / "missing.xml")] + args, capture_output=True, text=True, timeout=120)
        out = p.stdout + p.stderr
        assert p.returncode != 0 and "Usage" in out and "--adaptive" in out and "--target-error" in out, out
        assert "missing.xml" not in out
    p = subprocess.run([exe, str(tmp_path / "missing.xml"), "--gpus", "2", "--target-error", "0.1", "--adaptive"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "one device" in p.stdout + p.stderr and "missing.xml" not in p.stdout + p.stderr
