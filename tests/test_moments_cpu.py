"""Second moments and the error map without a GPU: the numpy restatements the GPU tests lean on (tests/moments_ref.py)
against the oracle's splat and a binary64 evaluation, the registers of film.hip's kernels, and the command line."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi
from nori_amd.scene import RFilter
from tests import film_cases, moments_ref as mr
from tests.backends import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _positions(width, height, n=50, seed=11):
    """n frame positions: uniform ones, ones within 1e-3 of a pixel edge on either side, the frame's corners"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 1, (n, 2)) * (width, height)
    edge = np.floor(p[: n // 2]) + rng.choice([1e-3, 1e-4, 0.0, 1 - 1e-3, 1 - 1e-4], (n // 2, 2)) * rng.choice([1.0, 0.5], (n // 2, 2))
    p[: n // 2] = edge
    p[-4:] = [(0.0, 0.0), (width - 1e-3, height - 1e-3), (0.25, height - 0.5), (width - 0.5, 1e-3)]
    return np.clip(p, 0, (np.nextafter(np.float32(width), 0), np.nextafter(np.float32(height), 0))).astype(np.float32)


@pytest.mark.parametrize("rfilter", [RFilter("gaussian"), RFilter("tent"), RFilter("gaussian", radius=5.2, stddev=1.3), RFilter("mitchell", radius=4.0),
                                     RFilter("box")], ids=lambda f: f"{f.type}-{f.radius}")
def test_restated_weights_are_the_oracles_splat(rfilter):
    """One sample at a time into a zeroed frame of one block (31 x 29 <= 32 x 32, so block and frame coordinates agree): the
    W channel ImageBlock::put leaves is float32(wx wy) of the restatement bit for bit, at every pixel."""
    width, height = 31, 29
    o = Oracle(film_cases.cornell(width, height, 1, rfilter))
    table, radius = o.filter_table(), mr.filter_radius(rfilter)
    assert o.border == mr.border_of(radius)
    touched = 0
    for p in _positions(width, height):
        got = o.splat(p[None], np.ones((1, 3), np.float32))[..., 3]
        x0, y0, w = mr.sample_weights(p, width, height, radius, table)
        want = np.zeros_like(got)
        want[y0:y0 + w.shape[0], x0:x0 + w.shape[1]] = w
        assert np.array_equal(got, want), p
        touched += w.size
    assert touched >= 50
    o.close()


def test_restated_error_map_against_binary64():
    rgbw, m2 = mr.hand_made_pair()
    err, empty = mr.error_map(rgbw, m2, 2)
    ref = mr.error_map_f64(rgbw, m2, 2)
    assert err.dtype == np.float32 and err.shape == (9, 11) and np.isfinite(err).all() and (err >= 0).all()
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    worst = float((np.abs(err.astype(np.float64) - ref) / ulp).max())
    print(f"[error map] float32 restatement against binary64: worst {worst:.2f} ulps")
    assert worst <= 4.0
    # the special pixels: W = 0 (twice) and W < 0 are empty with err 0; a variance below zero clamps, M = 0 and sum w^2 = 0 give 0
    assert int(empty.sum()) == 3 and not err[empty].any()
    assert err[3, 4] == 0 and err[4, 5] == 0 and err[5, 6] == 0 and not empty[3:6].any()
    assert err[6, 7] > 0 and err[7, 1] > 0
    s = mr.summary(err, empty, 0.1)
    assert s["n_pixels"] == 99 and s["n_empty"] == 3 and 0 < s["n_above"] < 99


@pytest.fixture(scope="module")
def film_kernels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as ge
    from kernel_resources import kernels
    out = tmp_path_factory.mktemp("asm") / "film.s"
    flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    p = subprocess.run([ge.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(ge.DEV, "film.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return {r["demangled"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: r for r in kernels(str(out))}


# film.hip's kernels as they compiled before the film kept moments: (VGPRs, SGPRs, scratch bytes, static LDS bytes)
BEFORE = {
    "film_gather_kernel": (75, 84, 0, 136),
    "film_gather_strips_kernel<2, 4, 128, 21>": (94, 45, 0, 136),
    "film_gather_strips_kernel<1, 3, 128, 38>": (73, 45, 0, 136),
    "film_resolve_kernel": (20, 48, 0, 0),
    "film_block_reference_kernel": (53, 79, 0, 132),
    "film_block_reference_staged_kernel": (80, 89, 0, 144),
    "film_resolve_reference_kernel": (24, 37, 0, 65536),
}
NEW = ["film_gather_m2_kernel", "film_gather_strips_m2_kernel<2, 4, 128, 21>", "film_gather_strips_m2_kernel<1, 3, 128, 38>",
       "film_error_map_kernel", "film_error_reduce_kernel"]


def test_plain_renders_run_the_kernels_of_before(film_kernels):
    """A render without moments launches the same kernels with the same resources; the moments forms are kernels of their own,
    without scratch and within the registers of the forms they mirror."""
    rows = film_kernels
    assert set(rows) == set(BEFORE) | set(NEW), sorted(rows)
    for name, want in BEFORE.items():
        k = rows[name]
        assert (k["vgpr"], k["sgpr"], k["scratch"], k["lds"]) == want, (name, k)
    for name in NEW:
        assert rows[name]["scratch"] == 0, rows[name]
    for plain, m2 in (("film_gather_kernel", "film_gather_m2_kernel"),
                      ("film_gather_strips_kernel<2, 4, 128, 21>", "film_gather_strips_m2_kernel<2, 4, 128, 21>"),
                      ("film_gather_strips_kernel<1, 3, 128, 38>", "film_gather_strips_m2_kernel<1, 3, 128, 38>")):
        assert rows[m2]["vgpr"] <= rows[plain]["vgpr"] and rows[m2]["lds"] <= rows[plain]["lds"], (rows[plain], rows[m2])


@pytest.mark.parametrize("args", [["--target-error", "x"], ["--target-error", "-0.5"], ["--target-error"], ["--target-error", "0.1", "--pass-spp", "0"],
                                  ["--target-error", "0.1", "--pass-spp", "4k"], ["--pass-spp", "4"]], ids=lambda a: " ".join(a))
def test_cli_rejects_bad_target_error_arguments(tmp_path, args):
    """before anything is loaded or a device is asked for: the scene file does not even exist"""
    exe = os.path.join(_capi.LIB_DIR, "nori")
    p = subprocess.run([exe, str(tmp_path / "missing.xml")] + args, capture_output=True, text=True, timeout=120)
    out = p.stdout + p.stderr
    assert p.returncode != 0 and "Usage" in out and ("--target-error" in out or "--pass-spp" in out), out
    assert "missing.xml" not in out


def test_cli_target_error_refuses_several_gpus(tmp_path):
    exe = os.path.join(_capi.LIB_DIR, "nori")
    p = subprocess.run([exe, str(tmp_path / "missing.xml"), "--gpus", "2", "--target-error", "0.1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "one device" in p.stdout + p.stderr and "missing.xml" not in p.stdout + p.stderr
