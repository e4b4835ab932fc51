"""The allocation of sample levels without a GPU: the properties of the restatement (tests/allocate_ref.py) on made-up arrays, the
resources of film_alloc.hip's kernels, the bindings and the command line."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nori_amd import _capi
from tests import allocate_ref as al

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ------------------------------------------------------------------ the levels
def test_levels_follow_the_budget():
    assert al.levels(8, 64) == [8, 16, 32, 64]
    assert al.levels(8, 127) == [8, 16, 32, 64]                  # floor(log2(127 / 8)) = 3
    assert al.levels(8, 8) == [8] and al.levels(8, 15) == [8]    # one level: nothing can move
    assert al.levels(2, 1 << 20) == [2 << j for j in range(8)]   # J stops at 7
    assert al.levels(16, 256) == [16, 32, 64, 128, 256]
    for J in range(8):
        ps = al.pairs(J)
        assert len(ps) == J * (J + 1) // 2 <= al.MAX_BUCKETS
        assert [al.bucket_of(J, i, j) for i, j in ps] == list(range(len(ps)))      # ascending in i, then j


# ------------------------------------------------------------------ the rule on made-up arrays
def _scalar_rule(E, target, headroom, spp, l):
    """the rule for one tile in Python scalars of float32: (level, done)"""
    E, target, headroom = F(E), F(target), F(headroom)
    J = len(spp) - 1
    with np.errstate(all="ignore"):
        if E <= target:
            return l, True
        r = F(E / target)
        need = F(F(headroom * F(spp[l])) * F(r * r))
        j = l
        while j < J and not (F(spp[j]) >= need):
            j += 1
    return j, j == l


def _made_up(n, seed, J):
    rng = np.random.default_rng(seed)
    e = rng.uniform(0.0, 0.6, n).astype(F)
    e[rng.integers(0, n, n // 10)] = F(0.1)                                                             # equal to the target
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, 1e-30], F)
    e[rng.choice(n, special.size, replace=False)] = special
    return e, rng.integers(0, J + 1, n).astype(np.uint32), (rng.uniform(0, 1, n) < 0.2).astype(np.uint32)


@pytest.mark.parametrize("headroom", [1.0, 1.5])
@pytest.mark.parametrize("target", [0.1, 0.0, 0.25])
def test_the_vectorised_rule_is_the_scalar_rule_and_has_its_properties(target, headroom):
    spp = al.levels(8, 256)
    J = len(spp) - 1
    e, level, done = _made_up(700, 3, J)
    new_level, new_done, bucket = al.classify(e, target, headroom, spp, level, done)
    for t in range(e.size):
        if done[t]:
            want = (int(level[t]), True, al.STAYS)
        else:
            j, stop = _scalar_rule(e[t], target, headroom, spp, int(level[t]))
            want = (int(level[t]) if stop else j, stop, al.STAYS if stop else al.bucket_of(J, int(level[t]), j))
        assert (int(new_level[t]), bool(new_done[t]), int(bucket[t])) == want, (t, e[t], level[t], done[t])
    assert (new_level >= level).all() and (new_level <= J).all()                       # levels never fall
    assert (new_done >= done).all()                                                    # a done tile never returns
    moved = new_level != level
    with np.errstate(invalid="ignore"):
        assert not (moved & (e <= F(target))).any() and not (moved & (done != 0)).any()      # a tile moves only when E > target (or NaN) and it is live
    assert ((bucket != al.STAYS) == moved).all() and moved.any() and not moved.all()
    nan = np.isnan(e) & (done == 0)
    assert (new_level[nan] == J).all()                                                 # a NaN goes to the top
    if target == 0.0:
        with np.errstate(invalid="ignore"):
            up = (done == 0) & ~(e <= 0)
        assert (new_level[up] == J).all()                                              # target 0: everything above zero goes to the top
    tile_spp = np.asarray(spp)[new_level]
    assert set(tile_spp.tolist()) <= set(spp)                                          # tile_spp stays within the levels


def test_headroom_raises_levels_and_never_lowers_one():
    spp = al.levels(8, 256)
    e, level, done = _made_up(700, 4, len(spp) - 1)
    a, _, _ = al.classify(e, 0.1, 1.0, spp, level, done)
    b, _, _ = al.classify(e, 0.1, 2.0, spp, level, done)
    assert (b >= a).all() and (b > a).any()


@pytest.mark.parametrize("n", [9, 300, 70000])
def test_buckets_partition_the_movers(n):
    spp = al.levels(8, 1024)
    J = len(spp) - 1
    e, level, done = _made_up(n, n, J)
    new_level, new_done, tiles, begin = al.allocate(e, 0.1, 1.0, spp, level, done)
    moved = np.flatnonzero(new_level != level)
    assert begin.size == al.MAX_BUCKETS + 1 and begin[0] == 0 and (np.diff(begin.astype(np.int64)) >= 0).all() and begin[-1] == tiles.size
    assert sorted(tiles.tolist()) == moved.tolist()                                    # every mover once, nothing else
    for (i, j) in al.pairs(J):
        b = al.bucket_of(J, i, j)
        part = tiles[begin[b]:begin[b + 1]]
        assert (np.diff(part.astype(np.int64)) > 0).all()                              # ascending id inside a pair
        assert (level[part] == i).all() and (new_level[part] == j).all()
    assert (begin[J * (J + 1) // 2:] == tiles.size).all()


def test_the_loop_over_callbacks_stops_and_logs():
    """a made-up world: the error of a tile falls as c_t / sqrt(spp)"""
    spp = al.levels(8, 64)
    c = np.array([0.1, 0.3, 0.5, 2.0, np.nan, 0.0], F)
    got = np.zeros(c.size, np.int64)

    def render(tiles, lo, hi):
        got[slice(None) if tiles is None else tiles] += hi - lo

    evaluate = lambda live: (c / np.sqrt(np.maximum(got, 1).astype(F))).astype(F)
    log, done, passes, calls = al.loop(c.size, spp, 0.1, 1.0, 3, render, evaluate)
    assert log.shape == (4, c.size) and (np.diff(log.astype(np.int64), axis=0) >= 0).all() and (log[0] == 0).all()
    assert got.tolist() == [spp[l] for l in log[-1]]                                   # every tile received exactly its level's samples
    assert log[-1].tolist() == [0, 1, 2, 3, 3, 0] and done.all() and passes == len(calls)
    for k in range(1, 4):
        moves = al.moves_of_log(log, k, len(spp) - 1)
        assert all((log[k - 1][t] == i).all() and (log[k][t] == j).all() for t, i, j in moves)
    one = al.loop(c.size, spp, 0.1, 1.0, 1, lambda *a: None, evaluate)
    assert one[0].shape == (2, c.size)


# ------------------------------------------------------------------ the new device source
@pytest.fixture(scope="module")
def alloc_kernels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as ge
    from kernel_resources import kernels
    assert "film_alloc.hip" in ge.HIP_SOURCES
    res = {}
    for tag, extra in (("product", []), ("count", ["-DNORI_COUNT_EXCURSIONS=1"])):
        out = tmp_path_factory.mktemp("asm") / f"film_alloc_{tag}.s"
        flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")] + extra
        p = subprocess.run([ge.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(ge.DEV, "film_alloc.hip"), "-o", str(out)],
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        res[tag] = {r["demangled"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: r for r in kernels(str(out))}
    return res


def test_alloc_kernels_have_no_scratch(alloc_kernels):
    # LDS: four 64-bit words of packed counters per lane of a block, or the 256 run sums of the scan
    want = {"film_alloc_classify_kernel": 0, "film_alloc_count_kernel": 8192, "film_alloc_scan_kernel": 1024, "film_alloc_scatter_kernel": 8192,
            "film_alloc_inverse_kernel": 0, "film_alloc_tile_spp_kernel": 0}
    for tag, ks in alloc_kernels.items():
        assert set(ks) == set(want), (tag, sorted(ks))
        for name, k in ks.items():
            assert k["scratch"] == 0 and k["vgpr"] <= 64 and k["lds"] == want[name], (tag, name, k)


# ------------------------------------------------------------------ bindings, command line
NEW = ("nori_hip_allocate_tiles", "nori_hip_render_allocated", "nori_hip_render_allocated_host")


def test_capi_declares_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "nori_hip.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*|nori_hip_ctx \*)\s*(nori_hip_\w+)\(", header, re.M))
    lib = _capi.load_hip()
    for name in NEW:
        assert name in declared and name in _capi.HIP_PROTOTYPES and hasattr(lib, name), name
    assert declared <= set(_capi.HIP_PROTOTYPES)
    assert _capi.HIP_ABI_VERSION == 8 and "#define NORI_HIP_ABI_VERSION 8 " in header and lib.nori_hip_abi_version() == 8
    for name in NEW:      # the prototypes have the arity of the declarations
        decl = re.search(r"^int " + name + r"\((.*?)\);", header, re.M | re.S).group(1)
        n_args = len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(","))
        assert n_args == len(_capi.HIP_PROTOTYPES[name][1]), (name, n_args)
    from nori_amd.render import Renderer
    for name in ("allocate_tiles", "render_allocated_host", "render_allocated_denoised_host", "allocate_levels"):
        assert callable(getattr(Renderer, name)), name
    assert Renderer.allocate_levels(8, 64) == al.levels(8, 64) and Renderer.allocate_levels(2, 1 << 20) == al.levels(2, 1 << 20)


def test_allocate_params_marshal_as_the_header_lays_them_out():
    header = open(os.path.join(ROOT, "include", "nori_hip.h")).read()
    body = re.search(r"typedef struct nori_allocate_params \{(.*?)\} nori_allocate_params;", header, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|int32_t|float)\s+(\w+);", body, re.M)
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(_capi.AllocateParams._fields_)
    assert ctypes.sizeof(_capi.AllocateParams) == 20
    ap = _capi.AllocateParams(8, 3, 0.05, 1.5, 1)
    raw = np.frombuffer(bytes(ap), np.uint32)
    assert raw[:2].tolist() == [8, 3] and raw[2:4].view(np.float32).tolist() == [F(0.05), F(1.5)] and raw[4] == 1
    assert _capi.ALLOC_MAX_BUCKETS == al.MAX_BUCKETS == 28 and _capi.ALLOC_MAX_LEVEL == al.MAX_LEVEL


def test_cli_takes_allocate_as_a_modifier_only(tmp_path):
    """before anything is loaded or a device is asked for: the scene file does not even exist"""
    exe = os.path.join(_capi.LIB_DIR, "nori")
    scene = str(tmp_path / "missing.xml")
    for args, words in ((["--allocate"], ("--allocate", "--target-error E or --target-denoised-error E")),
                        (["--target-error", "0.05", "--adaptive", "--allocate"], ("--allocate", "--adaptive")),
                        (["--target-error", "0.05", "--allocate", "--gpus", "2"], ("--allocate", "one device")),
                        (["--target-denoised-error", "0.05", "--allocate", "--gpus", "2"], ("one device",)),
                        (["--target-error", "0.05", "--pilot-spp", "8"], ("--pilot-spp", "goes with --allocate")),
                        (["--target-error", "0.05", "--rounds", "2"], ("--rounds", "goes with --allocate")),
                        (["--target-error", "0.05", "--allocate", "--pilot-spp", "1"], ("--pilot-spp", ">= 2")),
                        (["--target-error", "0.05", "--allocate", "--pilot-spp", "x"], ("--pilot-spp", ">= 2")),
                        (["--target-error", "0.05", "--allocate", "--rounds", "0"], ("--rounds", ">= 1")),
                        (["--target-error", "0.05", "--allocate", "--rounds"], ("--rounds", ">= 1"))):
        p = subprocess.run([exe, scene] + args, capture_output=True, text=True, timeout=120)
        out = p.stdout + p.stderr
        assert p.returncode != 0 and "Usage" in out and "missing.xml" not in out, (args, out)
        for word in words:
            assert word in out, (args, out)
    for args in (["--target-error", "0.05", "--allocate"], ["--target-error", "0.05", "--allocate", "--pilot-spp", "8", "--rounds", "2"],
                 ["--target-denoised-error", "0.02", "--allocate", "--pilot-spp", "4", "--feature-spp", "3"]):
        p = subprocess.run([exe, scene] + args, capture_output=True, text=True, timeout=120)      # accepted: the scene is then opened, and is missing
        assert p.returncode != 0 and "Usage" not in p.stdout + p.stderr and "missing.xml" in p.stdout + p.stderr, args
