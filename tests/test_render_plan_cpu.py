"""The host-side arithmetic of a render call (nori_amd/csrc/device/render_plan.h: tile geometry, the megakernel's chunk plan and sample
cut, the wavefront engine's memory budget and its out-of-memory ladder) on the CPU, through tests/render_plan/harness.cpp -- a
stand-alone program built here with g++, once plain and once with -fsanitize=address,undefined, and run as a process of its own.

The expected values come from the functions below: the arithmetic as render_impl had it inline before it was split out (integer
operations restated line by line, uint32_t / size_t as Python ints -- the cases stay inside both), not from the header.  The budget
and the ladder decide how a frame is cut into batches, hence its bits: on a GPU only tests/test_gpu_wavefront.py reaches them, through
NORI_HIP_WF_IGNORE_FREE."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "render_plan", "harness.cpp")
CXXFLAGS = ["-std=c++17", "-Wall", "-Wextra"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]}
PER_PATH, PER_SAMPLE = 216, 20      # anything fixed will do: the real ones come from wavefront_bytes_per_* at run time
K = 1 << 20


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("render_plan")
    procs = {name: subprocess.Popen(["g++"] + CXXFLAGS + flags + ["-o", str(d / name), SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for name, flags in BUILDS.items()}
    out = {}
    for name, p in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, log
        out[name] = str(d / name)
    return out


def run(program, tmp_path, cases):
    """one process for all cases (the sanitizers' runtime is linked into the program statically): a list of integers per case"""
    path = tmp_path / "cases"
    path.write_text("".join(" ".join(str(x) for x in c) + "\n" for c in cases))
    p = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == len(cases)
    return [line.split() for line in lines]


# ---- the arithmetic as render_impl had it inline

def geometry(width, height, tile_mod, tile_rem, border):
    tiles_x, tiles_y = (width + 16 - 1) // 16, (height + 16 - 1) // 16
    n_tiles = tiles_x * tiles_y
    n_sel = (n_tiles - tile_rem + tile_mod - 1) // tile_mod if n_tiles > tile_rem else 0
    return [tiles_x, tiles_y, n_sel, 16 + 2 * border]


def chunks(n_sel_tiles, spp_count, target_wgs):
    n_chunks = 1
    if 0 < n_sel_tiles < target_wgs:
        n_chunks = (target_wgs + n_sel_tiles - 1) // n_sel_tiles
    n_chunks = max(1, min(n_chunks, max(1, spp_count // 8)))
    chunk_spp = (spp_count + n_chunks - 1) // max(1, n_chunks)
    if chunk_spp == 0:
        chunk_spp = 1
    return [max(1, (spp_count + chunk_spp - 1) // chunk_spp), chunk_spp]


def cut(spp_count, n_sel_tiles, cap):
    return [max(1, min(spp_count, cap // (n_sel_tiles * 256)))]


def budget(call_samples, opt_paths, opt_samples, reference, usable):
    want = call_samples if reference else opt_samples if opt_samples else opt_paths
    max_samples = max(256, min(want, call_samples))
    max_paths = max(256, min(opt_paths, max_samples))
    if usable is not None and max_paths * PER_PATH + max_samples * PER_SAMPLE > usable:
        if reference:
            max_paths = max(256, (usable - max_samples * PER_SAMPLE) // PER_PATH if usable > max_samples * PER_SAMPLE else 0)
        elif usable >= max_paths * (PER_PATH + 4 * PER_SAMPLE):
            max_samples = (usable - max_paths * PER_PATH) // PER_SAMPLE
        else:
            max_paths = max(256, usable // (PER_PATH + 4 * PER_SAMPLE))
            max_samples = min(max_samples, 4 * max_paths)
    return [max_paths, max_samples]


def ladder(max_paths, max_samples, reference):
    """the pairs the retry loop went through until it broke off"""
    rungs = []
    while True:
        pool_bigger = max_paths * PER_PATH >= max_samples * PER_SAMPLE or reference
        if pool_bigger and max_paths > K:
            max_paths //= 2
        elif reference:
            break
        elif max_samples > K:
            max_samples //= 2
            max_paths = min(max_paths, max_samples)
        elif max_paths > K:
            max_paths //= 2
        else:
            break
        rungs.append((max_paths, max_samples))
        assert len(rungs) < 200
    return rungs


def budget_case(call_samples, opt_paths, opt_samples, reference, usable):
    return ["budget", call_samples, opt_paths, opt_samples, int(reference), PER_PATH, PER_SAMPLE, -1 if usable is None else usable]


AMPLE = 1 << 38
NEED = (1 << 22) * PER_PATH + (1 << 28) * PER_SAMPLE      # a pool of 2^22 paths, batches of 2^28 samples
BUDGETS = {
    "headline": ((1 << 28, 1 << 29, 0, False, AMPLE), [1 << 28, 1 << 28]),
    "no samples": ((0, 1 << 29, 0, False, AMPLE), [256, 256]),
    "100 samples": ((100, 1 << 29, 0, False, AMPLE), [256, 256]),
    "samples below paths": ((1 << 28, 1 << 22, 1 << 20, False, AMPLE), [1 << 20, 1 << 20]),
    "just below the need": ((1 << 30, 1 << 22, 1 << 28, False, NEED - 1), [1 << 22, (1 << 28) - 1]),
    "the need exactly": ((1 << 30, 1 << 22, 1 << 28, False, NEED), [1 << 22, 1 << 28]),
    "far below the need": ((1 << 30, 1 << 29, 0, False, 1 << 26), None),
    "so far below that the pool is the floor": ((1 << 30, 1 << 29, 0, False, 1000), [256, 1024]),
    "reference, enough": ((1 << 24, 1 << 29, 1 << 20, True, AMPLE), [1 << 24, 1 << 24]),
    "reference, too little for the pool": ((1 << 24, 1 << 29, 0, True, (1 << 24) * PER_SAMPLE + 1000 * PER_PATH + 5), [1000, 1 << 24]),
    "reference, less than the batch needs": ((1 << 24, 1 << 29, 0, True, (1 << 24) * PER_SAMPLE - 1), [256, 1 << 24]),
    "reference, exactly the batch": ((1 << 24, 1 << 29, 0, True, (1 << 24) * PER_SAMPLE), [256, 1 << 24]),
    "unknown": ((1 << 30, 1 << 29, 0, False, None), [1 << 29, 1 << 29]),
    "unknown, both options": ((1 << 30, 1 << 22, 1 << 28, False, None), [1 << 22, 1 << 28]),
}


@pytest.mark.parametrize("build", list(BUILDS))
def test_wavefront_budget(programs, tmp_path, build):
    names = list(BUDGETS)
    got = run(programs[build], tmp_path, [budget_case(*BUDGETS[n][0]) for n in names])
    for name, g in zip(names, got):
        args, literal = BUDGETS[name]
        paths, samples = (int(x) for x in g)
        assert [paths, samples] == budget(*args), name
        if literal is not None:
            assert [paths, samples] == literal, name
        assert paths >= 256 and samples >= 256 and (args[3] or paths <= samples), name      # (reference order: the pool need not hold the batch)
    far = [int(x) for x in got[names.index("far below the need")]]
    assert far[0] == (1 << 26) // (PER_PATH + 4 * PER_SAMPLE) and far[0] < 1 << 29 and far[1] <= 4 * far[0] and far[1] < 1 << 29      # both shrink
    kept = [int(x) for x in got[names.index("just below the need")]]
    assert kept[0] == 1 << 22 and kept[1] < 1 << 28      # the pool is kept, the samples are cut


LADDERS = [(1 << 29, 1 << 29), (1 << 22, 1 << 28), (1 << 20, 1 << 20)]


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("reference", [False, True], ids=["fast", "reference"])
def test_out_of_memory_ladder(programs, tmp_path, build, reference):
    got = run(programs[build], tmp_path, [["ladder", p, s, int(reference), PER_PATH, PER_SAMPLE] for p, s in LADDERS])
    for (p0, s0), g in zip(LADDERS, got):
        assert g[-1] == "end", "the ladder does not end"
        nums = [int(x) for x in g[:-1]]
        rungs = list(zip(nums[0::2], nums[1::2]))
        assert rungs == ladder(p0, s0, reference), (p0, s0)
        prev = (p0, s0)
        for paths, samples in rungs:
            if samples == prev[1]:      # a rung that halves the pool: the batches, hence the frame's bits, stay
                assert paths == prev[0] // 2
            else:                       # a rung that halves the samples
                assert not reference and samples == prev[1] // 2 and paths <= samples
            assert paths >= K // 2 and samples >= K // 2
            prev = (paths, samples)
        if reference:
            assert all(s == s0 for _, s in rungs)
    # the sequences themselves, written out once: the pool goes first while it is the bigger
    assert ladder(1 << 29, 1 << 29, False)[:5] == [(1 << 28, 1 << 29), (1 << 27, 1 << 29), (1 << 26, 1 << 29), (1 << 25, 1 << 29), (1 << 25, 1 << 28)]
    assert ladder(1 << 22, 1 << 28, True) == [(1 << 21, 1 << 28), (1 << 20, 1 << 28)]
    assert ladder(1 << 20, 1 << 20, False) == [] and ladder(1 << 20, 1 << 20, True) == []
    assert ladder(1 << 22, 1 << 28, False)[-1] == (K, K)


CHUNKS = [(4096, 256, 16384), (1, 256, 16384), (20000, 256, 16384), (4096, 7, 16384), (4096, 0, 16384), (0, 256, 16384), (0, 0, 16384),
          (4096, 256, 1), (1, 256, 1), (16383, 9, 16384), (16384, 256, 16384), (3, 1000, 16384)]
CUTS = [(256, 4096, 1 << 29), (256, 4096, 256), (256, 4096, 4096 * 256 * 3), (256, 4096, 4096 * 256 * 3 - 1), (256, 4096, 4096 * 256 * 256),
        (256, 4096, 4096 * 256 * 257), (1, 1, 256), (0, 4096, 1 << 29)]


@pytest.mark.parametrize("build", list(BUILDS))
def test_chunk_plan_and_sample_cut(programs, tmp_path, build):
    got = run(programs[build], tmp_path, [["chunks", *c] for c in CHUNKS] + [["cut", *c] for c in CUTS])
    got = [[int(x) for x in g] for g in got]
    for c, g in zip(CHUNKS, got):
        assert g == chunks(*c), c
        n_chunks, chunk_spp = g
        assert n_chunks >= 1 and chunk_spp >= 1 and n_chunks * chunk_spp >= c[1] and (n_chunks - 1) * chunk_spp < max(c[1], 1)      # the chunks cover the samples, none is empty
    assert got[0] == [4, 64]                     # 4096 tiles x 256 spp: 4 chunks of 64
    assert got[4] == [1, 1]                      # no samples: chunk_spp 1, one chunk
    assert got[7] == [1, 256] and got[8] == [1, 256]      # target_wgs 1
    for c, g in zip(CUTS, got[len(CHUNKS):]):
        assert g == cut(*c), c
    cuts = [g[0] for g in got[len(CHUNKS):]]
    assert cuts[:6] == [256, 1, 3, 2, 256, 256]      # one launch; 1 spp per launch; cap exactly tiles * 256 * k, and one sample less


GEOMETRY = [(1, 1, 1, 0, 0), (16, 16, 1, 0, 1), (17, 33, 1, 0, 2), (17, 33, 3, 0, 8), (17, 33, 3, 1, 0), (17, 33, 3, 2, 0), (17, 33, 7, 5, 0),
            (17, 33, 7, 6, 0), (17, 33, 8, 6, 0), (17, 33, 8, 7, 0), (1024, 1024, 1, 0, 1), (1024, 1024, 4096, 4095, 1), (1024, 1024, 5000, 4096, 1)]


@pytest.mark.parametrize("build", list(BUILDS))
def test_tile_geometry(programs, tmp_path, build):
    got = run(programs[build], tmp_path, [["geo", *c] for c in GEOMETRY])
    got = [[int(x) for x in g] for g in got]
    for c, g in zip(GEOMETRY, got):
        assert g == geometry(*c), c
    assert got[0] == [1, 1, 1, 16] and got[1] == [1, 1, 1, 18] and got[2] == [2, 3, 6, 20]
    assert [g[2] for g in got[3:6]] == [2, 2, 2] and sum(g[2] for g in got[3:6]) == 6      # tile_mod 3: every tile in exactly one share
    assert [g[2] for g in got[6:10]] == [1, 0, 0, 0]      # tile_rem on and past the last tile
    assert got[10][:3] == [64, 64, 4096] and got[11][2] == 1 and got[12][2] == 0
