"""Restatement in numpy of the allocation of sample levels (include/nori_hip.h: nori_hip_allocate_tiles, nori_hip_render_allocated):
the rule, the grouping of the moving tiles by pair, and the loop over callbacks that render and evaluate -- for
tests/test_allocate_cpu.py, which checks its properties on made-up arrays, and tests/test_gpu_allocate.py, which holds the device to
it bit for bit.  Tile errors come from tests/adaptive_ref.py (raw) and tests/denoise_error_ref.py (denoised).

    spp_j = pilot_spp << j, j = 0 .. J, J = min(7, floor(log2(spp_count / pilot_spp)))
    per tile not done, float32:  if E <= target: done
                                 else r = E / target; need = (headroom * float(spp_l)) * (r * r)
                                      j = l; while j < J and not (float(spp_j) >= need): j += 1
                                      if j == l: done  else: l -> j
    bucket of a move (i, j), i < j:  b = i J - i (i - 1) / 2 + (j - i - 1)
"""
from __future__ import annotations

import numpy as np

F = np.float32
MAX_LEVEL = 7
MAX_BUCKETS = MAX_LEVEL * (MAX_LEVEL + 1) // 2
STAYS = 0xFFFFFFFF


def levels(pilot_spp, spp_count):
    """[spp_0, ..., spp_J]"""
    assert pilot_spp >= 2 and spp_count >= pilot_spp
    J = 0
    while J < MAX_LEVEL and (pilot_spp << (J + 1)) <= spp_count:
        J += 1
    return [pilot_spp << j for j in range(J + 1)]


def pairs(J):
    """the pairs (i, j), i < j <= J, in bucket order"""
    return [(i, j) for i in range(J) for j in range(i + 1, J + 1)]


def bucket_of(J, i, j):
    return i * J - i * (i - 1) // 2 + (j - i - 1)


def classify(tile_err, target, headroom, spp, level, done):
    """one round: (new level, new done, bucket per tile or STAYS).  Every operation is a float32 operation of its own."""
    e = np.asarray(tile_err, F).reshape(-1)
    level = np.array(level, np.uint32).reshape(-1)
    done = (np.array(done).reshape(-1) != 0).astype(np.uint32)
    J = len(spp) - 1
    table = np.asarray(spp, np.uint32)
    target, headroom = F(target), F(headroom)
    live = done == 0
    with np.errstate(all="ignore"):
        below = live & (e <= target)
        moving = live & ~below
        r = (e / target).astype(F)
        need = ((headroom * table[level].astype(F)).astype(F) * (r * r).astype(F)).astype(F)
        j = level.copy()
        for _ in range(J):      # while j < J and not (float(spp_j) >= need): j += 1
            step = moving & (j < J) & ~(table[np.minimum(j, J)].astype(F) >= need)
            j = np.where(step, j + 1, j).astype(np.uint32)
    stops = below | (moving & (j == level))
    moves = moving & (j != level)
    bucket = np.full(e.size, STAYS, np.uint32)
    li, lj = level[moves].astype(np.int64), j[moves].astype(np.int64)
    bucket[moves] = (li * J - li * (li - 1) // 2 + (lj - li - 1)).astype(np.uint32)
    done = np.where(stops, 1, done).astype(np.uint32)
    level = np.where(moves, j, level).astype(np.uint32)
    return level, done, bucket


def group(bucket, J):
    """(tiles grouped by bucket, ascending id inside one; bucket_begin: MAX_BUCKETS + 1 offsets, entries from J (J + 1) / 2 on = the total)"""
    bucket = np.asarray(bucket, np.uint32)
    n_buckets = J * (J + 1) // 2
    tiles, begin = [], np.zeros(MAX_BUCKETS + 1, np.uint32)
    for b in range(n_buckets):
        begin[b] = len(tiles)
        tiles.extend(np.flatnonzero(bucket == b).tolist())
    begin[n_buckets:] = len(tiles)
    return np.asarray(tiles, np.uint32), begin


def allocate(tile_err, target, headroom, spp, level, done):
    """nori_hip_allocate_tiles: (level, done, tiles, bucket_begin)"""
    level, done, bucket = classify(tile_err, target, headroom, spp, level, done)
    tiles, begin = group(bucket, len(spp) - 1)
    return level, done, tiles, begin


def loop(n_tiles, spp, target, headroom, max_rounds, render, evaluate):
    """nori_hip_render_allocated over callbacks: render(tiles or None for all, spp_from, spp_to) adds samples [spp_from, spp_to) of the
    tiles; evaluate(not_done: uint32 ids, ascending or grouped) returns the tile errors of the frames as they are.  Returns (level_log
    [max_rounds + 1, n_tiles], done, passes, the calls made as (tiles, spp_from, spp_to))."""
    J = len(spp) - 1
    level, done = np.zeros(n_tiles, np.uint32), np.zeros(n_tiles, np.uint32)
    calls = [(None, 0, spp[0])]
    render(None, 0, spp[0])
    log = [level.copy()]
    rounds = 0
    while rounds < max_rounds:
        te = evaluate(np.flatnonzero(done == 0).astype(np.uint32))
        level, done, tiles, begin = allocate(te, target, headroom, spp, level, done)
        if tiles.size == 0:
            break
        for (i, j) in pairs(J):
            b = bucket_of(J, i, j)
            part = tiles[begin[b]:begin[b + 1]]
            if part.size:
                render(part, spp[i], spp[j])
                calls.append((part, spp[i], spp[j]))
        rounds += 1
        log.append(level.copy())
    while len(log) < max_rounds + 1:
        log.append(level.copy())
    return np.stack(log), done, len(calls), calls


def moves_of_log(log, k, J):
    """the render calls of round k (1-based) read off a level log: [(tiles, i, j)] in bucket order, empty pairs left out"""
    before, after = np.asarray(log[k - 1]), np.asarray(log[k])
    out = []
    for (i, j) in pairs(J):
        tiles = np.flatnonzero((before == i) & (after == j)).astype(np.uint32)
        if tiles.size:
            out.append((tiles, i, j))
    return out
