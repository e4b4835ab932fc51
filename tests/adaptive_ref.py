"""Restatements in numpy of the tile errors and the tile selection (include/nori_hip.h: nori_hip_tile_errors,
nori_hip_select_tiles), for tests/test_adaptive_cpu.py -- which checks them on hand-made frames -- and
tests/test_gpu_adaptive.py, which then holds the device to them bit for bit.

    thread ly * 16 + lx of tile (tx, ty):  e = err of frame pixel (16 tx + lx, 16 ty + ly)  (tests/moments_ref.error_map), 0 outside the frame
    the 256 values as binary64, added in a tree: for off = 128, 64, ..., 1: lane t < off takes lane t + off
    tile_err = float32(sum / n),  n = pixels of the tile inside the frame
"""
from __future__ import annotations

import numpy as np

from tests import moments_ref as mr

TILE = 16
F = np.float32


def tile_grid(width, height):
    """(tiles_y, tiles_x)"""
    return (height + TILE - 1) // TILE, (width + TILE - 1) // TILE


def tile_pixels(width, height):
    """[tiles_y, tiles_x] pixels of every tile inside the frame"""
    ty, tx = tile_grid(width, height)
    ny = np.minimum(TILE, height - TILE * np.arange(ty))
    nx = np.minimum(TILE, width - TILE * np.arange(tx))
    return ny[:, None] * nx[None, :]


def tree_sum(lanes):
    """[..., 256] binary64 -> [...]: lane t takes lane t + off for off = 128, 64, ..., 1, in that order"""
    s = np.array(lanes, np.float64)
    assert s.shape[-1] == TILE * TILE
    off = TILE * TILE // 2
    while off:
        s[..., :off] = s[..., :off] + s[..., off:2 * off]
        off //= 2
    return s[..., 0]


def tile_errors_of_map(err):
    """[tiles_y, tiles_x] float32 from the error map [height, width] (float32, 0 at empty pixels)"""
    err = np.asarray(err, F)
    height, width = err.shape
    ty, tx = tile_grid(width, height)
    padded = np.zeros((ty * TILE, tx * TILE), np.float64)
    padded[:height, :width] = err.astype(np.float64)
    lanes = padded.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty, tx, TILE * TILE)      # lane = ly * 16 + lx
    return (tree_sum(lanes) / tile_pixels(width, height).astype(np.float64)).astype(F)


def tile_errors(rgbw, m2, border):
    err, _ = mr.error_map(rgbw, m2, border)
    return tile_errors_of_map(err)


def select(tile_err, target, tiles):
    """the tiles of `tiles` with not (tile_err[t] <= target), in their order: a NaN stays in"""
    e = np.asarray(tile_err, F).reshape(-1)
    tiles = np.asarray(tiles, np.uint32).reshape(-1)
    with np.errstate(invalid="ignore"):
        keep = ~(e[tiles] <= F(target))
    return tiles[keep]


def random_pair(width, height, border, seed):
    """A made-up (rgbw, m2) pair of a width x height frame (+ border) in the manner of moments_ref.hand_made_pair, with the special
    pixels -- W = 0, W < 0, a negative variance, M = 0 -- scattered over it and one tile of nothing but empty pixels."""
    rng = np.random.default_rng(seed)
    h, w = height + 2 * border, width + 2 * border
    n = rng.uniform(3.0, 40.0, (h, w)).astype(F)
    mean = rng.uniform(0.0, 3.0, (h, w, 3)).astype(F)
    spread = rng.uniform(1.2, 6.0, (h, w, 3)).astype(F)
    rgbw = np.concatenate([mean * n[..., None], n[..., None]], -1).astype(F)
    m2 = np.concatenate([mean * mean * spread * n[..., None], (n * F(0.4))[..., None]], -1).astype(F)
    # errors that differ from tile to tile, so that a target splits the tiles: scale the moments per tile
    ty, tx = tile_grid(width, height)
    scale = rng.uniform(1.0, 3.0, (ty, tx)).astype(F)
    core = m2[border:border + height, border:border + width]
    core[..., :3] *= np.repeat(np.repeat(scale, TILE, 0), TILE, 1)[:height, :width, None]
    ys, xs = rng.integers(0, height, 40), rng.integers(0, width, 40)
    for i, (y, x) in enumerate(zip(ys, xs)):
        y, x = int(y) + border, int(x) + border
        kind = i % 4
        if kind == 0:
            rgbw[y, x, 3] = 0                                   # W = 0 with colour
        elif kind == 1:
            rgbw[y, x, 3] = F(-0.25)                            # W < 0
        elif kind == 2:
            m2[y, x, :3] = rgbw[y, x, :3] * F(0.01)             # q < mu^2: the variance clamps to 0
        else:
            m2[y, x] = 0                                        # M = 0
    if ty > 1 and tx > 1:                                       # a whole tile of empty pixels: tile error 0
        rgbw[border + TILE:border + 2 * TILE, border + TILE:border + 2 * TILE] = 0
    return rgbw, m2
