"""Restatements in numpy of what the second-moment film and the error map compute (include/nori_hip.h:
nori_hip_render_moments, nori_hip_error_map), for tests/test_moments_cpu.py -- which checks them against the oracle and a
binary64 evaluation -- and tests/test_gpu_moments.py, which then holds the device to them.

Weights follow ImageBlock::put of the reference (src/block.cpp:70-84) in the coordinates of the sample's 32x32 block:
    pos   = p - 0.5 - (block_offset - border)                                        float32
    pixel x of the block's bordered accumulator is touched iff ceil(pos.x - r) <= x <= floor(pos.x + r), clipped to it
    wx[x] = table[(int) (|x - pos.x| * lookup)],  lookup = 32 / r,  wy[y] likewise      float32
    w     = float32(wx * wy)
"""
from __future__ import annotations

import numpy as np

BLOCK = 32      # NORI_BLOCK_SIZE
F = np.float32


def filter_radius(rfilter) -> float:
    """the radius the reference's filters end up with (src/rfilter.cpp: tent and box ignore the parameter)"""
    return {"tent": 1.0, "box": 0.5}.get(rfilter.type, float(rfilter.radius))


def border_of(radius) -> int:
    return int(np.ceil(F(radius) - F(0.5)))      # src/block.cpp:20


def sample_weights(p, width, height, radius, table):
    """One sample at frame position p = (px, py), float32: (x0, y0, w) -- w[j, i] = float32(wx[i] * wy[j]) is the weight the
    pixel (x0 + i, y0 + j) of the BORDERED FRAME receives (frame pixel + border).  The sample belongs to the 32x32 block
    that holds the pixel floor(p)."""
    r, b = F(radius), border_of(radius)
    lookup = F(F(len(table) - 1) / r)
    px, py = F(p[0]), F(p[1])
    offx, offy = (int(np.floor(px)) // BLOCK) * BLOCK, (int(np.floor(py)) // BLOCK) * BLOCK
    bw, bh = min(BLOCK, width - offx), min(BLOCK, height - offy)

    def axis(pc, off, size):
        pos = F(F(pc - F(0.5)) - F(off - b))
        lo, hi = max(0, int(np.ceil(F(pos - r)))), min(size + 2 * b - 1, int(np.floor(F(pos + r))))
        xs = np.arange(lo, hi + 1)
        idx = (np.abs(xs.astype(F) - pos).astype(F) * lookup).astype(F).astype(np.int64)
        return lo + off, np.asarray(table, F)[idx]

    x0, wx = axis(px, offx, bw)
    y0, wy = axis(py, offy, bh)
    return x0, y0, (wy[:, None] * wx[None, :]).astype(F)


def sum_w2(positions, width, height, radius, table):
    """binary64 sum over the samples of (float32(wx wy))^2 per pixel of the bordered frame, the sum of |.| (the same: the
    terms are squares) and the number of terms per pixel: what assert_within_summation_bound takes."""
    b = border_of(radius)
    total = np.zeros((height + 2 * b, width + 2 * b), np.float64)
    terms = np.zeros(total.shape, np.uint32)
    for p in np.asarray(positions, F).reshape(-1, 2):
        x0, y0, w = sample_weights(p, width, height, radius, table)
        w2 = (w * w).astype(F).astype(np.float64)      # float32(w w), as the device adds it
        total[y0:y0 + w.shape[0], x0:x0 + w.shape[1]] += w2
        terms[y0:y0 + w.shape[0], x0:x0 + w.shape[1]] += 1
    return total, terms


def error_map(rgbw, m2, border):
    """The formula of nori_hip_error_map operation by operation in float32: (err [height, width], empty mask)."""
    b = int(border)
    h, w = rgbw.shape[0] - 2 * b, rgbw.shape[1] - 2 * b
    S = np.asarray(rgbw, F)[b:b + h, b:b + w]
    M = np.asarray(m2, F)[b:b + h, b:b + w]
    with np.errstate(all="ignore"):
        live = S[..., 3] > 0
        r = (F(1) / S[..., 3]).astype(F)
        k = ((M[..., 3] * r).astype(F) * r).astype(F)
        num, den = np.zeros((h, w), F), np.zeros((h, w), F)
        for c in range(3):
            mu = (S[..., c] * r).astype(F)
            q = (M[..., c] * r).astype(F)
            v = (q - (mu * mu).astype(F)).astype(F)
            v = np.where(v > 0, v, F(0)).astype(F)
            num = (num + np.sqrt((v * k).astype(F)).astype(F)).astype(F)
            den = (den + np.abs(mu)).astype(F)
        err = (num / (den + F(0.03)).astype(F)).astype(F)
    return np.where(live, err, F(0)).astype(F), ~live


def error_map_f64(rgbw, m2, border):
    """the same formula evaluated in binary64 (no intermediate rounding)"""
    b = int(border)
    h, w = rgbw.shape[0] - 2 * b, rgbw.shape[1] - 2 * b
    S = np.asarray(rgbw, np.float64)[b:b + h, b:b + w]
    M = np.asarray(m2, np.float64)[b:b + h, b:b + w]
    with np.errstate(all="ignore"):
        live = S[..., 3] > 0
        r = 1.0 / S[..., 3]
        k = M[..., 3] * r * r
        mu = S[..., :3] * r[..., None]
        v = np.maximum(M[..., :3] * r[..., None] - mu * mu, 0.0)
        err = np.sqrt(v * k[..., None]).sum(-1) / (np.abs(mu).sum(-1) + float(F(0.03)))
    return np.where(live, err, 0.0)


def summary(err, empty, threshold):
    """numpy's side of nori_error_summary"""
    err = np.asarray(err, F)
    return dict(sum_err=float(err.astype(np.float64).sum()), max_err=float(err.max()), n_pixels=int(err.size),
                n_empty=int(np.count_nonzero(empty)), n_above=int(np.count_nonzero(err > F(threshold))))


def hand_made_pair(border=2, seed=5):
    """A (rgbw, m2) pair of an 11 x 9 frame (+ border) with ordinary pixels and the special ones: W = 0, W < 0, q < mu^2 and
    M = 0.  The ordinary pixels have E[L^2] / mean^2 in [3, 6]: v = q - mu^2 then cancels at most a third of q, so the
    float32 evaluation stays within a few ulps of the exact one (relative error of v <= 3.3 u, of sqrt(v k) <= 3.1 u, of
    err <= 7.1 u < 4 ulps' worth, u = 2^-24) and a comparison at 4 ulps tests the formula, not the conditioning of a
    variance near zero."""
    rng = np.random.default_rng(seed)
    h, w = 9 + 2 * border, 11 + 2 * border
    n = rng.uniform(3.0, 40.0, (h, w)).astype(F)                          # sum of weights
    mean = rng.uniform(0.0, 3.0, (h, w, 3)).astype(F)
    rgbw = np.concatenate([mean * n[..., None], n[..., None]], -1).astype(F)
    spread = rng.uniform(3.0, 6.0, (h, w, 3)).astype(F)                   # E[L^2] / mean^2
    m2 = np.concatenate([mean * mean * spread * n[..., None], (n * F(0.4))[..., None]], -1).astype(F)
    b = border
    rgbw[b + 0, b + 0] = 0; m2[b + 0, b + 0] = 0                          # nothing reached the pixel
    rgbw[b + 1, b + 2, 3] = 0                                             # W = 0 with colour
    rgbw[b + 2, b + 3, 3] = F(-0.25)                                      # W < 0 (negative lobes)
    m2[b + 3, b + 4, :3] = rgbw[b + 3, b + 4, :3] * F(0.01)               # q < mu^2: the variance clamps to 0
    m2[b + 4, b + 5] = 0                                                  # M = 0
    m2[b + 5, b + 6, 3] = 0                                               # sum w^2 = 0 alone
    rgbw[b + 6, b + 7, :3] = 0                                            # black pixel with spread: den = 0.03 only
    rgbw[b + 7, b + 1, 0] = F(-1.5)                                       # a negative mean (Mitchell): |mu|
    return rgbw, m2


def emitter_wall(width, height, spp, rfilter, radiance, integrator="path_mats"):
    """One emitter quad that fills the view: black diffuse albedo, so every camera sample carries exactly `radiance`."""
    from nori_amd.scene import Bsdf, Camera, Integrator, Mesh, Scene
    from tests import scenes
    v, f = scenes.quad((-10, -10, 0), (10, -10, 0), (10, 10, 0), (-10, 10, 0))
    wall = Mesh(v, f, bsdf=Bsdf("diffuse", (0.0, 0.0, 0.0)), radiance=tuple(float(c) for c in radiance), name="wall")
    cam = Camera(width, height, 40.0, to_world=scenes.lookat((0, 0, 3), (0, 0, 0), (0, 1, 0)))
    return Scene([wall], cam, rfilter, Integrator(integrator), spp)
