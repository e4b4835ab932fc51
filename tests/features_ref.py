"""Restatement, without a GPU, of the first-hit feature frames (include/nori_hip.h: nori_hip_render_features) from the CPU oracle's
operator twins: the camera samples, the three values of each sample, the binary64 film of a set of samples and the decode.
tests/test_features_cpu.py checks the restatement against the oracle's `normals` frames; tests/test_gpu_features.py holds the
device to it.

Per camera sample (px, py, s), float32:
    pcg32.seed(py * width + px, s); j = the first two floats; pixelSample = (px + j.x, py + j.y)
    ray = sampleRay(pixelSample); its = the closest hit
    albedo  miss (0, 0, 0); mirror / dielectric (1, 1, 1); else bsdf.albedo, a textured mesh the texture lookup at its.uv
    normal  0.5 n + 0.5 per component of its.sh_n; miss (0.5, 0.5, 0.5)
    depth   (t, float32(t t), 1); miss (0, 0, 0)
"""
from __future__ import annotations

import numpy as np

from tests import moments_ref as mr
from tests import texture_ref as tref
from tests.backends import Oracle

F = np.float32
NAMES = ("albedo", "normal", "depth")
NO_HIT = 0xFFFFFFFF


def camera_samples(width, height, s) -> np.ndarray:
    """(height * width, 2) float32: pixelSample of sample index s of every pixel, raster order"""
    y, x = np.mgrid[0:height, 0:width]
    seeds = (y.astype(np.uint64) * np.uint64(width) + x.astype(np.uint64)).reshape(-1)
    j = Oracle.pcg32_floats(seeds, np.full(seeds.shape, s, np.uint64), 2)
    ps = np.empty((seeds.shape[0], 2), F)
    ps[:, 0] = x.reshape(-1).astype(F) + j[:, 0]
    ps[:, 1] = y.reshape(-1).astype(F) + j[:, 1]
    return ps


def sample_values(scene, ps, oracle=None) -> dict:
    """{"albedo", "normal", "depth"}: (n, 3) float32 each, and "hit": (n,) bool, for the pixel samples ps of `scene`"""
    o = oracle or Oracle(scene, use_bvh=True)
    its = o.intersect(o.sample_rays(ps))
    if oracle is None:
        o.close()
    n = ps.shape[0]
    hit = its["mesh"] != NO_HIT
    albedo, normal, depth = np.zeros((n, 3), F), np.full((n, 3), F(0.5)), np.zeros((n, 3), F)
    for mi, m in enumerate(scene.meshes):
        sel = hit & (its["mesh"] == mi)
        if not sel.any():
            continue
        if m.bsdf.type in ("mirror", "dielectric"):
            albedo[sel] = F(1)
        elif m.albedo_texture is not None:
            albedo[sel] = tref.lookup(scene.textures[m.albedo_texture], its["uv"][sel])
        else:
            albedo[sel] = np.asarray(m.bsdf.albedo, F)
    normal[hit] = F(0.5) * its["sh_n"][hit].astype(F) + F(0.5)
    t = its["t"][hit].astype(F)
    depth[hit] = np.stack([t, (t * t).astype(F), np.ones_like(t)], axis=1)
    return {"albedo": albedo, "normal": normal, "depth": depth, "hit": hit}


def job_samples(scene, spp_begin, spp_count, oracle=None):
    """(ps (n, 2), values dict) of samples [spp_begin, spp_begin + spp_count) of every pixel of the frame"""
    c = scene.camera
    o = oracle or Oracle(scene, use_bvh=True)
    ps = np.concatenate([camera_samples(c.width, c.height, s) for s in range(spp_begin, spp_begin + spp_count)])
    vals = sample_values(scene, ps, o)
    if oracle is None:
        o.close()
    return ps, vals


def film_f64(ps, values, width, height, radius, table):
    """The binary64 film of the samples (ps, values (n, 3)) -- every value must pass the film's guard --: (total, abs_total)
    [rows, cols, 4] of the bordered frame, the sums of v * float32(wx wy) and of their magnitudes in RGBW, and terms [rows, cols],
    the number of samples that reach each pixel: what assert_within_summation_bound (tests/test_gpu_parity.py) takes.  `values`
    may be a list of arrays: one (total, abs_total) per entry, the weights computed once."""
    many = isinstance(values, (list, tuple))
    vs = [np.asarray(v, F).astype(np.float64) for v in (values if many else [values])]
    for v in vs:
        assert np.isfinite(v).all() and (v >= 0).all()
    b = mr.border_of(radius)
    shape = (height + 2 * b, width + 2 * b, 4)
    rgbw = np.ones((len(ps), len(vs), 1, 1, 4), np.float64)      # [sample, plane, 1, 1, channel]
    for i, v in enumerate(vs):
        rgbw[:, i, 0, 0, :3] = v
    totals, abss = np.zeros((len(vs),) + shape, np.float64), np.zeros((len(vs),) + shape, np.float64)
    terms = np.zeros(shape[:2], np.uint32)
    for k, p in enumerate(np.asarray(ps, F).reshape(-1, 2)):
        x0, y0, w = mr.sample_weights(p, width, height, radius, table)
        term = w.astype(np.float64)[None, :, :, None] * rgbw[k]
        terms[y0:y0 + w.shape[0], x0:x0 + w.shape[1]] += 1
        totals[:, y0:y0 + w.shape[0], x0:x0 + w.shape[1]] += term
        abss[:, y0:y0 + w.shape[0], x0:x0 + w.shape[1]] += np.abs(term)
    out = [(totals[i], abss[i], terms) for i in range(len(vs))]
    return out if many else out[0]


def decode(frames: dict, border: int) -> dict:
    """the decode the header states, spelt out per pixel class: albedo rgb / W; normal 2 rgb / W - 1; depth (R / B, B / W, G / B);
    0 where a divisor is <= 0.  Without the border, float32."""
    out = {}
    for name, a in frames.items():
        a = np.asarray(a, F)
        h, w = a.shape[0] - 2 * border, a.shape[1] - 2 * border
        c = a[border:border + h, border:border + w]
        res = np.zeros((h, w, 3), F)
        W = c[..., 3]
        ok = W > 0
        if name == "albedo":
            res[ok] = c[..., :3][ok] / W[ok][:, None]
        elif name == "normal":
            res[ok] = F(2) * (c[..., :3][ok] / W[ok][:, None]) - F(1)
        else:
            cov = c[..., 2] > 0
            res[..., 0][cov] = c[..., 0][cov] / c[..., 2][cov]
            res[..., 1][ok] = c[..., 2][ok] / W[ok]
            res[..., 2][cov] = c[..., 1][cov] / c[..., 2][cov]
        out[name] = res
    return out
