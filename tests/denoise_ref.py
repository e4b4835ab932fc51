"""The denoiser of include/nori_hip.h (nori_hip_denoise) restated in numpy float32, operation by operation: guides() is step A,
denoise() step B.  Whole-frame arrays shifted per tap and per patch offset, the loops in the stated order; a sequential
`acc = acc + shifted` reproduces each pixel's own order of additions.  exp is Oracle.libm("exp", x), which
tests/test_gpu_arith.py proves bit-equal to the device's det_expf."""
from __future__ import annotations

import numpy as np

from tests.backends import Oracle

F = np.float32
DEFAULTS = dict(radius=5, patch=1, k_c=1.0, alpha=1.0, tau_albedo=0.02, tau_normal=0.1, k_depth=0.1, tau_cov=0.05)
MU, VAR, ALBEDO, NORMAL, Z, COV, VALID = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12), 12, 13, 14


def _core(a, border, h, w):
    return np.asarray(a, F)[border:border + h, border:border + w]


def _quot(a, b):
    """a / b where b > 0, else 0"""
    with np.errstate(all="ignore"):
        return np.where(b > 0, (a / b).astype(F), F(0)).astype(F)


def guides(rgbw, m2, albedo=None, normal=None, depth=None, border=0):
    """(height, width, 16) float32: mu[3], var[3], albedo[3], normal[3], z, cov, valid, 0"""
    b = int(border)
    h, w = rgbw.shape[0] - 2 * b, rgbw.shape[1] - 2 * b
    S, M = _core(rgbw, b, h, w), _core(m2, b, h, w)
    g = np.zeros((h, w, 16), F)
    with np.errstate(all="ignore"):
        live = S[..., 3] > 0
        r = (F(1) / S[..., 3]).astype(F)
        k = ((M[..., 3] * r).astype(F) * r).astype(F)
        for c in range(3):
            mu = (S[..., c] * r).astype(F)
            q = (M[..., c] * r).astype(F)
            v = (q - (mu * mu).astype(F)).astype(F)
            v = np.where(v > 0, v, F(0)).astype(F)
            g[..., c] = np.where(live, mu, F(0))
            g[..., 3 + c] = np.where(live, (v * k).astype(F), F(0))
        g[..., VALID] = live.astype(F)
        if albedo is not None:
            A = _core(albedo, b, h, w)
            for c in range(3):
                g[..., 6 + c] = _quot(A[..., c], A[..., 3])
        if normal is not None:
            N = _core(normal, b, h, w)
            for c in range(3):
                n = (F(2) * (N[..., c] / N[..., 3]).astype(F)).astype(F) - F(1)
                g[..., 9 + c] = np.where(N[..., 3] > 0, n.astype(F), F(0))
        if depth is not None:
            D = _core(depth, b, h, w)
            g[..., COV] = _quot(D[..., 2], D[..., 3])
            g[..., Z] = _quot(D[..., 0], D[..., 2])
    return g


def _shift(a, dx, dy):
    """out[y, x] = a[y + dy, x + dx] inside the frame, 0 outside"""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    ys, ye = max(0, -dy), min(h, h - dy)
    xs, xe = max(0, -dx), min(w, w - dx)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def denoise(g, with_albedo=True, with_normal=True, with_depth=True, **params):
    """(rgb (height, width, 3), wsum (height, width)) of guide records g; with_*: whether that feature frame was given"""
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    p = {**DEFAULTS, **params}
    R, Fp = int(p["radius"]), int(p["patch"])
    alpha = F(p["alpha"])
    kc2 = F(p["k_c"]) * F(p["k_c"])
    kd2 = F(p["k_depth"]) * F(p["k_depth"])
    tau_a, tau_n, tau_c = F(p["tau_albedo"]), F(p["tau_normal"]), F(p["tau_cov"])
    g = np.asarray(g, F)
    h, w = g.shape[:2]
    valid = g[..., VALID] != 0
    mu, var = g[..., MU], g[..., VAR]
    num, wsum = np.zeros((h, w, 3), F), np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                gq = _shift(g, dx, dy)
                valid_q = gq[..., VALID] != 0
                tap = valid & valid_q
                if not tap.any():
                    continue
                # 1: delta(p', p' + tap) of every pixel p'
                delta = np.zeros((h, w), F)
                for c in range(3):
                    vp, vq = var[..., c], gq[..., 3 + c]
                    t = (mu[..., c] - gq[..., c]).astype(F)
                    nume = ((t * t).astype(F) - (alpha * (vp + np.where(vq < vp, vq, vp)).astype(F)).astype(F)).astype(F)
                    deno = (F(1e-10) + (kc2 * (vp + vq).astype(F)).astype(F)).astype(F)
                    delta = (delta + (nume / deno).astype(F)).astype(F)
                # 2: the patch
                acc, cnt = np.zeros((h, w), F), np.zeros((h, w), np.int32)
                for oy in range(-Fp, Fp + 1):
                    for ox in range(-Fp, Fp + 1):
                        ok = _shift(tap, ox, oy)
                        acc = np.where(ok, (acc + _shift(delta, ox, oy)).astype(F), acc)
                        cnt = cnt + ok
                d = (acc / (F(3) * cnt.astype(F)).astype(F)).astype(F)
                d = np.where(d > 0, d, F(0)).astype(F)
                # 3: the exponent
                e = d
                if with_albedo:
                    s = np.zeros((h, w), F)
                    for c in range(3):
                        t = (g[..., 6 + c] - gq[..., 6 + c]).astype(F)
                        s = (s + (t * t).astype(F)).astype(F)
                    e = (e + (s / tau_a).astype(F)).astype(F)
                if with_normal:
                    s = np.zeros((h, w), F)
                    for c in range(3):
                        t = (g[..., 9 + c] - gq[..., 9 + c]).astype(F)
                        s = (s + (t * t).astype(F)).astype(F)
                    e = (e + (s / tau_n).astype(F)).astype(F)
                if with_depth:
                    zp, zq = g[..., Z], gq[..., Z]
                    t = (zp - zq).astype(F)
                    gg = ((kd2 * ((zp * zp).astype(F) + (zq * zq).astype(F)).astype(F)).astype(F) + F(1e-12)).astype(F)
                    e = (e + ((t * t).astype(F) / gg).astype(F)).astype(F)
                    u = (g[..., COV] - gq[..., COV]).astype(F)
                    e = (e + ((u * u).astype(F) / tau_c).astype(F)).astype(F)
                # 4: the weight
                keep = tap & (e <= F(87))
                wgt = np.zeros((h, w), F)
                if keep.any():
                    wgt[keep] = Oracle.libm("exp", (-e[keep]).astype(F))
                # 5
                for c in range(3):
                    num[..., c] = np.where(tap, (num[..., c] + (wgt * gq[..., c]).astype(F)).astype(F), num[..., c])
                wsum = np.where(tap, (wsum + wgt).astype(F), wsum)
        rgb = np.where(valid[..., None], (num / wsum[..., None]).astype(F), F(0)).astype(F)
    return rgb, np.where(valid, wsum, F(0)).astype(F)


def denoise_frames(rgbw, m2, albedo=None, normal=None, depth=None, border=0, **params):
    g = guides(rgbw, m2, albedo, normal, depth, border)
    return denoise(g, albedo is not None, normal is not None, depth is not None, **params)


def trimmed_error(x, ref, trim=0.01):
    """per pixel sum_c (x - ref)^2 / (sum_c ref^2 + 0.01), averaged after discarding the largest `trim` of the pixels"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    e = np.sort((((x - ref) ** 2).sum(-1) / ((ref ** 2).sum(-1) + 0.01)).reshape(-1))
    return float(e[:e.size - int(np.ceil(trim * e.size))].mean())
