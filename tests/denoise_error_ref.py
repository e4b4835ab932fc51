"""The denoiser with the variance of its output, and the error of a denoised frame (include/nori_hip.h: nori_hip_denoise_var,
nori_hip_denoised_error_map, nori_hip_denoised_tile_errors), restated in numpy: denoise_var() is tests/denoise_ref.denoise plus the
vnum sum in float32 and the stated order; pixel_error() the formula; tile_errors() the tile tree of tests/adaptive_ref; summary()
the summary in the device's fixed order (256 pixels per workgroup in the tree, lane t then adds the partials t, t + 256, ... in
ascending order, and the tree again), so sum_err is comparable bit for bit."""
from __future__ import annotations

import numpy as np

from tests import adaptive_ref as ar, denoise_ref as dr
from tests.backends import Oracle

F = np.float32


def denoise_var(g, with_albedo=True, with_normal=True, with_depth=True, **params):
    """(rgb (height, width, 3), var (height, width, 3), wsum (height, width)) of guide records g.  The loop of dr.denoise, statement
    for statement (tests/test_denoise_error_cpu.py holds rgb and wsum to it bit for bit), with in step 5
        ww = w * w;  vnum_c = vnum_c + ww * var_qc   and after the loop   var_c = (vnum_c / wsum) / wsum"""
    unknown = set(params) - set(dr.DEFAULTS)
    assert not unknown, unknown
    p = {**dr.DEFAULTS, **params}
    R, Fp = int(p["radius"]), int(p["patch"])
    alpha = F(p["alpha"])
    kc2 = F(p["k_c"]) * F(p["k_c"])
    kd2 = F(p["k_depth"]) * F(p["k_depth"])
    tau_a, tau_n, tau_c = F(p["tau_albedo"]), F(p["tau_normal"]), F(p["tau_cov"])
    g = np.asarray(g, F)
    h, w = g.shape[:2]
    valid = g[..., dr.VALID] != 0
    mu, var = g[..., dr.MU], g[..., dr.VAR]
    num, vnum, wsum = np.zeros((h, w, 3), F), np.zeros((h, w, 3), F), np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                gq = dr._shift(g, dx, dy)
                tap = valid & (gq[..., dr.VALID] != 0)
                if not tap.any():
                    continue
                delta = np.zeros((h, w), F)
                for c in range(3):
                    vp, vq = var[..., c], gq[..., 3 + c]
                    t = (mu[..., c] - gq[..., c]).astype(F)
                    nume = ((t * t).astype(F) - (alpha * (vp + np.where(vq < vp, vq, vp)).astype(F)).astype(F)).astype(F)
                    deno = (F(1e-10) + (kc2 * (vp + vq).astype(F)).astype(F)).astype(F)
                    delta = (delta + (nume / deno).astype(F)).astype(F)
                acc, cnt = np.zeros((h, w), F), np.zeros((h, w), np.int32)
                for oy in range(-Fp, Fp + 1):
                    for ox in range(-Fp, Fp + 1):
                        ok = dr._shift(tap, ox, oy)
                        acc = np.where(ok, (acc + dr._shift(delta, ox, oy)).astype(F), acc)
                        cnt = cnt + ok
                d = (acc / (F(3) * cnt.astype(F)).astype(F)).astype(F)
                d = np.where(d > 0, d, F(0)).astype(F)
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
                    zp, zq = g[..., dr.Z], gq[..., dr.Z]
                    t = (zp - zq).astype(F)
                    gg = ((kd2 * ((zp * zp).astype(F) + (zq * zq).astype(F)).astype(F)).astype(F) + F(1e-12)).astype(F)
                    e = (e + ((t * t).astype(F) / gg).astype(F)).astype(F)
                    u = (g[..., dr.COV] - gq[..., dr.COV]).astype(F)
                    e = (e + ((u * u).astype(F) / tau_c).astype(F)).astype(F)
                keep = tap & (e <= F(87))
                wgt = np.zeros((h, w), F)
                if keep.any():
                    wgt[keep] = Oracle.libm("exp", (-e[keep]).astype(F))
                ww = (wgt * wgt).astype(F)
                for c in range(3):
                    num[..., c] = np.where(tap, (num[..., c] + (wgt * gq[..., c]).astype(F)).astype(F), num[..., c])
                wsum = np.where(tap, (wsum + wgt).astype(F), wsum)
                for c in range(3):
                    vnum[..., c] = np.where(tap, (vnum[..., c] + (ww * gq[..., 3 + c]).astype(F)).astype(F), vnum[..., c])
        rgb = np.where(valid[..., None], (num / wsum[..., None]).astype(F), F(0)).astype(F)
        vout = np.where(valid[..., None], ((vnum / wsum[..., None]).astype(F) / wsum[..., None]).astype(F), F(0)).astype(F)
    return rgb, vout, np.where(valid, wsum, F(0)).astype(F)


def denoise_var_frames(rgbw, m2, albedo=None, normal=None, depth=None, border=0, **params):
    g = dr.guides(rgbw, m2, albedo, normal, depth, border)
    return denoise_var(g, albedo is not None, normal is not None, depth is not None, **params)


def pixel_error(rgb, var, wsum):
    """(err (height, width) float32, empty mask): num = sum_c sqrt(var_c), den = sum_c |rgb_c| in order, err = num / (den + 0.03f);
    0 and empty where !(wsum > 0)"""
    rgb, var, wsum = np.asarray(rgb, F), np.asarray(var, F), np.asarray(wsum, F)
    with np.errstate(all="ignore"):
        live = wsum > 0
        num, den = np.zeros(wsum.shape, F), np.zeros(wsum.shape, F)
        for c in range(3):
            num = (num + np.sqrt(var[..., c]).astype(F)).astype(F)
            den = (den + np.abs(rgb[..., c])).astype(F)
        err = (num / (den + F(0.03)).astype(F)).astype(F)
    return np.where(live, err, F(0)).astype(F), ~live


def tile_errors(rgb, var, wsum):
    """(tiles_y, tiles_x) float32: the tile tree of tests/adaptive_ref over pixel_error"""
    return ar.tile_errors_of_map(pixel_error(rgb, var, wsum)[0])


def _blocks(a, dtype):
    flat = np.asarray(a).reshape(-1)
    n_blocks = (flat.size + 255) // 256
    out = np.zeros(n_blocks * 256, dtype)
    out[:flat.size] = flat
    return out.reshape(n_blocks, 256)


def summary(err, empty, threshold):
    """nori_error_summary of the map in the device's order: the fields but `threshold`"""
    err = np.asarray(err, F)
    part = ar.tree_sum(_blocks(err, np.float64))                 # one partial per workgroup of 256 raster pixels
    lanes = np.zeros(256, np.float64)
    for i in range(part.size):                                   # lane t adds partials t, t + 256, ... in ascending order
        lanes[i % 256] = lanes[i % 256] + part[i]
    return dict(sum_err=float(ar.tree_sum(lanes)), max_err=float(err.max()) if err.size else 0.0, n_pixels=int(err.size),
                n_empty=int(np.count_nonzero(empty)), n_above=int(np.count_nonzero(err > F(threshold))))


def replay_loop(render_pass, n_tiles, filter_frames, target, pass_spp, budget):
    """The loop of nori_hip_render_adaptive_denoised from outside.  render_pass(k, active, count) adds pass k's samples of the
    tiles `active`; filter_frames() -> (rgb, var, wsum) of the frames as they stand (whole frame).  Returns (tile_spp, active at the
    end, passes, [(k, tile errors, stay)] of every evaluated pass)."""
    active = np.arange(n_tiles, dtype=np.uint32)
    tile_spp = np.zeros(n_tiles, np.int64)
    done, passes, log = 0, 0, []
    while done < budget and active.size:
        count = min(pass_spp, budget - done)
        render_pass(passes, active, count)
        tile_spp[active] += count
        done += count
        passes += 1
        if passes >= 2:
            te = tile_errors(*filter_frames()).reshape(-1)
            stay = ar.select(te, target, active)
            log.append((passes - 1, te, stay))
            active = stay
    return tile_spp, active, passes, log
