/*
 * denoise_filter.h -- step B of the denoiser (include/nori_hip.h: nori_hip_denoise) as ONE device function, instantiated twice:
 *   VAR = false  denoise_filter_kernel<F, RMAX> of denoise.hip: the filter as denoise.h describes it, same LDS, same bits
 *   VAR = true   denoise_filter_var_kernel<F, RMAX> of denoise_error.hip: the same loop with three more accumulators, the variance
 *                of the output under fixed weights (include/nori_hip.h: nori_hip_denoise_var).  var_q of the tap is read from the
 *                staged planes 3 - 5, so the LDS is the same.
 * (The film's _m2 kernels are the precedent: one text, a compile-time flag.)  The caller names the tile: blockIdx.x for the
 * whole frame, an entry of a tile list otherwise; only that tile's pixels are written.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "denoise.h"
#include "film.h"
#include "rt_math.h"

namespace nrt {

constexpr int kDnBlock = 256;
/* 4 waves per SIMD = 128 VGPRs, and LDS allows 4 workgroups per CU (160 KiB) up to R = 5 (29-38 KiB); the planes of the
   large window (39-48 KiB) leave 3, so those instantiations ask for no more than they can have */
constexpr int dn_min_waves(int rmax) { return rmax > 5 ? 2 : 4; }
constexpr int kDeltaStride = 40;      /* float2 per row of the delta plane: 80 dwords = 16 mod 64 (denoise.h) */

/* step B (include/nori_hip.h).  Staged planes: 0-2 mu, 3-5 var, 6 valid, each SIDE x SIDE with the tile at (HALO, HALO);
   a pixel outside the frame is staged as not valid, which is all the stated "outside the frame" tests need. */
template <int F, int RMAX, bool VAR>
__device__ __forceinline__ void denoise_filter_body(const DenoiseLaunch &dl, const float4 *__restrict__ guides, const int tile, float *__restrict__ rgb_out,
                                                    float *__restrict__ var_out, float *__restrict__ wsum_out) {
    constexpr int HALO = RMAX + F, SIDE = kTile + 2 * HALO, NPIX = SIDE * SIDE, DW = kTile + 2 * F;
    __shared__ float s_g[7][NPIX];
    __shared__ float2 s_delta[2][DW * kDeltaStride];
    const int tid = threadIdx.x;
    const int tiles_x = (dl.width + kTile - 1) / kTile;
    const int x0 = (tile % tiles_x) * kTile, y0 = (tile / tiles_x) * kTile;
    const int R = dl.radius;

    for (int i = tid; i < NPIX; i += kDnBlock) {
        const int sy = i / SIDE, sx = i - sy * SIDE;
        const int gx = x0 - HALO + sx, gy = y0 - HALO + sy;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, d = a;
        if (gx >= 0 && gy >= 0 && gx < dl.width && gy < dl.height) {
            const float4 *g = guides + ((size_t) gy * (size_t) dl.width + (size_t) gx) * 4;
            a = g[0]; b = g[1]; d = g[3];
        }
        s_g[0][i] = a.x; s_g[1][i] = a.y; s_g[2][i] = a.z;
        s_g[3][i] = a.w; s_g[4][i] = b.x; s_g[5][i] = b.y;
        s_g[6][i] = d.z;
    }

    int px, py; film_tile_pixel(tid, x0, y0, px, py);
    const int lx = px - x0, ly = py - y0;
    const bool live = px < dl.width && py < dl.height;
    const int centre = (ly + HALO) * SIDE + (lx + HALO);
    const bool with_albedo = (dl.terms & kDenoiseAlbedo) != 0u, with_normal = (dl.terms & kDenoiseNormal) != 0u, with_depth = (dl.terms & kDenoiseDepth) != 0u;
    float ap[3] = {0.0f, 0.0f, 0.0f}, np[3] = {0.0f, 0.0f, 0.0f}, zp = 0.0f, covp = 0.0f;
    if (live && dl.terms != 0u) {
        const float4 *g = guides + ((size_t) py * (size_t) dl.width + (size_t) px) * 4;
        const float4 g1 = g[1], g2 = g[2], g3 = g[3];
        ap[0] = g1.z; ap[1] = g1.w; ap[2] = g2.x; np[0] = g2.y; np[1] = g2.z; np[2] = g2.w; zp = g3.x; covp = g3.y;
    }
    __syncthreads();
    const bool valid_p = live && s_g[6][centre] != 0.0f;

    float num[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    float vnum[3] = {0.0f, 0.0f, 0.0f};      /* VAR: sum of w^2 var_q */
    int tap = 0;
    for (int dy = -R; dy <= R; ++dy) {
        for (int dx = -R; dx <= R; ++dx, ++tap) {
            float2 *plane = s_delta[tap & 1];
            const int shift = dy * SIDE + dx;
            /* 1: delta(p', p' + tap) of every p' of the tile and its patch halo, once */
            for (int i = tid; i < DW * DW; i += kDnBlock) {
                const int iy = i / DW, ix = i - iy * DW;
                const int pc = (iy + HALO - F) * SIDE + (ix + HALO - F), qc = pc + shift;
                float delta = 0.0f, ok = 0.0f;
                if (s_g[6][pc] != 0.0f && s_g[6][qc] != 0.0f) {
                    ok = 1.0f;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float mp = s_g[c][pc], mq = s_g[c][qc], vp = s_g[3 + c][pc], vq = s_g[3 + c][qc];
                        const float t = mp - mq;
                        const float nume = t * t - dl.alpha * (vp + (vq < vp ? vq : vp));
                        const float deno = 1e-10f + dl.kc2 * (vp + vq);
                        delta = delta + nume / deno;
                    }
                }
                plane[iy * kDeltaStride + ix] = make_float2(delta, ok);
            }
            __syncthreads();      /* the only barrier of a tap: the next tap writes the other plane, which every thread has finished reading */
            /* 2-5: this thread's patch, exponent, weight */
            const int qc = centre + shift;
            if (valid_p && s_g[6][qc] != 0.0f) {
                float acc = 0.0f;
                int cnt = 0;
#pragma unroll
                for (int oy = -F; oy <= F; ++oy)
#pragma unroll
                    for (int ox = -F; ox <= F; ++ox) {
                        const float2 v = plane[(ly + F + oy) * kDeltaStride + (lx + F + ox)];
                        if (v.y != 0.0f) { acc = acc + v.x; cnt += 1; }
                    }
                float d = acc / (3.0f * (float) cnt);
                if (!(d > 0.0f)) d = 0.0f;
                float e = d;
                if (dl.terms != 0u) {
                    const float4 *g = guides + ((size_t) (py + dy) * (size_t) dl.width + (size_t) (px + dx)) * 4;
                    if (with_albedo || with_normal) {
                        const float4 g1 = g[1], g2 = g[2];
                        if (with_albedo) {
                            const float aq[3] = {g1.z, g1.w, g2.x};
                            float s = 0.0f;
#pragma unroll
                            for (int c = 0; c < 3; ++c) { const float t = ap[c] - aq[c]; s = s + t * t; }
                            e = e + s / dl.tau_albedo;
                        }
                        if (with_normal) {
                            const float nq[3] = {g2.y, g2.z, g2.w};
                            float s = 0.0f;
#pragma unroll
                            for (int c = 0; c < 3; ++c) { const float t = np[c] - nq[c]; s = s + t * t; }
                            e = e + s / dl.tau_normal;
                        }
                    }
                    if (with_depth) {
                        const float4 g3 = g[3];
                        const float zq = g3.x, covq = g3.y;
                        const float t = zp - zq;
                        const float gg = dl.kd2 * (zp * zp + zq * zq) + 1e-12f;
                        e = e + (t * t) / gg;
                        const float u = covp - covq;
                        e = e + (u * u) / dl.tau_cov;
                    }
                }
                const float w = e <= 87.0f ? det_expf(-e) : 0.0f;
#pragma unroll
                for (int c = 0; c < 3; ++c) num[c] = num[c] + w * s_g[c][qc];
                wsum = wsum + w;
                if constexpr (VAR) {
                    const float ww = w * w;
#pragma unroll
                    for (int c = 0; c < 3; ++c) vnum[c] = vnum[c] + ww * s_g[3 + c][qc];
                }
            }
        }
    }
    if (!live) return;
    const size_t o = (size_t) py * (size_t) dl.width + (size_t) px;
    if (valid_p) {
        rgb_out[o * 3 + 0] = num[0] / wsum; rgb_out[o * 3 + 1] = num[1] / wsum; rgb_out[o * 3 + 2] = num[2] / wsum;
    } else {
        rgb_out[o * 3 + 0] = 0.0f; rgb_out[o * 3 + 1] = 0.0f; rgb_out[o * 3 + 2] = 0.0f;
    }
    if constexpr (VAR) {
        if (valid_p) {
            var_out[o * 3 + 0] = (vnum[0] / wsum) / wsum; var_out[o * 3 + 1] = (vnum[1] / wsum) / wsum; var_out[o * 3 + 2] = (vnum[2] / wsum) / wsum;
        } else {
            var_out[o * 3 + 0] = 0.0f; var_out[o * 3 + 1] = 0.0f; var_out[o * 3 + 2] = 0.0f;
        }
    }
    if (wsum_out) wsum_out[o] = valid_p ? wsum : 0.0f;
}

} // namespace nrt
