/* denoise.hip -- the guide records and the NL-means filter of nori_hip_denoise (see denoise.h). */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "denoise.h"
#include "film.h"
#include "rt_math.h"

using namespace nrt;

namespace {

constexpr int kDnBlock = 256;
/* 4 waves per SIMD = 128 VGPRs, and LDS allows 4 workgroups per CU (160 KiB) up to R = 5 (29-38 KiB); the planes of the
   large window (39-48 KiB) leave 3, so those instantiations ask for no more than they can have */
constexpr int dn_min_waves(int rmax) { return rmax > 5 ? 2 : 4; }
constexpr int kDeltaStride = 40;      /* float2 per row of the delta plane: 80 dwords = 16 mod 64 (denoise.h) */

/* step A (include/nori_hip.h): one thread per pixel of the frame without its border */
__global__ __launch_bounds__(kDnBlock) void denoise_guides_kernel(int width, int height, int border, const float *__restrict__ rgbw, const float *__restrict__ m2,
                                                                  const float *__restrict__ albedo, const float *__restrict__ normal,
                                                                  const float *__restrict__ depth, float4 *__restrict__ guides) {
    const size_t i = (size_t) blockIdx.x * kDnBlock + (size_t) threadIdx.x, n = (size_t) width * (size_t) height;
    if (i >= n) return;
    const int y = (int) (i / (size_t) width), x = (int) (i - (size_t) y * (size_t) width);
    const size_t at = ((size_t) (y + border) * (size_t) (width + 2 * border) + (size_t) (x + border)) * 4;
    const float4 S = *reinterpret_cast<const float4 *>(rgbw + at), M = *reinterpret_cast<const float4 *>(m2 + at);
    float mu[3], var[3];
    const bool valid = denoise_pixel_moments(f4{S.x, S.y, S.z, S.w}, f4{M.x, M.y, M.z, M.w}, mu, var);
    float a[3] = {0.0f, 0.0f, 0.0f}, nn[3] = {0.0f, 0.0f, 0.0f}, z = 0.0f, cov = 0.0f;
    if (albedo) {
        const float4 A = *reinterpret_cast<const float4 *>(albedo + at);
        a[0] = denoise_quot(A.x, A.w); a[1] = denoise_quot(A.y, A.w); a[2] = denoise_quot(A.z, A.w);
    }
    if (normal) {
        const float4 N = *reinterpret_cast<const float4 *>(normal + at);
        if (N.w > 0.0f) { nn[0] = 2.0f * (N.x / N.w) - 1.0f; nn[1] = 2.0f * (N.y / N.w) - 1.0f; nn[2] = 2.0f * (N.z / N.w) - 1.0f; }
    }
    if (depth) {
        const float4 D = *reinterpret_cast<const float4 *>(depth + at);
        cov = denoise_quot(D.z, D.w); z = denoise_quot(D.x, D.z);
    }
    float4 *g = guides + i * 4;
    g[0] = make_float4(mu[0], mu[1], mu[2], var[0]);
    g[1] = make_float4(var[1], var[2], a[0], a[1]);
    g[2] = make_float4(a[2], nn[0], nn[1], nn[2]);
    g[3] = make_float4(z, cov, valid ? 1.0f : 0.0f, 0.0f);
}

/* step B (include/nori_hip.h).  Staged planes: 0-2 mu, 3-5 var, 6 valid, each SIDE x SIDE with the tile at (HALO, HALO);
   a pixel outside the frame is staged as not valid, which is all the stated "outside the frame" tests need. */
template <int F, int RMAX>
__global__ __launch_bounds__(kDnBlock, dn_min_waves(RMAX)) void denoise_filter_kernel(DenoiseLaunch dl, const float4 *__restrict__ guides, float *__restrict__ rgb_out,
                                                                               float *__restrict__ wsum_out) {
    constexpr int HALO = RMAX + F, SIDE = kTile + 2 * HALO, NPIX = SIDE * SIDE, DW = kTile + 2 * F;
    __shared__ float s_g[7][NPIX];
    __shared__ float2 s_delta[2][DW * kDeltaStride];
    const int tid = threadIdx.x;
    const int tiles_x = (dl.width + kTile - 1) / kTile;
    const int x0 = ((int) blockIdx.x % tiles_x) * kTile, y0 = ((int) blockIdx.x / tiles_x) * kTile;
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
    if (wsum_out) wsum_out[o] = valid_p ? wsum : 0.0f;
}

template <int F, int RMAX>
hipError_t launch_filter(const DenoiseLaunch &dl, const float *d_guides, float *d_rgb_out, float *d_wsum, hipStream_t s) {
    const unsigned n_tiles = (unsigned) ((dl.width + kTile - 1) / kTile) * (unsigned) ((dl.height + kTile - 1) / kTile);
    hipLaunchKernelGGL((denoise_filter_kernel<F, RMAX>), dim3(n_tiles), dim3(kDnBlock), 0, s, dl, reinterpret_cast<const float4 *>(d_guides), d_rgb_out, d_wsum);
    return hipGetLastError();
}

template <int F>
hipError_t launch_filter_patch(const DenoiseLaunch &dl, const float *d_guides, float *d_rgb_out, float *d_wsum, hipStream_t s) {
    return dl.radius <= 5 ? launch_filter<F, 5>(dl, d_guides, d_rgb_out, d_wsum, s) : launch_filter<F, 8>(dl, d_guides, d_rgb_out, d_wsum, s);
}

} // namespace

namespace nrt {

std::string denoise_store_guides(DenoiseStore &ds, void *stream, size_t n_pixels, float **out) {
    const size_t need = std::max<size_t>(n_pixels, 1) * kGuideFloats;
    DenoiseStore::Slot *slot = nullptr;
    for (DenoiseStore::Slot &s : ds.slots)
        if (s.stream == stream) slot = &s;
    if (!slot) { ds.slots.push_back(DenoiseStore::Slot{stream, nullptr, 0}); slot = &ds.slots.back(); }
    if (slot->floats < need || !slot->guides) {
        /* (hipFree waits for the device: no kernel still reads the buffer that goes) */
        if (slot->guides) (void) hipFree(slot->guides);
        slot->guides = nullptr; slot->floats = 0;
        const hipError_t e = hipMalloc((void **) &slot->guides, need * sizeof(float));
        if (e != hipSuccess) return std::string("denoise: guide records: ") + hipGetErrorString(e);
        slot->floats = need;
    }
    *out = slot->guides;
    return std::string();
}

void denoise_store_release(DenoiseStore &ds) {
    for (DenoiseStore::Slot &s : ds.slots)
        if (s.guides) (void) hipFree(s.guides);
    ds.slots.clear();
}

uint32_t denoise_filter_lds_bytes(int radius, int patch) {
    const int side = kTile + 2 * ((radius <= 5 ? 5 : 8) + patch);
    return (uint32_t) (7 * side * side * sizeof(float) + 2 * kDeltaStride * (kTile + 2 * patch) * sizeof(float2));
}

hipError_t denoise_guides_launch(int width, int height, int border, const float *d_rgbw, const float *d_m2, const float *d_albedo,
                                 const float *d_normal, const float *d_depth, float *d_guides, void *stream) {
    const size_t n = (size_t) width * (size_t) height;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_guides_kernel, dim3((unsigned) ((n + kDnBlock - 1) / kDnBlock)), dim3(kDnBlock), 0, (hipStream_t) stream, width, height, border,
                       d_rgbw, d_m2, d_albedo, d_normal, d_depth, reinterpret_cast<float4 *>(d_guides));
    return hipGetLastError();
}

hipError_t denoise_filter_launch(const DenoiseLaunch &dl, const float *d_guides, float *d_rgb_out, float *d_wsum, void *stream) {
    if (dl.width <= 0 || dl.height <= 0) return hipSuccess;
    if (dl.radius < 1 || dl.radius > kDenoiseMaxRadius || dl.patch < 0 || dl.patch > kDenoiseMaxPatch) return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t) stream;
    switch (dl.patch) {
    case 0: return launch_filter_patch<0>(dl, d_guides, d_rgb_out, d_wsum, s);
    case 1: return launch_filter_patch<1>(dl, d_guides, d_rgb_out, d_wsum, s);
    default: return launch_filter_patch<2>(dl, d_guides, d_rgb_out, d_wsum, s);
    }
}

} // namespace nrt
