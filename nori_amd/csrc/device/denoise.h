/*
 * denoise.h -- the feature- and variance-guided NL-means denoiser of rendered frames (include/nori_hip.h, nori_hip_denoise).
 * The consumer of the moment frame (film.h) and of the first-hit feature frames (features.h); no counterpart in the reference.
 *
 * A translation unit of its own (denoise.hip): nothing of the path tracer's, the film's or the feature pass's kernels is
 * touched.  Two kernels:
 *   denoise_guides_kernel          step A, elementwise: one thread per frame pixel reads the RGBW, moment and feature pixels and
 *                                  writes the pixel's guide record, 16 floats (kGuide* below), four float4 stores.
 *   denoise_filter_kernel<F, RMAX> step B: one 256-thread workgroup per 16x16 output tile, thread = pixel_in_tile in
 *                                  film_tile_pixel's 8x8-quad numbering.  mu, var and valid of the tile and a halo of RMAX + F
 *                                  are staged in LDS once (7 planes).  Per tap (dy, dx) -- uniform over the workgroup -- the
 *                                  workgroup writes the per-pixel colour distance delta(p', p' + tap) and whether the pair
 *                                  qualifies for the (16 + 2F)^2 pixels p' of the tile and its patch halo ONCE into an LDS plane
 *                                  (float2, double buffered: one barrier per tap); each thread then adds its own patch from that
 *                                  plane in the stated oy, ox order.  The sums have the bits of the naive form, which would
 *                                  evaluate every delta (2F + 1)^2 times.  The features of the tap's pixel are read from the guide
 *                                  records in memory (three float4 per tap, L1 / L2 hits: neighbouring threads read neighbouring
 *                                  records, and every record is read by (2R + 1)^2 threads of at most four tiles).
 *                                  F is a template parameter (the patch loop unrolls); RMAX in {5, 8} sizes the static LDS:
 *                                  R <= 5 runs <F, 5>, larger windows <F, 8>.  The delta plane's row stride is 40 float2 = 80
 *                                  dwords = 16 mod 64: the four pixel rows of a 32-lane half of ds_read_b64 fall on disjoint
 *                                  banks.  LDS: 7 * (16 + 2 (RMAX + F))^2 * 4 + 2 * 40 * (16 + 2F) * 8 bytes -- 33472 at the
 *                                  default R = 5, F = 1 and 49088 at R = 8, F = 2: every instantiation stays below the 64 KiB a
 *                                  workgroup gets without opting in, so the large window is served by the same kernel with a
 *                                  larger static array, features from memory in both.
 *                                  Its body is one __device__ function in denoise_filter.h, which denoise_error.hip compiles a second
 *                                  time with the accumulators of the output's variance (denoise_error.h).
 * No atomics: the same frames give the same bytes.
 */
#pragma once
#include <string>
#include <vector>

#include "rt_types.h"

namespace nrt {

constexpr int kGuideFloats = 16;      /* mu[3], var[3], albedo[3], normal[3], z, cov, valid, 0 */
constexpr uint32_t kDenoiseAlbedo = 1u, kDenoiseNormal = 2u, kDenoiseDepth = 4u;      /* which feature terms step B adds */
constexpr int kDenoiseMaxRadius = 8, kDenoiseMaxPatch = 2;

/* mu and var of one pixel (include/nori_hip.h, step A): the terms of film_pixel_error (film_tiles.h), restated identically --
   float32, no contraction, IEEE division.  S: the RGBW pixel, M: the moment pixel.  false: an empty pixel, mu = var = 0. */
NORI_HD bool denoise_pixel_moments(const f4 &S, const f4 &M, float mu[3], float var[3]) {
    mu[0] = mu[1] = mu[2] = 0.0f; var[0] = var[1] = var[2] = 0.0f;
    if (!(S.w > 0.0f)) return false;
    const float r = 1.0f / S.w, k = (M.w * r) * r;
    const float Sc[3] = {S.x, S.y, S.z}, Mc[3] = {M.x, M.y, M.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float m = Sc[c] * r, q = Mc[c] * r;
        float v = q - m * m;
        if (!(v > 0.0f)) v = 0.0f;
        mu[c] = m; var[c] = v * k;
    }
    return true;
}

/* a quotient of the feature decode: 0 where the divisor is not above 0 */
NORI_HD float denoise_quot(float a, float b) { return b > 0.0f ? a / b : 0.0f; }

/* what one launch of the filter needs beside the guide records: the frame's size and nori_denoise_params with the two squares
   formed once (float32, on the host: one IEEE multiplication each) */
struct DenoiseLaunch {
    int32_t width, height;
    int32_t radius, patch;
    uint32_t terms;                 /* kDenoiseAlbedo | kDenoiseNormal | kDenoiseDepth: the feature frames that were given */
    float kc2, alpha;               /* k_c * k_c */
    float tau_albedo, tau_normal;
    float kd2, tau_cov;             /* k_depth * k_depth */
};

/* What a context holds for the denoiser: guide records for nori_hip_denoise, one buffer per stream that ever called it (two
   streams may run at once and must not share one), grown on demand, freed by denoise_store_release. */
struct DenoiseStore {
    struct Slot { void *stream; float *guides; size_t floats; };
    std::vector<Slot> slots;
};
/* the guide buffer of `stream`, at least n_pixels records; "" or an error */
std::string denoise_store_guides(DenoiseStore &ds, void *stream, size_t n_pixels, float **out);
void denoise_store_release(DenoiseStore &ds);

/* static LDS of the filter kernel that serves (radius, patch) */
uint32_t denoise_filter_lds_bytes(int radius, int patch);
/* step A: d_albedo / d_normal / d_depth may each be null (fields 0).  Frames carry `border` pixels on every side. */
hipError_t denoise_guides_launch(int width, int height, int border, const float *d_rgbw, const float *d_m2, const float *d_albedo,
                                 const float *d_normal, const float *d_depth, float *d_guides, void *stream);
/* step B: d_rgb_out height * width * 3 floats, d_wsum height * width floats or null.  radius in 1..8, patch in 0..2 (checked by the caller). */
hipError_t denoise_filter_launch(const DenoiseLaunch &dl, const float *d_guides, float *d_rgb_out, float *d_wsum, void *stream);

} // namespace nrt
