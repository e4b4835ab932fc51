/*
 * denoise_error.h -- the denoiser with the variance of its output, and the error of a denoised frame: per pixel, as a map with its
 * summary, and as tile means (include/nori_hip.h: nori_hip_denoise_var, nori_hip_denoised_error_map, nori_hip_denoised_tile_errors).
 * What lets the adaptive loop retire tiles on the error of the frame the user will look at (nori_hip_render_adaptive_denoised).
 *
 * A translation unit of its own (denoise_error.hip); nothing of denoise.hip's, the film's or the tile list's kernels is touched:
 *   denoise_filter_var_kernel<F, RMAX>   step B with three more accumulators (denoise_filter.h, VAR = true): per tap ww = w * w,
 *                                        vnum_c = vnum_c + ww * var_qc with var_q from the staged planes 3 - 5 -- the LDS, the launch
 *                                        bounds and the bits of rgb_out and wsum are those of denoise_filter_kernel<F, RMAX>.  One
 *                                        workgroup handles the tile list ? list[blockIdx.x] : blockIdx.x; pixels of other tiles are
 *                                        not written, guide records are read for the whole frame (halos reach into neighbours).
 *   denoise_error_map_kernel             one thread per frame pixel: denoised_pixel_error below, and the workgroup's partial sums in
 *   denoise_error_reduce_kernel          the fixed tree of film.hip's error map (lane t takes lane t + off, off = 128 .. 1; one
 *                                        workgroup then adds the partials t, t + 256, ... in ascending order and the tree again).
 *   denoise_tile_errors_kernel           film_tile_errors_kernel for the denoised pixel error: one workgroup per tile of the frame,
 *                                        thread ly * 16 + lx, the binary64 tree, tile_err = (float) (sum / pixels inside).
 * No atomics: the same inputs give the same bytes.
 */
#pragma once
#include <string>

#include "denoise.h"
#include "film.h"
#include "rt_types.h"

namespace nrt {

/* The relative standard error of one denoised pixel (include/nori_hip.h: nori_hip_denoised_error_map states it): the form of
   film_pixel_error (film_tiles.h) with the filter's output and its variance in place of the pixel's mean and the variance of that
   mean, so a target means the same thing to both loops.  float32, no contraction, IEEE division and square root.  The one
   statement of the formula: the map and the tile errors both call it. */
NORI_HD float denoised_pixel_error(const float rgb[3], const float var[3], float wsum, bool &empty) {
    empty = false;
    if (!(wsum > 0.0f)) { empty = true; return 0.0f; }
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        num = num + __builtin_sqrtf(var[c]);
        den = den + __builtin_fabsf(rgb[c]);
    }
    return num / (den + 0.03f);
}

/* What a context holds for the summary of the denoised error map: its partial sums, grown on demand. */
struct DenoiseErrorStore {
    void *partials = nullptr;
    size_t blocks = 0;
};
void denoise_error_release(DenoiseErrorStore &s);

/* step B with the output variance over the tiles of d_list (DEVICE, n_list entries), or, d_list null, over all tiles of the frame.
   d_rgb_out, d_var_out: height * width * 3 floats; d_wsum: height * width floats or null.  radius, patch: checked by the caller. */
hipError_t denoise_filter_var_launch(const DenoiseLaunch &dl, const float *d_guides, const uint32_t *d_list, uint32_t n_list,
                                     float *d_rgb_out, float *d_var_out, float *d_wsum, void *stream);
/* the error map of a denoised frame and its summary: d_err (height * width floats) and `out` may each be null.  With `out` the call
   goes through the store's partial sums and synchronises `stream`.  "" or an error. */
std::string denoised_error_map(DenoiseErrorStore &store, int width, int height, const float *d_rgb, const float *d_var, const float *d_wsum,
                               float *d_err, float threshold, FilmErrorSummary *out, void *stream);
/* d_tile_err[t] for every tile of the frame; asynchronous on `stream` */
std::string denoised_tile_errors(int width, int height, const float *d_rgb, const float *d_var, const float *d_wsum, float *d_tile_err, void *stream);

} // namespace nrt
