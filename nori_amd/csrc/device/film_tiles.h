/*
 * film_tiles.h -- tile lists: the film for renders of exactly the listed 16x16 tiles, per-tile errors, selection.
 *
 * A render names its tiles either as the progression tile_rem + ordinal * tile_mod (every render before the adaptive loop)
 * or as a LIST: ascending raster ids in device memory, ordinal -> tile, plus its INVERSE table, one uint32 per tile of the
 * frame, tile -> ordinal or kTileNotListed.  RenderArgs, WfLaunch / WfBatch and FilmLaunch carry the list as a pointer that
 * is null for the progression; the sample store and the tile accumulators are indexed by ordinal either way, so a list
 * changes nothing but which pixels an ordinal stands for.
 *
 *   film_resolve_tiles_kernel  film_resolve_kernel with the ordinal read from the inverse table: the same loop over the
 *                 covering tiles and parts in the same order, so a list that equals a progression gives the frame the same
 *                 bits.  (A kernel of its own: one more pointer argument would cost film_resolve_kernel four SGPRs.)
 *   film_tile_errors_kernel    one workgroup per tile of the frame, thread ly * 16 + lx evaluates film_pixel_error of frame pixel
 *                 (x0 + lx, y0 + ly) -- 0 outside the frame --, the 256 values are added in binary64 in the fixed tree of the
 *                 error map's summary (lane t takes lane t + off, off = 128 .. 1), tile_err = (float) (sum / pixels inside).
 *   film_tile_select_*         the tiles of a list with !(tile_err <= target), in the list's order: a stable compaction by
 *                 prefix sum (count per 256 entries, one workgroup scans the counts, scatter), never an atomic append --
 *                 the order is part of the result.  Writes the new list, its length and its inverse table.
 * None uses atomics: the same inputs give the same bytes.
 */
#pragma once
#include <string>

#include "film.h"
#include "rt_types.h"

namespace nrt {

constexpr uint32_t kTileNotListed = 0xffffffffu;

/* The relative standard error of one pixel's mean (include/nori_hip.h: nori_hip_error_map states it operation by operation;
   float32, no contraction, IEEE division and square root -- hipcc's correctly rounded default).  S: the RGBW pixel, M: the
   moment pixel.  The one statement of the formula: the error map and the tile errors both call it. */
NORI_HD float film_pixel_error(const f4 &S, const f4 &M, bool &empty) {
    empty = false;
    if (!(S.w > 0.0f)) { empty = true; return 0.0f; }
    const float r = 1.0f / S.w, k = (M.w * r) * r;
    float num = 0.0f, den = 0.0f;
    const float Sc[3] = {S.x, S.y, S.z}, Mc[3] = {M.x, M.y, M.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float mu = Sc[c] * r, q = Mc[c] * r;
        float v = q - mu * mu;
        if (!(v > 0.0f)) v = 0.0f;
        num = num + __builtin_sqrtf(v * k);
        den = den + __builtin_fabsf(mu);
    }
    return num / (den + 0.03f);
}

/* What a context holds for tile lists (owned by nori_hip_ctx, grown on demand, freed by film_tiles_release): two lists -- the
   current one, and the one a selection writes --, the inverse table of the current one, its length on the device, the counts of
   the selection's scan, the tile errors and the samples per tile of the adaptive loop. */
struct FilmTiles {
    uint32_t *list[2] = {nullptr, nullptr};
    uint32_t *inverse = nullptr;
    uint32_t *d_count = nullptr;        /* length of the list the last selection wrote */
    uint32_t *block_counts = nullptr;   /* survivors per 256 entries, then their exclusive prefix sums */
    float *tile_err = nullptr;
    uint32_t *tile_spp = nullptr;
    size_t capacity = 0;                /* tiles of the frame the arrays were sized for */
    int cur = 0;                        /* which list is the current one */
    uint32_t n = 0;                     /* its length */
};

/* (re)allocates for a frame of n_frame_tiles tiles.  "" or an error. */
std::string film_tiles_reserve(FilmTiles &t, size_t n_frame_tiles);
void film_tiles_release(FilmTiles &t);
/* makes `tiles` (HOST, strictly ascending, every id < n_frame_tiles: checked by the caller) the current list, with its inverse
   table; synchronises `stream` (the host arrays are temporaries) */
std::string film_tiles_upload(FilmTiles &t, const uint32_t *tiles, uint32_t n, size_t n_frame_tiles, void *stream);
/* the resolve of a render by list (film_resolve calls it when the launch carries an inverse table) */
void film_resolve_tiles(const DevScene &sc, const FilmStore &st, const FilmLaunch &fl, float *d_rgbw, void *stream);
/* d_tile_err[t] for every tile of the frame; asynchronous on `stream` */
std::string film_tile_errors(const DevScene &sc, const float *d_rgbw, const float *d_m2, float *d_tile_err, void *stream);
/* the current list's tiles with !(d_tile_err[t] <= target) become the current list (and inverse table); t.n is read back:
   synchronises `stream` */
std::string film_tiles_select(FilmTiles &t, const float *d_tile_err, float target, size_t n_frame_tiles, void *stream);
/* d_tile_spp[t] += spp for the tiles of the current list */
void film_tiles_add_spp(const FilmTiles &t, uint32_t *d_tile_spp, uint32_t spp, void *stream);

} // namespace nrt
