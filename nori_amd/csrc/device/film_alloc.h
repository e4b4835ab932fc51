/*
 * film_alloc.h -- sample levels per tile from the tile errors: classification, grouping of the moving tiles by (from, to) pair.
 *
 * The loop of nori_hip_render_allocated (include/nori_hip.h states the rule operation by operation) keeps a LEVEL l and a DONE
 * flag per tile of the frame; level j stands for spp_j = pilot_spp << j samples, j = 0 .. J <= 7.  A round turns the tile errors into
 * new levels and into one array of the tiles that move, grouped by pair (i, j), i < j, ascending in i then j, ascending tile id
 * inside a pair: bucket b = i J - i (i - 1) / 2 + (j - i - 1), n_buckets = J (J + 1) / 2 <= 28, bucket_begin[b] .. bucket_begin[b + 1].
 *
 *   film_alloc_classify_kernel  one thread per tile applies the rule: writes level, done and the tile's bucket (kAllocStays for a tile
 *                 that does not move).  The level table is a kernel argument.
 *   film_alloc_count_kernel     one workgroup per 256 tiles: the tiles of the block in every bucket, to counts[b * n_blocks + block]
 *                 -- bucket-major, so that ONE exclusive scan of the whole array is at once the offset of every (bucket, block).  The
 *                 28 counters of a block come from one LDS scan: a tile adds 1 to the 9-bit field of its bucket, seven fields to a
 *                 64-bit word, four words; the inclusive scan of the words over the 256 lanes scans every bucket's flags at once.
 *   film_alloc_scan_kernel      one workgroup: lane t owns a run of consecutive counts, the runs' sums are scanned in LDS
 *                 (film_tile_select_scan_kernel's form); the first offset of a bucket goes to bucket_begin[b], the total to
 *                 bucket_begin[n_buckets].
 *   film_alloc_scatter_kernel   one workgroup per 256 tiles: a moving tile goes to offsets[b * n_blocks + block] + its rank among the
 *                 block's tiles of the same bucket with a smaller id -- its field of the same LDS scan, less one.
 *   film_alloc_inverse_kernel   tile -> ordinal for one bucket's slice of the array (the table set to kTileNotListed beforehand), so that a
 *                 render by list resolves through film_resolve_tiles_kernel unchanged.
 *   film_alloc_tile_spp_kernel  tile_spp[t] = spp_level[t].
 * None uses atomics: the order is part of the result and the same inputs give the same bytes, as for film_tile_select_*.  Sized for
 * the 2^20 tiles of a 16384^2 frame: 4096 blocks x 28 buckets = 114688 counts, 448 per lane of the scan.
 */
#pragma once
#include <string>

#include "film_tiles.h"

namespace nrt {

constexpr int kAllocMaxLevel = 7;                                                       /* J <= 7: eight levels */
constexpr int kAllocMaxBuckets = kAllocMaxLevel * (kAllocMaxLevel + 1) / 2;             /* 28 pairs */
constexpr uint32_t kAllocStays = 0xffffffffu;

/* spp[j] = pilot_spp << j for j = 0 .. J; entries above J repeat spp[J] (never read) */
struct AllocLevels {
    uint32_t spp[kAllocMaxLevel + 1];
    uint32_t J;
};

/* the levels of a budget: J = min(7, floor(log2(spp_count / pilot_spp))); false if pilot_spp < 2 or spp_count < pilot_spp */
inline bool alloc_levels(uint32_t pilot_spp, uint32_t spp_count, AllocLevels &lv) {
    if (pilot_spp < 2u || spp_count < pilot_spp) return false;
    uint32_t J = 0;
    while (J < (uint32_t) kAllocMaxLevel && ((uint64_t) pilot_spp << (J + 1)) <= (uint64_t) spp_count) ++J;
    lv.J = J;
    for (uint32_t j = 0; j <= (uint32_t) kAllocMaxLevel; ++j) lv.spp[j] = pilot_spp << (j < J ? j : J);
    return true;
}
/* spp[j] by selection over the eight entries: the table stays in scalar registers for a level that differs from lane to lane */
NORI_HD uint32_t alloc_spp(const AllocLevels &lv, uint32_t j) {
    uint32_t v = lv.spp[0];
#pragma unroll
    for (uint32_t k = 1; k <= (uint32_t) kAllocMaxLevel; ++k) v = j == k ? lv.spp[k] : v;
    return v;
}
NORI_HD uint32_t alloc_n_buckets(uint32_t J) { return J * (J + 1u) / 2u; }
NORI_HD uint32_t alloc_bucket(uint32_t J, uint32_t i, uint32_t j) { return i * J - i * (i - 1u) / 2u + (j - i - 1u); }      /* i < j <= J; (i (i - 1) is even: unsigned wrap at i = 0 gives 0 * ... = 0) */

/* The rule for one tile that is not done (include/nori_hip.h: nori_hip_render_allocated): float32, no contraction, IEEE division.
   Returns the new level; done is set where the tile stops.  The one statement of the rule on the device. */
NORI_HD uint32_t alloc_rule(float E, float target, float headroom, const AllocLevels &lv, uint32_t l, bool &done) {
    done = false;
    if (E <= target) { done = true; return l; }
    const float r = E / target;
    const float need = (headroom * (float) alloc_spp(lv, l)) * (r * r);
    uint32_t j = l;
    while (j < lv.J && !((float) alloc_spp(lv, j) >= need)) ++j;
    if (j == l) done = true;      /* it sits at the top level: unconverged */
    return j;
}

/* What a context holds for the allocation (owned by nori_hip_ctx, grown on demand, freed by film_alloc_release) */
struct FilmAlloc {
    uint32_t *level = nullptr;        /* per tile of the frame */
    uint32_t *done = nullptr;         /* per tile: 0 or 1 */
    uint32_t *bucket = nullptr;       /* per tile: the bucket of the round's move, or kAllocStays */
    uint32_t *list = nullptr;         /* the moving tiles of the last round, grouped by bucket */
    uint32_t *counts = nullptr;       /* n_buckets * n_blocks: counts, then their exclusive prefix sums */
    uint32_t *bucket_begin = nullptr; /* kAllocMaxBuckets + 1 words */
    size_t capacity = 0;              /* tiles of the frame the arrays were sized for */
};

std::string film_alloc_reserve(FilmAlloc &a, size_t n_frame_tiles);
void film_alloc_release(FilmAlloc &a);
/* one round on `stream`: a.level / a.done (DEVICE, current) and d_tile_err -> new a.level / a.done, a.list, and bucket_begin[0 ..
   n_buckets] read back to the HOST array (kAllocMaxBuckets + 1 words; entries above n_buckets repeat the total): synchronises `stream` */
std::string film_alloc_round(FilmAlloc &a, const float *d_tile_err, float target, float headroom, const AllocLevels &lv, size_t n_frame_tiles,
                             uint32_t *bucket_begin, void *stream);
/* d_inverse (n_frame_tiles words) becomes tile -> ordinal for a.list[begin .. begin + n), kTileNotListed elsewhere; asynchronous */
std::string film_alloc_inverse(const FilmAlloc &a, uint32_t begin, uint32_t n, uint32_t *d_inverse, size_t n_frame_tiles, void *stream);
/* d_tile_spp[t] = lv.spp[a.level[t]]; asynchronous */
std::string film_alloc_tile_spp(const FilmAlloc &a, const AllocLevels &lv, uint32_t *d_tile_spp, size_t n_frame_tiles, void *stream);

} // namespace nrt
