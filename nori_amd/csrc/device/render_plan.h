/* render_plan.h -- the host-side arithmetic of a render call as pure functions over plain numbers: tile geometry, the megakernel's
 * chunk plan and sample cut, the wavefront engine's memory budget and out-of-memory ladder (which batches a frame is cut into, hence
 * its bits).  Plain C++17: no HIP, no getenv (the callers read the hooks); pinned without a GPU by tests/test_render_plan_cpu.py. */
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace render_plan {
constexpr int kTileSize = 16;      /* NORI_TILE_SIZE (rt_types.h kTile; ctx.h asserts they agree) */
struct TileGeometry { uint32_t tiles_x, tiles_y, n_sel_tiles; };
struct ChunkPlan { uint32_t n_chunks, chunk_spp; };
struct WfBudget { size_t max_paths, max_samples; };      /* paths in flight (records of the state pool), camera samples per batch (the film's sample store) */
constexpr size_t kUsableUnknown = ~(size_t) 0;      /* no free-memory figure: the options stand */

/* the frame's tiles, and how many of them the progression tile_rem, tile_rem + tile_mod, ... selects (tile_mod >= 1) */
inline TileGeometry tile_geometry(int width, int height, uint32_t tile_mod, uint32_t tile_rem) {
    TileGeometry g;
    g.tiles_x = (uint32_t) ((width + kTileSize - 1) / kTileSize);
    g.tiles_y = (uint32_t) ((height + kTileSize - 1) / kTileSize);
    const uint32_t n_tiles = g.tiles_x * g.tiles_y;
    g.n_sel_tiles = n_tiles > tile_rem ? (n_tiles - tile_rem + tile_mod - 1) / tile_mod : 0;
    return g;
}
inline int32_t tile_width(int border) { return kTileSize + 2 * border; }      /* a tile with the filter's border around it */

/* spp chunking: one workgroup per (tile, chunk of samples); enough workgroups for the dispatcher
   to balance load (target_wgs: measured best around 16 k), at least 8 spp per chunk */
inline ChunkPlan plan_chunks(uint32_t n_sel_tiles, uint32_t spp_count, uint32_t target_wgs) {
    uint32_t n_chunks = 1;
    if (n_sel_tiles > 0 && n_sel_tiles < target_wgs) n_chunks = (target_wgs + n_sel_tiles - 1) / n_sel_tiles;
    n_chunks = std::max(1u, std::min(n_chunks, std::max(1u, spp_count / 8)));
    ChunkPlan p;
    p.chunk_spp = (spp_count + n_chunks - 1) / std::max(1u, n_chunks);
    if (p.chunk_spp == 0) p.chunk_spp = 1;
    p.n_chunks = std::max(1u, (spp_count + p.chunk_spp - 1) / p.chunk_spp);
    return p;
}

/* the sample cut: a call that produces more samples than the film store's budget `cap` is cut into launches of this many spp (n_sel_tiles >= 1) */
inline uint32_t spp_per_launch(uint32_t spp_count, uint32_t n_sel_tiles, size_t cap) {
    return (uint32_t) std::max<size_t>(1, std::min<size_t>(spp_count, cap / ((size_t) n_sel_tiles * 256)));
}

/* What the call can use at all: a batch never holds more samples than the call has, the pool never more paths than a batch
   (reference film order: the frame is one batch whatever the options say -- the pool need not hold it); then bounded by the
   `usable` bytes of the device */
inline WfBudget wavefront_budget(size_t call_samples, size_t opt_paths, size_t opt_samples, bool film_reference, size_t per_path, size_t per_sample, size_t usable) {
    const size_t want_samples = film_reference ? call_samples : opt_samples ? opt_samples : opt_paths;
    WfBudget b;
    b.max_samples = std::max<size_t>(256, std::min(want_samples, call_samples));
    b.max_paths = std::max<size_t>(256, std::min(opt_paths, b.max_samples));
    if (usable != kUsableUnknown && b.max_paths * per_path + b.max_samples * per_sample > usable) {
        /* reference film order: the batch is the frame, the pool takes what is left.  Else the pool keeps its size while the
           sample store can still hold four pools' worth of samples; else both shrink */
        if (film_reference) b.max_paths = std::max<size_t>(256, usable > b.max_samples * per_sample ? (usable - b.max_samples * per_sample) / per_path : 0);
        else if (usable >= b.max_paths * (per_path + 4 * per_sample)) b.max_samples = (usable - b.max_paths * per_path) / per_sample;
        else { b.max_paths = std::max<size_t>(256, usable / (per_path + 4 * per_sample)); b.max_samples = std::min(b.max_samples, 4 * b.max_paths); }
    }
    return b;
}

/* One rung of the out-of-memory ladder; false: there is none left.  The bigger of the two is halved -- the POOL while it is, which
   leaves the batches, hence the bits of the frame, as they were; reference order's one batch cannot shrink; floors at 2^20 */
inline bool wavefront_oom_step(WfBudget &b, bool film_reference, size_t per_path, size_t per_sample) {
    const size_t floor = (size_t) 1 << 20;
    const bool pool_bigger = b.max_paths * per_path >= b.max_samples * per_sample || film_reference;
    if (pool_bigger && b.max_paths > floor) b.max_paths /= 2;
    else if (film_reference) return false;
    else if (b.max_samples > floor) { b.max_samples /= 2; b.max_paths = std::min(b.max_paths, b.max_samples); }
    else if (b.max_paths > floor) b.max_paths /= 2;
    else return false;
    return true;
}
} // namespace render_plan
