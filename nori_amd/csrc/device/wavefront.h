/* wavefront.h -- the wavefront render engine (see wavefront.hip). */
#pragma once
#include <string>

#include "../../../include/nori_hip.h"
#include "film.h"
#include "rt_types.h"

namespace nrt {

struct WfLaunch {
    uint32_t spp_begin, spp_count;
    uint32_t tile_mod, tile_rem;
    uint32_t tiles_x, tiles_y, n_sel_tiles;
    int32_t tile_w;
    int stack_depth;            /* traversal stack entries the tree needs: max_depth + 1 */
    bool count_traversal;
    bool time_kernels;          /* HIP events around every launch (ktimer.h) */
    size_t max_paths;           /* paths in flight: records of the state pool */
    size_t max_samples;         /* camera samples per batch: what the film's sample store holds at a time (a batch bigger than max_paths
                                   starts its samples pass by pass -- regeneration, wavefront.hip) */
    bool film_reference;        /* add the samples in the reference's order (film.h): needs the whole frame in ONE batch */
    const FilmBlockRows *film_share = nullptr;      /* reference order: the selected tiles are these block rows (tile_mod 1, tile_rem = their first tile) */
    float *d_m2 = nullptr;      /* non-null: the film keeps the samples' second moments and adds them into this frame (film.h) ... */
    FilmMoments *moments = nullptr;      /* ... through the context's second set of accumulators */
    const uint32_t *tile_list = nullptr;      /* a render by list (film_tiles.h): the n_sel_tiles tiles by ordinal, DEVICE memory; null: the progression ... */
    const uint32_t *tile_inverse = nullptr;   /* ... and the list's inverse table for the resolve */
};

struct WfStats {
    unsigned long long n_camera = 0, n_closest = 0, n_shadow = 0, n_nodes = 0, n_tris = 0, n_invalid = 0;
    uint32_t n_batches = 0, n_iterations = 0, n_launches = 0;
    size_t state_bytes = 0;
    float class_ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};      /* KernelClass: trace, shade, film, overlapped tails */
    uint32_t class_launches[4] = {0, 0, 0, 0};
    uint32_t trace_cus = 0;                      /* CUs wf_extend's persistent grid fills: the device's */
    uint32_t tail_cus = 0;                       /* CUs set aside for the tails of the batches (0: tails run on the bulk's stream) */
    uint32_t record = 0;                         /* NORI_WF_RECORD_*: the path record this call's kernels used (wf_records.h) */
};

/* The engine's per-context resources (path-state pool, streams / events, device properties);
 * created on the context's device, owned by nori_hip_ctx, never shared between contexts. */
struct WfEngine;
WfEngine *wavefront_create();
void wavefront_destroy(WfEngine *);
/* HBM bytes one path in flight costs (two state copies + hit record) and one camera sample of a batch costs in the film's
   sample store (both halves of it): size max_paths and max_samples */
size_t wavefront_bytes_per_path();
size_t wavefront_bytes_per_sample();
/* gives the engine's pool back to the device (an out-of-memory retry starts from nothing) */
void wavefront_release_pool(WfEngine *engine);
/* device bytes this context already holds for rendering (they are reusable, so they count as free) */
size_t wavefront_held_bytes(const WfEngine *engine, const FilmStore &film);

/* Renders the selected tiles / samples into d_rgbw (accumulating), on `stream`, with the context's
 * engine resources and film store.  Synchronises the stream.  Returns "" or an error message. */
std::string wavefront_render(WfEngine &engine, FilmStore &film_store, const DevScene &sc, const float *d_filter_table,
                             const WfLaunch &launch, float *d_rgbw, void *stream, WfStats &stats);

/* wf_extend on rays the caller brings (nori_hip_debug_extend, include/nori_hip.h): n records written into state copy 0 as wf_shade
 * would have stored them, ONE launch over the stored paths -- planned by the function that plans a render's launches, environment
 * knobs included --, then the hit records (4n floats, untouched slots keep NORI_EXTEND_SENTINEL) and counts[4] = closest-hit
 * queries, shadow queries, node tests, triangle tests (the last two in counting launches).  All arrays in HOST memory, checked by
 * the caller; n <= wavefront_trace_max_rays(the context's wavefront_paths).  Synchronous on the default stream. */
size_t wavefront_trace_max_rays(size_t max_paths);
std::string wavefront_trace(WfEngine &engine, const DevScene &sc, int stack_depth, bool count_traversal, const float *origins, const float *dir_a,
                            const float *dir_b, const uint32_t *flags, size_t n, float *hits, unsigned long long counts[4]);

/* node records of the LDS image (rt_top.h) that fit next to wf_extend's traversal stacks, per node layout */
int wf_top_capacity(bool wide_nodes, bool records_32b, bool deeper_than_lds_stack);

/* The first pass by per-tile candidate lists (wavefront_first.hip, first_lists.h): a pinhole camera, a BVH2 tree, no counting.
   The engine keeps the lists of its context; they are rebuilt when what they were built for changes (the tree, the camera record,
   the frame's tiles, the filter border, K) and dropped by wavefront_invalidate, which the context calls on every upload and
   acceleration-structure build.  A call with more than one of its selected tiles in sixteen on overflow keeps the old kernel
   (wavefront_render: a ray of an overflow tile costs several times the old kernel's average, a ray of a list tile a third).  Read once per process:
   NORI_HIP_WF_FIRST=0 the old first pass, =2 the lists whatever share of the tiles overflows (tests, A/B); NORI_HIP_WF_FIRST_K=n the
   cap of a list (0: every tile overflows); NORI_HIP_WF_FIRST_REBUILD=1 the lists are built again in every render call. */
struct WfFirstLists;
struct WfFirstInfo { uint32_t K = 0, list_tiles = 0, overflow_tiles = 0; float build_ms = 0.0f; bool rebuilt = false; };
WfFirstLists *wf_first_create();
void wf_first_destroy(WfFirstLists *);
void wf_first_invalidate(WfFirstLists *);
bool wf_first_applies(const DevScene &sc, bool count_traversal);
bool wf_first_forced();
/* builds the lists if they are not the ones of (sc, frame); synchronises `stream` when it builds.  Returns "" or an error message. */
std::string wf_first_prepare(WfFirstLists &lists, const DevScene &sc, uint32_t tiles_x, uint32_t tiles_y, int32_t tile_w, void *stream, WfFirstInfo &info);
/* list / overflow tiles among the tiles a call selects (the progression tile_rem + k tile_mod; a render by tile list, whose list lies in
   device memory, gets the whole frame's counts) */
void wf_first_selected(const WfFirstLists &lists, uint32_t tile_mod, uint32_t tile_rem, uint32_t n_sel, bool by_list, uint32_t &list_tiles, uint32_t &overflow_tiles);
/* in the place of wf_extend<..., kFreshOnly, ...>: wf_buf, batch as for wf_env_launch_shade; grid: workgroups of 256 threads, at most
   as many lanes as the traversal-stack spill buffer was sized for */
void wf_first_launch_extend(const WfFirstLists &lists, const DevScene &sc, const void *wf_buf, int cur, const void *batch, int grid, void *stream);
void wavefront_invalidate(WfEngine *engine);
/* nori_hip_debug_first_lists (include/nori_hip.h): wf_first_build for the 16 x 16 tiles of sc's frame at cap K into buffers of the
   call's own; count[n_tiles] and pairs[n_tiles][max(K, 1)] in HOST memory.  Synchronous on the default stream; touches no engine. */
std::string wf_first_debug_lists(const DevScene &sc, uint32_t K, uint32_t *count, uint32_t *pairs);

/* -DNORI_COUNT_EXCURSIONS builds: adds this translation unit's excursion counters (rt_types.h) to out[4], optionally
   resetting them; false in the product build */
bool wavefront_excursions(unsigned long long out[4], bool reset);

} // namespace nrt
