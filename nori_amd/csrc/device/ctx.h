/* ctx.h -- the context behind the C ABI and what the entry points of nori_hip.hip, frame_api.hip, env_map.hip, medium.hip, grid_medium.hip and lights.hip (those units only) need
 * of it: the error mapping, the device guard, scratch buffers, the frame's sizes, the stats of a call. */
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../../include/nori_hip.h"
#include "film.h"
#include "film_tiles.h"
#include "film_alloc.h"
#include "features.h"
#include "denoise.h"
#include "denoise_error.h"
#include "scene_prep.h"
#include "wavefront.h"
#include "render_plan.h"

using namespace nrt;
static_assert(render_plan::kTileSize == kTile, "render_plan.h plans in tiles of rt_types.h");

struct nori_hip_ctx {
    int device = 0;
    std::string error;
    bool have_scene = false, have_accel = false;
    HostScene host;
    HostBvh bvh;
    DevScene dev;
    std::vector<void *> allocs_scene, allocs_accel;
    std::vector<void *> allocs_env;      /* the environment map (env_map.hip): texels, tables, the record DevScene::env points at */
    uint32_t env_size = 0;               /* its N; 0 while dev.env is null */
    const float *d_env_weight = nullptr; /* its texel weights (nori_hip_debug_env_tables; the path reads the CDFs only) */
    void *d_lights = nullptr;            /* the delta lights (lights.hip): the array DevScene::lights points at */
    std::vector<LightRec> host_lights;   /* ... as stored (nori_hip_get_lights) */
    void *d_grid_rho = nullptr;          /* the grid medium's voxels (grid_medium.hip): the array DevScene::gmed.rho points at */
    nori_grid_medium_desc grid_desc = {};/* ... its record as stored, rho null (nori_hip_get_grid_medium) */
    float *d_filter = nullptr;
    const uint32_t *d_tri_mesh = nullptr;
    unsigned long long *d_stats = nullptr;
    nori_accel_info info;
    int stack_depth = 32;
    uint64_t lbvh_bytes = 0;
    uint32_t lbvh_refs = 0;      /* references the device builder built the tree over (0: the host built it) */
    uint32_t n_pairs = 0;        /* pair records of the tree in device memory (nori_hip_debug_tree) */
    int engine = -1;                /* -1 auto, 0 megakernel, 1 wavefront */
    int accel_layout = -1;          /* -1 auto (wide from 2^20 triangles), 0 bvh2, 1 bvh4q (wide nodes) */
    bool film_reference = false;    /* film_order = reference: samples added in the reference's own order (film.h) */
    /* 216 B of state each (two copies of the 100-B record + the hit record) + 20 B of film, twice when a call has several batches (the
       sample store's two halves, wavefront.hip "tail overlap"): 2^29 paths = 137 GB of the 288 GB.
       A batch ends with a tail that lasts as long as its longest path (wf_finish: ~19 ms on the pa5 table scene), so fewer,
       bigger batches are cheaper: the table scene at 2048^2 x 1024 spp is 8 batches instead of the 16 of 2^28 */
    size_t wavefront_paths = (size_t) 1 << 29;
    /* camera samples per batch (0: as many as the pool holds paths -- every batch starts all its samples in its first pass, the
       fastest schedule: profiles/r6_12_pool_sweep_two_launches.txt): 20 B each in the film's sample store, twice when a call has several
       batches.  A batch bigger than the pool starts its samples pass by pass in the slots finished paths leave (regeneration,
       wavefront.hip): the pool bounds the STATE, this bounds the film store.  What it is for: a context short of memory keeps its
       batches -- hence the bits of its frame -- on a smaller pool (the out-of-memory retry below), and film_order = reference,
       which needs the frame in ONE batch, runs on any pool */
    size_t wavefront_samples = 0;
    /* render-time resources of THIS context (never shared, freed in nori_hip_destroy): the wavefront
       engine's state pool / streams / events and the film's sample store + tile accumulators */
    WfEngine *wf = nullptr;
    FilmStore film;
    FilmMoments moments;      /* renders that keep second moments, nori_hip_error_map: a second set of tile accumulators, partial sums */
    FilmTiles tiles;          /* renders by tile list, tile selection, the adaptive loop: lists, inverse table, tile errors (film_tiles.h) */
    FilmAlloc alloc;          /* nori_hip_allocate_tiles, nori_hip_render_allocated: levels, done flags, the moving tiles grouped by pair (film_alloc.h) */
    FeatureStore features;    /* nori_hip_render_features: a sample plane and a set of tile accumulators per feature (features.h) */
    DenoiseStore denoise;     /* nori_hip_denoise: the guide records between its two kernels, a buffer per stream (denoise.h) */
    DenoiseErrorStore denoise_error;      /* nori_hip_denoised_error_map: the partial sums of its summary (denoise_error.h) */
};

#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess) {                                                                   \
            (ctx)->error = std::string(#expr) + ": " + hipGetErrorString(e__);                     \
            return e__ == hipErrorOutOfMemory ? NORI_ERR_OUT_OF_MEMORY :                          \
                   (e__ == hipErrorNoDevice || e__ == hipErrorInvalidDevice) ? NORI_ERR_NO_DEVICE : NORI_ERR_INTERNAL; \
        }                                                                                          \
    } while (0)

#define REQUIRE_ACCEL(ctx)                                                                 \
    do {                                                                                   \
        if (!(ctx)) return NORI_ERR_INVALID_ARGUMENT;                                      \
        if (!(ctx)->have_accel) { (ctx)->error = "no acceleration structure built"; return NORI_ERR_NOT_READY; } \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; (void) hipSetDevice(dev); }
    ~DeviceGuard() { if (prev >= 0) (void) hipSetDevice(prev); }
};

/* small RAII device buffer for the host-buffer convenience entry points */
struct Scratch {
    void *p = nullptr;
    ~Scratch() { if (p) (void) hipFree(p); }
};
#define SCRATCH_IN(ctx, var, host, bytes)                                           \
    Scratch var;                                                                    \
    HIP_TRY(ctx, hipMalloc(&var.p, std::max<size_t>((bytes), 16)));                 \
    if (host) HIP_TRY(ctx, hipMemcpy(var.p, host, (bytes), hipMemcpyHostToDevice))
#define SCRATCH_OUT(ctx, var, bytes)                                                \
    Scratch var;                                                                    \
    HIP_TRY(ctx, hipMalloc(&var.p, std::max<size_t>((bytes), 16)))

static inline size_t frame_floats(const nori_hip_ctx *ctx) {
    const int b = ctx->host.filter.border;
    return (size_t) (ctx->host.camera.width + 2 * b) * (size_t) (ctx->host.camera.height + 2 * b) * 4;
}
static inline uint32_t frame_tiles(const nori_hip_ctx *ctx) {
    return (uint32_t) ((ctx->host.camera.width + kTile - 1) / kTile) * (uint32_t) ((ctx->host.camera.height + kTile - 1) / kTile);
}

/* The stats of one render call on stream s, when the caller asked for them (on): the context's counters cleared and an event
   recorded before the work; after it the elapsed time and the counters.  The events are destroyed on every return path. */
struct StatsScope {
    nori_hip_ctx *ctx; hipStream_t s; bool on;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ~StatsScope() { if (ev0) (void) hipEventDestroy(ev0); if (ev1) (void) hipEventDestroy(ev1); }
    int begin() {
        if (!on) return NORI_OK;
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_stats, 0, 16 * sizeof(unsigned long long), s));
        HIP_TRY(ctx, hipEventCreate(&ev0)); HIP_TRY(ctx, hipEventCreate(&ev1));
        HIP_TRY(ctx, hipEventRecord(ev0, s));
        return NORI_OK;
    }
    int end(float &ms, unsigned long long h[16]) {
        HIP_TRY(ctx, hipEventRecord(ev1, s));
        HIP_TRY(ctx, hipEventSynchronize(ev1));
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ev0, ev1));
        HIP_TRY(ctx, hipMemcpy(h, ctx->d_stats, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return NORI_OK;
    }
};

/* the film's view of a launch over all n_sel_tiles selected tiles, their samples from index 0 of the store, n_spp per pixel */
static inline FilmLaunch film_launch_for(uint32_t tiles_x, uint32_t tiles_y, uint32_t n_sel_tiles, uint32_t tile_mod, uint32_t tile_rem, int32_t tile_w,
                                         uint32_t n_spp, const uint32_t *tile_list = nullptr, const uint32_t *tile_inverse = nullptr) {
    FilmLaunch fl;
    fl.tile_first = 0; fl.store_tile_first = 0; fl.n_tiles = n_sel_tiles; fl.tile_mod = tile_mod; fl.tile_rem = tile_rem;
    fl.tiles_x = tiles_x; fl.tiles_y = tiles_y; fl.tile_w = tile_w; fl.n_spp = n_spp; fl.tile_list = tile_list; fl.tile_inverse = tile_inverse;
    return fl;
}

/* environment hooks of the launches shaped like the megakernel's: workgroups to aim for (plan_chunks), the film store's budget in samples (spp_per_launch) */
static inline uint32_t env_target_wgs() { const char *e = getenv("NORI_HIP_TARGET_WGS"); return e ? (uint32_t) std::max(1, atoi(e)) : 16384u; }
static inline size_t env_film_samples() { const char *e = getenv("NORI_HIP_FILM_SAMPLES"); return e ? (size_t) std::max(256ll, atoll(e)) : (size_t) 1 << 29; }

/* env_map.hip: frees the context's environment map and clears DevScene::env (an upload, nori_hip_destroy, a new map) */
void env_release(nori_hip_ctx *ctx);
/* lights.hip: frees the context's delta lights and clears DevScene::lights / n_lights (an upload, nori_hip_destroy, a new set) */
void lights_release(nori_hip_ctx *ctx);
/* grid_medium.hip: frees the context's grid medium and clears DevScene::gmed and, if it was the grid's, DevScene::medium (an upload,
   nori_hip_destroy, a new grid, a homogeneous medium set in its place) */
void grid_medium_release(nori_hip_ctx *ctx);

/* nori_hip.hip.  What a render refuses of its parameters, in order (features: the pass of nori_hip_render_features, which shares three of the
   refusals and has one of its own among them), and of them what a render by tile list refuses.  render_impl: every render -- share: the block rows of a
   reference-order film (accumulators to share->block_acc instead of a frame); d_m2: the samples' second moments are added here; tiles: the tiles of its current list */
int check_render_params(nori_hip_ctx *ctx, const nori_render_params *params, const FilmBlockRows *share, const float *d_m2, const FilmTiles *tiles, bool features = false);
int check_tiles_params(nori_hip_ctx *ctx, const nori_render_params *params, const FilmBlockRows *share);
int render_impl(nori_hip_ctx *ctx, const nori_render_params *params, void *d_rgbw, nori_render_stats *stats, const FilmBlockRows *share,
                float *d_m2 = nullptr, const FilmTiles *tiles = nullptr);
