/* frame_api.hip -- the frame-level half of the C ABI of include/nori_hip.h: nori_hip_render and what is built on it (moments, error map,
 * render to an error, tile lists, selection, the adaptive loop, feature frames, the denoiser, the denoiser with its error and the loop that
 * stops on it, sample levels per tile from a pilot, block rows) and the _host twins.  No kernel lives here: every render ends in render_impl
 * (nori_hip.hip), everything else in film.hip / film_tiles.hip / film_alloc.hip / features.hip / denoise.hip / denoise_error.hip. */
#include <cstring>
#include <initializer_list>
#include "ctx.h"      /* (the HIP runtime, <algorithm>, <string>, <vector>) */
#include "ktimer.h"

#define RC_TRY(expr) do { if (int rc__ = (expr)) return rc__; } while (0)

/* The device side of a _host twin: ONE allocation per call (hipMalloc is slow, and the adaptive CLI path calls these per frame), cut
   into the parts in order (at most 12) and freed on every return path; call(d) gets their device addresses.  A render ADDS into its
   frames, so the render twins ask for zero; the twins that upload zero nothing.  The downloads are blocking copies: behind the
   kernels of the default stream -- a call that queued work on another stream synchronises it itself. */
struct HostPart { size_t bytes; const void *in; void *out; };      /* in: uploaded before the call, out: downloaded after it; NULL: not */
template <class Call>
static int host_twin(nori_hip_ctx *ctx, bool zero, std::initializer_list<HostPart> parts, Call call) {
    DeviceGuard g(ctx->device);
    size_t total = 0;
    for (const HostPart &p : parts) total += p.bytes;
    Scratch buf;
    HIP_TRY(ctx, hipMalloc(&buf.p, std::max<size_t>(total, 16)));
    if (zero) HIP_TRY(ctx, hipMemset(buf.p, 0, total));
    char *d[12], *at = (char *) buf.p;
    int n = 0;
    for (const HostPart &p : parts) { d[n++] = at; if (p.in) HIP_TRY(ctx, hipMemcpy(at, p.in, p.bytes, hipMemcpyHostToDevice)); at += p.bytes; }
    RC_TRY(call(d));
    n = 0;
    for (const HostPart &p : parts) { if (p.out) HIP_TRY(ctx, hipMemcpy(p.out, d[n], p.bytes, hipMemcpyDeviceToHost)); ++n; }
    return NORI_OK;
}
static size_t frame_bytes(const nori_hip_ctx *ctx) { return frame_floats(ctx) * sizeof(float); }
static size_t pixel_bytes(const nori_hip_ctx *ctx) { return (size_t) ctx->host.camera.width * (size_t) ctx->host.camera.height * sizeof(float); }

extern "C" {

int nori_hip_render(nori_hip_ctx *ctx, const nori_render_params *params, void *d_rgbw, nori_render_stats *stats) {
    return render_impl(ctx, params, d_rgbw, stats, nullptr);
}

int nori_hip_render_host(nori_hip_ctx *ctx, const nori_render_params *params, float *rgbw, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !rgbw) return NORI_ERR_INVALID_ARGUMENT;
    nori_render_stats local;
    return host_twin(ctx, true, {{frame_bytes(ctx), nullptr, rgbw}}, [&](char **d) { return nori_hip_render(ctx, params, d[0], stats ? stats : &local); });
}

int nori_hip_render_moments(nori_hip_ctx *ctx, const nori_render_params *params, void *d_rgbw, void *d_m2, nori_render_stats *stats) {
    if (ctx && (!d_rgbw || !d_m2)) { ctx->error = "render_moments: needs an RGBW frame and a moment frame"; return NORI_ERR_INVALID_ARGUMENT; }
    return render_impl(ctx, params, d_rgbw, stats, nullptr, (float *) d_m2);
}

int nori_hip_render_moments_host(nori_hip_ctx *ctx, const nori_render_params *params, float *rgbw, float *m2, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !rgbw || !m2) return NORI_ERR_INVALID_ARGUMENT;
    nori_render_stats local;
    const size_t fb = frame_bytes(ctx);
    return host_twin(ctx, true, {{fb, nullptr, rgbw}, {fb, nullptr, m2}}, [&](char **d) { return nori_hip_render_moments(ctx, params, d[0], d[1], stats ? stats : &local); });
}

int nori_hip_error_map(nori_hip_ctx *ctx, const void *d_rgbw, const void *d_m2, void *d_err, float threshold, nori_error_summary *out, void *stream) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    if (!d_rgbw || !d_m2 || (!d_err && !out)) { ctx->error = "error_map: needs both frames and a map or a summary to fill"; return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    FilmErrorSummary sum;
    const std::string err = film_error_map(ctx->moments, ctx->dev, (const float *) d_rgbw, (const float *) d_m2, (float *) d_err, threshold, out ? &sum : nullptr, stream);
    if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
    if (out) {
        memset(out, 0, sizeof(*out));
        out->sum_err = sum.sum_err; out->max_err = sum.max_err; out->threshold = threshold;
        out->n_pixels = sum.n_pixels; out->n_empty = sum.n_empty; out->n_above = sum.n_above;
    }
    return NORI_OK;
}

int nori_hip_error_map_host(nori_hip_ctx *ctx, const float *rgbw, const float *m2, float *err, float threshold, nori_error_summary *out) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    if (!rgbw || !m2 || (!err && !out)) { ctx->error = "error_map: needs both frames and a map or a summary to fill"; return NORI_ERR_INVALID_ARGUMENT; }
    const size_t fb = frame_bytes(ctx);
    return host_twin(ctx, false, {{fb, rgbw, nullptr}, {fb, m2, nullptr}, {pixel_bytes(ctx), nullptr, err}},
                     [&](char **d) { return nori_hip_error_map(ctx, d[0], d[1], err ? d[2] : nullptr, threshold, out, nullptr); });
}

static void add_stats(nori_render_stats &total, const nori_render_stats &st) {
    total.n_camera_samples += st.n_camera_samples; total.n_closest_rays += st.n_closest_rays; total.n_shadow_rays += st.n_shadow_rays;
    total.n_node_tests += st.n_node_tests; total.n_tri_tests += st.n_tri_tests; total.n_invalid += st.n_invalid;
    total.kernel_ms += st.kernel_ms; total.trace_ms += st.trace_ms; total.shade_ms += st.shade_ms; total.film_ms += st.film_ms; total.tail_ms += st.tail_ms;
    total.n_workgroups += st.n_workgroups; total.n_trace_launches += st.n_trace_launches;
    total.lds_bytes = st.lds_bytes; total.engine = st.engine; total.trace_cus = st.trace_cus; total.tail_cus = st.tail_cus; total.wf_record = st.wf_record;
}

int nori_hip_render_to_error(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t pass_spp, float target_mean_err,
                             void *d_rgbw, void *d_m2, uint32_t *spp_done, nori_error_summary *last, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !d_rgbw || !d_m2) return NORI_ERR_INVALID_ARGUMENT;
    if (pass_spp == 0) { ctx->error = "render_to_error: pass_spp must be at least 1"; return NORI_ERR_INVALID_ARGUMENT; }
    if (!(target_mean_err >= 0.0f)) { ctx->error = "render_to_error: the target error must be a number >= 0"; return NORI_ERR_INVALID_ARGUMENT; }
    if (params->tile_mod != 1) { ctx->error = "render_to_error: renders whole frames (tile_mod 1): the error of a share says nothing about the frame"; return NORI_ERR_INVALID_ARGUMENT; }
    nori_render_stats total; memset(&total, 0, sizeof(total));
    nori_error_summary sum; memset(&sum, 0, sizeof(sum));
    bool evaluated = false;
    uint32_t done = 0, passes = 0;
    while (done < params->spp_count) {
        nori_render_params p = *params;
        p.spp_begin = params->spp_begin + done; p.spp_count = std::min(pass_spp, params->spp_count - done);
        nori_render_stats st;
        RC_TRY(nori_hip_render_moments(ctx, &p, d_rgbw, d_m2, &st));
        add_stats(total, st);
        done += p.spp_count; ++passes;
        evaluated = false;
        if (passes >= 2) {      /* (one pass of few samples has no variance to speak of) */
            RC_TRY(nori_hip_error_map(ctx, d_rgbw, d_m2, nullptr, target_mean_err, &sum, params->stream));
            evaluated = true;
            if (sum.sum_err / (double) sum.n_pixels <= (double) target_mean_err) break;
        }
    }
    if (last) {
        if (!evaluated) RC_TRY(nori_hip_error_map(ctx, d_rgbw, d_m2, nullptr, target_mean_err, &sum, params->stream));
        *last = sum;
    }
    if (spp_done) *spp_done = done;
    if (stats) *stats = total;
    return NORI_OK;
}

/* the error map of the two loops' twins (parts 0, 1, 2 = rgbw, m2, err), if it is asked for: queued on the caller's stream, hence
   the synchronisation before the blocking copies */
static int error_map_for_download(nori_hip_ctx *ctx, char **d, bool wanted, float target, void *stream) {
    if (wanted) { RC_TRY(nori_hip_error_map(ctx, d[0], d[1], d[2], target, nullptr, stream)); HIP_TRY(ctx, hipStreamSynchronize((hipStream_t) stream)); }
    return NORI_OK;
}

int nori_hip_render_to_error_host(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t pass_spp, float target_mean_err,
                                  float *rgbw, float *m2, float *err, uint32_t *spp_done, nori_error_summary *last, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !rgbw) return NORI_ERR_INVALID_ARGUMENT;
    const size_t fb = frame_bytes(ctx);
    return host_twin(ctx, true, {{fb, nullptr, rgbw}, {fb, nullptr, m2}, {pixel_bytes(ctx), nullptr, err}}, [&](char **d) {
        RC_TRY(nori_hip_render_to_error(ctx, params, pass_spp, target_mean_err, d[0], d[1], spp_done, last, stats));
        return error_map_for_download(ctx, d, err != nullptr, target_mean_err, params->stream);
    });
}

/* ---- tile lists, tile errors, selection, the adaptive loop (film_tiles.h) ---- */

/* a host list: strictly ascending raster ids of tiles of the frame */
static int check_tile_list(nori_hip_ctx *ctx, const char *what, const uint32_t *tiles, uint32_t n) {
    const uint32_t n_frame = frame_tiles(ctx);
    if (n && !tiles) { ctx->error = std::string(what) + ": no tile list"; return NORI_ERR_INVALID_ARGUMENT; }
    for (uint32_t i = 0; i < n; ++i) {
        if (tiles[i] >= n_frame) { ctx->error = std::string(what) + ": tile " + std::to_string(tiles[i]) + " (entry " + std::to_string(i) + ") is out of range: the frame has " + std::to_string(n_frame) + " tiles"; return NORI_ERR_INVALID_ARGUMENT; }
        if (i && tiles[i] <= tiles[i - 1]) { ctx->error = std::string(what) + ": the tile list must be strictly ascending (entry " + std::to_string(i) + ": " + std::to_string(tiles[i]) + " after " + std::to_string(tiles[i - 1]) + ")"; return NORI_ERR_INVALID_ARGUMENT; }
    }
    return NORI_OK;
}

int nori_hip_render_tiles(nori_hip_ctx *ctx, const nori_render_params *params, const uint32_t *tiles, uint32_t n_tiles,
                          void *d_rgbw, void *d_m2, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !d_rgbw) return NORI_ERR_INVALID_ARGUMENT;
    RC_TRY(check_tiles_params(ctx, params, nullptr));      /* before the list is looked at: an empty list is refused the same way */
    RC_TRY(check_tile_list(ctx, "render_tiles", tiles, n_tiles));
    if (n_tiles == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return NORI_OK; }      /* nothing is touched */
    DeviceGuard g(ctx->device);
    const std::string err = film_tiles_upload(ctx->tiles, tiles, n_tiles, frame_tiles(ctx), params->stream);
    if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
    return render_impl(ctx, params, d_rgbw, stats, nullptr, (float *) d_m2, &ctx->tiles);
}

int nori_hip_render_tiles_host(nori_hip_ctx *ctx, const nori_render_params *params, const uint32_t *tiles, uint32_t n_tiles,
                               float *rgbw, float *m2, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !rgbw) return NORI_ERR_INVALID_ARGUMENT;
    nori_render_stats local;
    const size_t fb = frame_bytes(ctx);
    return host_twin(ctx, true, {{fb, nullptr, rgbw}, {fb, nullptr, m2}},
                     [&](char **d) { return nori_hip_render_tiles(ctx, params, tiles, n_tiles, d[0], m2 ? d[1] : nullptr, stats ? stats : &local); });
}

int nori_hip_tile_errors(nori_hip_ctx *ctx, const void *d_rgbw, const void *d_m2, void *d_tile_err, void *stream) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    if (!d_rgbw || !d_m2 || !d_tile_err) { ctx->error = "tile_errors: needs both frames and an array to fill"; return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    const std::string err = film_tile_errors(ctx->dev, (const float *) d_rgbw, (const float *) d_m2, (float *) d_tile_err, stream);
    if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
    return NORI_OK;
}

int nori_hip_tile_errors_host(nori_hip_ctx *ctx, const float *rgbw, const float *m2, float *tile_err) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    if (!rgbw || !m2 || !tile_err) { ctx->error = "tile_errors: needs both frames and an array to fill"; return NORI_ERR_INVALID_ARGUMENT; }
    const size_t fb = frame_bytes(ctx);
    return host_twin(ctx, false, {{fb, rgbw, nullptr}, {fb, m2, nullptr}, {(size_t) frame_tiles(ctx) * sizeof(float), nullptr, tile_err}},
                     [&](char **d) { return nori_hip_tile_errors(ctx, d[0], d[1], d[2], nullptr); });
}

int nori_hip_select_tiles(nori_hip_ctx *ctx, const void *d_tile_err, float target, const uint32_t *tiles_in, uint32_t n_in,
                          uint32_t *tiles_out, uint32_t *n_out) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    if (!d_tile_err || !n_out || (n_in && !tiles_out)) { ctx->error = "select_tiles: needs the tile errors, a list to fill and its length"; return NORI_ERR_INVALID_ARGUMENT; }
    RC_TRY(check_tile_list(ctx, "select_tiles", tiles_in, n_in));
    DeviceGuard g(ctx->device);
    std::string err = film_tiles_upload(ctx->tiles, tiles_in, n_in, frame_tiles(ctx), nullptr);
    if (err.empty()) err = film_tiles_select(ctx->tiles, (const float *) d_tile_err, target, frame_tiles(ctx), nullptr);
    if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
    *n_out = ctx->tiles.n;
    if (ctx->tiles.n) HIP_TRY(ctx, hipMemcpy(tiles_out, ctx->tiles.list[ctx->tiles.cur], (size_t) ctx->tiles.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return NORI_OK;
}

int nori_hip_render_adaptive(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t pass_spp, float target_tile_err,
                             void *d_rgbw, void *d_m2, void *d_tile_spp, nori_adaptive_summary *out, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !d_rgbw || !d_m2) return NORI_ERR_INVALID_ARGUMENT;
    if (pass_spp == 0) { ctx->error = "render_adaptive: pass_spp must be at least 1"; return NORI_ERR_INVALID_ARGUMENT; }
    if (!(target_tile_err >= 0.0f)) { ctx->error = "render_adaptive: the target error must be a number >= 0"; return NORI_ERR_INVALID_ARGUMENT; }
    if (params->tile_mod != 1) { ctx->error = "render_adaptive: renders whole frames (tile_mod 1): the loop shares the tiles out itself"; return NORI_ERR_INVALID_ARGUMENT; }
    RC_TRY(check_tiles_params(ctx, params, nullptr));
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t) params->stream;
    FilmTiles &T = ctx->tiles;
    const uint32_t n_frame = frame_tiles(ctx);
    {      /* the active set starts as all tiles */
        std::vector<uint32_t> all(n_frame);
        for (uint32_t i = 0; i < n_frame; ++i) all[i] = i;
        const std::string err = film_tiles_upload(T, all.data(), n_frame, n_frame, s);
        if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
    }
    HIP_TRY(ctx, hipMemsetAsync(T.tile_spp, 0, (size_t) n_frame * sizeof(uint32_t), s));
    nori_render_stats total; memset(&total, 0, sizeof(total));
    uint32_t done = 0, passes = 0;
    bool evaluated = false;
    while (done < params->spp_count && T.n > 0) {
        nori_render_params p = *params;
        p.spp_begin = params->spp_begin + done; p.spp_count = std::min(pass_spp, params->spp_count - done);
        nori_render_stats st;
        RC_TRY(render_impl(ctx, &p, d_rgbw, &st, nullptr, (float *) d_m2, &T));
        add_stats(total, st);
        film_tiles_add_spp(T, T.tile_spp, p.spp_count, s);
        done += p.spp_count; ++passes;
        evaluated = false;
        if (passes >= 2) {      /* (one pass of few samples has no variance to speak of) */
            std::string err = film_tile_errors(ctx->dev, (const float *) d_rgbw, (const float *) d_m2, T.tile_err, s);
            if (err.empty()) err = film_tiles_select(T, T.tile_err, target_tile_err, n_frame, s);
            if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
            evaluated = true;
        }
    }
    if (out) {
        memset(out, 0, sizeof(*out));
        uint32_t n_unconverged = T.n;
        if (!evaluated) {      /* the samples were spent in one pass: the frames as they are left are measured once, without retiring anything */
            std::string err = film_tile_errors(ctx->dev, (const float *) d_rgbw, (const float *) d_m2, T.tile_err, s);
            if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
            std::vector<float> te(n_frame);
            HIP_TRY(ctx, hipMemcpyAsync(te.data(), T.tile_err, (size_t) n_frame * sizeof(float), hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            n_unconverged = 0;
            for (uint32_t i = 0; i < n_frame; ++i) n_unconverged += !(te[i] <= target_tile_err) ? 1u : 0u;
        }
        std::vector<uint32_t> spp(n_frame);
        HIP_TRY(ctx, hipMemcpyAsync(spp.data(), T.tile_spp, (size_t) n_frame * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        out->passes = passes; out->n_tiles = n_frame; out->n_unconverged = n_unconverged;
        out->spp_min = *std::min_element(spp.begin(), spp.end()); out->spp_max = *std::max_element(spp.begin(), spp.end());
        RC_TRY(nori_hip_error_map(ctx, d_rgbw, d_m2, nullptr, target_tile_err, &out->frame, params->stream));
    }
    if (d_tile_spp) HIP_TRY(ctx, hipMemcpyAsync(d_tile_spp, T.tile_spp, (size_t) n_frame * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (stats) *stats = total;
    return NORI_OK;
}

int nori_hip_render_adaptive_host(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t pass_spp, float target_tile_err,
                                  float *rgbw, float *m2, float *err, uint32_t *tile_spp, nori_adaptive_summary *out, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !rgbw) return NORI_ERR_INVALID_ARGUMENT;
    const size_t fb = frame_bytes(ctx);
    return host_twin(ctx, true, {{fb, nullptr, rgbw}, {fb, nullptr, m2}, {pixel_bytes(ctx), nullptr, err}, {(size_t) frame_tiles(ctx) * sizeof(uint32_t), nullptr, tile_spp}}, [&](char **d) {
        RC_TRY(nori_hip_render_adaptive(ctx, params, pass_spp, target_tile_err, d[0], d[1], d[3], out, stats));
        return error_map_for_download(ctx, d, err != nullptr, target_tile_err, params->stream);
    });
}

/* ---- first-hit feature frames (features.h): one trace for all requested features, then the film once per feature ---- */

int nori_hip_render_features(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t features,
                             void *d_albedo, void *d_normal, void *d_depth, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params) return NORI_ERR_INVALID_ARGUMENT;
    void *d_frame[kFeatureCount] = {d_albedo, d_normal, d_depth};
    if (features == 0u || (features & ~kFeatureAll)) { ctx->error = "render_features: the mask must name at least one of NORI_FEATURE_ALBEDO | NORMAL | DEPTH and nothing else"; return NORI_ERR_INVALID_ARGUMENT; }
    for (int f = 0; f < kFeatureCount; ++f)
        if ((features & (1u << f)) && !d_frame[f]) { ctx->error = "render_features: a requested feature has no frame"; return NORI_ERR_INVALID_ARGUMENT; }
    RC_TRY(check_render_params(ctx, params, nullptr, nullptr, nullptr, true));
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t) params->stream;

    /* the tile / chunk geometry of the megakernel path */
    const render_plan::TileGeometry geo = render_plan::tile_geometry(ctx->host.camera.width, ctx->host.camera.height, params->tile_mod, params->tile_rem);
    const int32_t tile_w = render_plan::tile_width(ctx->host.filter.border);
    const uint32_t need = ctx->bvh.max_depth + 1, spp_count = params->spp_count;
    unsigned long long n_invalid = 0; uint32_t n_workgroups = 0;

    StatsScope scope{ctx, s, stats != nullptr};
    RC_TRY(scope.begin());
    KernelTimer timer(stats && params->time_kernels != 0);
    if (geo.n_sel_tiles > 0 && spp_count > 0) {
        /* as the megakernel path of render_impl: a call that produces more samples than the store budget is cut into launches
           over sample sub-ranges, each followed by its gathers; the accumulators are carried from launch to launch */
        const uint32_t spp_per_launch = render_plan::spp_per_launch(spp_count, geo.n_sel_tiles, env_film_samples());
        const size_t n_samples = (size_t) geo.n_sel_tiles * 256 * spp_per_launch;
        FilmStore film;      /* pos, n_parts and the invalid counter are the film's own; always the fast film (no reference order of a feature frame exists) */
        std::string ferr = film_prepare(ctx->film, n_samples, geo.n_sel_tiles, tile_w, s, film);
        if (ferr.empty()) ferr = feature_store_prepare(ctx->features, features, film, n_samples, geo.n_sel_tiles, tile_w, s);
        if (!ferr.empty()) { ctx->error = ferr; return NORI_ERR_OUT_OF_MEMORY; }
        FilmLaunch fl = film_launch_for(geo.tiles_x, geo.tiles_y, geo.n_sel_tiles, params->tile_mod, params->tile_rem, tile_w, 0);
        for (uint32_t sb = 0; sb < spp_count; sb += spp_per_launch) {
            FeatureLaunch pl;
            pl.spp_begin = params->spp_begin + sb; pl.spp_count = std::min(spp_per_launch, spp_count - sb);
            pl.tile_mod = params->tile_mod; pl.tile_rem = params->tile_rem; pl.tiles_x = geo.tiles_x; pl.n_sel_tiles = geo.n_sel_tiles;
            const render_plan::ChunkPlan chunks = render_plan::plan_chunks(geo.n_sel_tiles, pl.spp_count, env_target_wgs());
            pl.n_chunks = chunks.n_chunks; pl.chunk_spp = chunks.chunk_spp; pl.mask = features;
            timer.begin(KC_TRACE, s);
            const hipError_t e = feature_pass_launch(ctx->dev, pl, need, film, ctx->features, ctx->d_stats, s);
            timer.end(s);
            HIP_TRY(ctx, e);
            fl.n_spp = pl.spp_count;
            timer.begin(KC_FILM, s);
            for (int f = 0; f < kFeatureCount; ++f)      /* before the next launch overwrites the store */
                if (features & (1u << f)) film_gather(ctx->dev, ctx->d_filter, feature_view(film, ctx->features, f), fl, s);
            timer.end(s);
            n_workgroups += pl.n_sel_tiles * pl.n_chunks;
        }
        timer.begin(KC_FILM, s);
        for (int f = 0; f < kFeatureCount; ++f)
            if (features & (1u << f)) film_resolve(ctx->dev, feature_view(film, ctx->features, f), fl, (float *) d_frame[f], s);
        timer.end(s);
        HIP_TRY(ctx, hipGetLastError());
        if (stats) n_invalid = film_invalid_count(film, s);
    }
    if (stats) {
        float ms = 0.0f; unsigned long long h[16];
        RC_TRY(scope.end(ms, h));
        memset(stats, 0, sizeof(*stats));
        stats->n_camera_samples = h[0]; stats->n_closest_rays = h[1]; stats->n_invalid = n_invalid;
        stats->kernel_ms = ms; stats->engine = 3u; stats->n_workgroups = n_workgroups;
        float cms[KC_COUNT]; unsigned int cl[KC_COUNT];
        timer.collect(cms, cl);
        stats->trace_ms = cms[KC_TRACE]; stats->film_ms = cms[KC_FILM]; stats->n_trace_launches = cl[KC_TRACE];
        stats->lds_bytes = feature_pass_lds_bytes(need);
    }
    return NORI_OK;
}

int nori_hip_render_features_host(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t features,
                                  float *albedo, float *normal, float *depth, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params) return NORI_ERR_INVALID_ARGUMENT;
    nori_render_stats local;
    const size_t fb = frame_bytes(ctx);
    /* (a frame that is absent gets a NULL device pointer; one that is given but not requested comes back as it went) */
    return host_twin(ctx, true, {{fb, nullptr, (features & 1u) ? albedo : nullptr}, {fb, nullptr, (features & 2u) ? normal : nullptr}, {fb, nullptr, (features & 4u) ? depth : nullptr}}, [&](char **d) {
        return nori_hip_render_features(ctx, params, features, albedo ? d[0] : nullptr, normal ? d[1] : nullptr, depth ? d[2] : nullptr, stats ? stats : &local);
    });
}

/* ---- the denoiser (denoise.h): guide records from the frames, then the NL-means filter over them ---- */

static int denoise_frames_ok(nori_hip_ctx *ctx, const void *rgbw, const void *m2, const void *out, const char *what) {
    if (!rgbw || !m2 || !out) { ctx->error = std::string(what) + ": needs the RGBW frame, the moment frame and a buffer to fill"; return NORI_ERR_INVALID_ARGUMENT; }
    return NORI_OK;
}

/* the launch of step B from the public parameters (NULL: the defaults), or the message of the first one out of range */
static std::string denoise_plan(const nori_denoise_params *params, DenoiseLaunch &dl) {
    const nori_denoise_params def = NORI_DENOISE_PARAMS_DEFAULT;
    const nori_denoise_params p = params ? *params : def;
    if (p.radius < 1u || p.radius > (uint32_t) kDenoiseMaxRadius) return "denoise: the window radius must be 1 .. 8";
    if (p.patch > (uint32_t) kDenoiseMaxPatch) return "denoise: the patch radius must be 0 .. 2";
    if (!(p.k_c > 0.0f)) return "denoise: k_c must be positive";
    if (!(p.alpha >= 0.0f)) return "denoise: alpha must not be negative";
    if (!(p.tau_albedo > 0.0f) || !(p.tau_normal > 0.0f) || !(p.tau_cov > 0.0f)) return "denoise: tau_albedo, tau_normal and tau_cov must be positive";
    if (!(p.k_depth > 0.0f)) return "denoise: k_depth must be positive";
    dl.radius = (int32_t) p.radius; dl.patch = (int32_t) p.patch;
    dl.kc2 = p.k_c * p.k_c; dl.alpha = p.alpha;
    dl.tau_albedo = p.tau_albedo; dl.tau_normal = p.tau_normal;
    dl.kd2 = p.k_depth * p.k_depth; dl.tau_cov = p.tau_cov;
    return std::string();
}

int nori_hip_denoise_guides(nori_hip_ctx *ctx, const void *d_rgbw, const void *d_m2, const void *d_albedo, const void *d_normal,
                            const void *d_depth, void *d_guides, void *stream) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    RC_TRY(denoise_frames_ok(ctx, d_rgbw, d_m2, d_guides, "denoise_guides"));
    DeviceGuard g(ctx->device);
    HIP_TRY(ctx, denoise_guides_launch(ctx->host.camera.width, ctx->host.camera.height, ctx->host.filter.border, (const float *) d_rgbw, (const float *) d_m2,
                                       (const float *) d_albedo, (const float *) d_normal, (const float *) d_depth, (float *) d_guides, stream));
    return NORI_OK;
}

int nori_hip_denoise(nori_hip_ctx *ctx, const nori_denoise_params *params, const void *d_rgbw, const void *d_m2, const void *d_albedo,
                     const void *d_normal, const void *d_depth, void *d_rgb_out, void *d_wsum, void *stream) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    RC_TRY(denoise_frames_ok(ctx, d_rgbw, d_m2, d_rgb_out, "denoise"));
    DenoiseLaunch dl;
    const std::string bad = denoise_plan(params, dl);
    if (!bad.empty()) { ctx->error = bad; return NORI_ERR_INVALID_ARGUMENT; }
    dl.width = ctx->host.camera.width; dl.height = ctx->host.camera.height;
    dl.terms = (d_albedo ? kDenoiseAlbedo : 0u) | (d_normal ? kDenoiseNormal : 0u) | (d_depth ? kDenoiseDepth : 0u);
    DeviceGuard g(ctx->device);
    float *d_guides = nullptr;
    const std::string err = denoise_store_guides(ctx->denoise, stream, (size_t) dl.width * (size_t) dl.height, &d_guides);
    if (!err.empty()) { ctx->error = err; return NORI_ERR_OUT_OF_MEMORY; }
    HIP_TRY(ctx, denoise_guides_launch(dl.width, dl.height, ctx->host.filter.border, (const float *) d_rgbw, (const float *) d_m2, (const float *) d_albedo,
                                       (const float *) d_normal, (const float *) d_depth, d_guides, stream));
    HIP_TRY(ctx, denoise_filter_launch(dl, d_guides, (float *) d_rgb_out, (float *) d_wsum, stream));
    return NORI_OK;
}

/* the host twins: parts 0 .. 4 = rgbw, m2, albedo, normal, depth; the frames that are given are uploaded, the others are NULL to the call */
#define DENOISE_IN {fb, rgbw, nullptr}, {fb, m2, nullptr}, {fb, albedo, nullptr}, {fb, normal, nullptr}, {fb, depth, nullptr}
#define DENOISE_ARGS d[0], d[1], albedo ? d[2] : nullptr, normal ? d[3] : nullptr, depth ? d[4] : nullptr

int nori_hip_denoise_guides_host(nori_hip_ctx *ctx, const float *rgbw, const float *m2, const float *albedo, const float *normal,
                                 const float *depth, float *guides) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    RC_TRY(denoise_frames_ok(ctx, rgbw, m2, guides, "denoise_guides"));
    const size_t fb = frame_bytes(ctx);
    return host_twin(ctx, false, {DENOISE_IN, {pixel_bytes(ctx) * kGuideFloats, nullptr, guides}}, [&](char **d) { return nori_hip_denoise_guides(ctx, DENOISE_ARGS, d[5], nullptr); });
}

int nori_hip_denoise_host(nori_hip_ctx *ctx, const nori_denoise_params *params, const float *rgbw, const float *m2, const float *albedo,
                          const float *normal, const float *depth, float *rgb_out, float *wsum) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    RC_TRY(denoise_frames_ok(ctx, rgbw, m2, rgb_out, "denoise"));
    const size_t fb = frame_bytes(ctx);
    return host_twin(ctx, false, {DENOISE_IN, {3 * pixel_bytes(ctx), nullptr, rgb_out}, {pixel_bytes(ctx), nullptr, wsum}},
                     [&](char **d) { return nori_hip_denoise(ctx, params, DENOISE_ARGS, d[5], wsum ? d[6] : nullptr, nullptr); });
}

/* ---- the denoiser with its output variance, the error of a denoised frame, the loop that stops on it (denoise_error.h) ---- */

/* steps A and B with the variance on `stream`: over the tiles of d_list (DEVICE), or, d_list null, over the whole frame */
static int denoise_var_run(nori_hip_ctx *ctx, DenoiseLaunch dl, const void *d_rgbw, const void *d_m2, const void *d_albedo, const void *d_normal,
                           const void *d_depth, const uint32_t *d_list, uint32_t n_list, void *d_rgb_out, void *d_var_out, void *d_wsum, void *stream) {
    dl.width = ctx->host.camera.width; dl.height = ctx->host.camera.height;
    dl.terms = (d_albedo ? kDenoiseAlbedo : 0u) | (d_normal ? kDenoiseNormal : 0u) | (d_depth ? kDenoiseDepth : 0u);
    float *d_guides = nullptr;
    const std::string err = denoise_store_guides(ctx->denoise, stream, (size_t) dl.width * (size_t) dl.height, &d_guides);
    if (!err.empty()) { ctx->error = err; return NORI_ERR_OUT_OF_MEMORY; }
    HIP_TRY(ctx, denoise_guides_launch(dl.width, dl.height, ctx->host.filter.border, (const float *) d_rgbw, (const float *) d_m2, (const float *) d_albedo,
                                       (const float *) d_normal, (const float *) d_depth, d_guides, stream));
    HIP_TRY(ctx, denoise_filter_var_launch(dl, d_guides, d_list, n_list, (float *) d_rgb_out, (float *) d_var_out, (float *) d_wsum, stream));
    return NORI_OK;
}

int nori_hip_denoise_var(nori_hip_ctx *ctx, const nori_denoise_params *params, const void *d_rgbw, const void *d_m2, const void *d_albedo,
                         const void *d_normal, const void *d_depth, const uint32_t *tiles, uint32_t n_tiles, void *d_rgb_out, void *d_var_out,
                         void *d_wsum, void *stream) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    RC_TRY(denoise_frames_ok(ctx, d_rgbw, d_m2, d_rgb_out, "denoise_var"));
    if (!d_var_out) { ctx->error = "denoise_var: needs a buffer for the variance"; return NORI_ERR_INVALID_ARGUMENT; }
    DenoiseLaunch dl;
    const std::string bad = denoise_plan(params, dl);
    if (!bad.empty()) { ctx->error = bad; return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    const uint32_t *d_list = nullptr;
    if (tiles) {
        RC_TRY(check_tile_list(ctx, "denoise_var", tiles, n_tiles));
        if (n_tiles == 0) return NORI_OK;      /* nothing is touched */
        const std::string err = film_tiles_upload(ctx->tiles, tiles, n_tiles, frame_tiles(ctx), stream);
        if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
        d_list = ctx->tiles.list[ctx->tiles.cur];
    }
    return denoise_var_run(ctx, dl, d_rgbw, d_m2, d_albedo, d_normal, d_depth, d_list, n_tiles, d_rgb_out, d_var_out, d_wsum, stream);
}

int nori_hip_denoise_var_host(nori_hip_ctx *ctx, const nori_denoise_params *params, const float *rgbw, const float *m2, const float *albedo,
                              const float *normal, const float *depth, const uint32_t *tiles, uint32_t n_tiles, float *rgb_out, float *var_out, float *wsum) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    RC_TRY(denoise_frames_ok(ctx, rgbw, m2, rgb_out, "denoise_var"));
    if (!var_out) { ctx->error = "denoise_var: needs a buffer for the variance"; return NORI_ERR_INVALID_ARGUMENT; }
    const size_t fb = frame_bytes(ctx), pb = pixel_bytes(ctx);
    /* (with a list the buffers go up as well as down: the pixels of the other tiles come back as they went) */
    return host_twin(ctx, false, {DENOISE_IN, {3 * pb, tiles ? rgb_out : nullptr, rgb_out}, {3 * pb, tiles ? var_out : nullptr, var_out}, {pb, tiles ? wsum : nullptr, wsum}},
                     [&](char **d) { return nori_hip_denoise_var(ctx, params, DENOISE_ARGS, tiles, n_tiles, d[5], d[6], wsum ? d[7] : nullptr, nullptr); });
}

static int denoised_frames_ok(nori_hip_ctx *ctx, const void *rgb, const void *var, const void *wsum, bool out, const char *what) {
    if (!rgb || !var || !wsum || !out) { ctx->error = std::string(what) + ": needs the denoised frame, its variance, its weight sums and something to fill"; return NORI_ERR_INVALID_ARGUMENT; }
    return NORI_OK;
}

int nori_hip_denoised_error_map(nori_hip_ctx *ctx, const void *d_rgb, const void *d_var, const void *d_wsum, void *d_err, float threshold,
                                nori_error_summary *out, void *stream) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    RC_TRY(denoised_frames_ok(ctx, d_rgb, d_var, d_wsum, d_err || out, "denoised_error_map"));
    DeviceGuard g(ctx->device);
    FilmErrorSummary sum;
    const std::string err = denoised_error_map(ctx->denoise_error, ctx->host.camera.width, ctx->host.camera.height, (const float *) d_rgb, (const float *) d_var,
                                               (const float *) d_wsum, (float *) d_err, threshold, out ? &sum : nullptr, stream);
    if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
    if (out) {
        memset(out, 0, sizeof(*out));
        out->sum_err = sum.sum_err; out->max_err = sum.max_err; out->threshold = threshold;
        out->n_pixels = sum.n_pixels; out->n_empty = sum.n_empty; out->n_above = sum.n_above;
    }
    return NORI_OK;
}

int nori_hip_denoised_error_map_host(nori_hip_ctx *ctx, const float *rgb, const float *var, const float *wsum, float *err, float threshold, nori_error_summary *out) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    RC_TRY(denoised_frames_ok(ctx, rgb, var, wsum, err || out, "denoised_error_map"));
    const size_t pb = pixel_bytes(ctx);
    return host_twin(ctx, false, {{3 * pb, rgb, nullptr}, {3 * pb, var, nullptr}, {pb, wsum, nullptr}, {pb, nullptr, err}},
                     [&](char **d) { return nori_hip_denoised_error_map(ctx, d[0], d[1], d[2], err ? d[3] : nullptr, threshold, out, nullptr); });
}

int nori_hip_denoised_tile_errors(nori_hip_ctx *ctx, const void *d_rgb, const void *d_var, const void *d_wsum, void *d_tile_err, void *stream) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    RC_TRY(denoised_frames_ok(ctx, d_rgb, d_var, d_wsum, d_tile_err != nullptr, "denoised_tile_errors"));
    DeviceGuard g(ctx->device);
    const std::string err = denoised_tile_errors(ctx->host.camera.width, ctx->host.camera.height, (const float *) d_rgb, (const float *) d_var, (const float *) d_wsum,
                                                 (float *) d_tile_err, stream);
    if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
    return NORI_OK;
}

int nori_hip_denoised_tile_errors_host(nori_hip_ctx *ctx, const float *rgb, const float *var, const float *wsum, float *tile_err) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    RC_TRY(denoised_frames_ok(ctx, rgb, var, wsum, tile_err != nullptr, "denoised_tile_errors"));
    const size_t pb = pixel_bytes(ctx);
    return host_twin(ctx, false, {{3 * pb, rgb, nullptr}, {3 * pb, var, nullptr}, {pb, wsum, nullptr}, {(size_t) frame_tiles(ctx) * sizeof(float), nullptr, tile_err}},
                     [&](char **d) { return nori_hip_denoised_tile_errors(ctx, d[0], d[1], d[2], d[3], nullptr); });
}

int nori_hip_render_adaptive_denoised(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t pass_spp, float target_tile_err,
                                      const nori_denoise_params *denoise_params, void *d_rgbw, void *d_m2, const void *d_albedo, const void *d_normal,
                                      const void *d_depth, void *d_rgb_out, void *d_var_out, void *d_wsum, void *d_tile_spp,
                                      nori_adaptive_summary *out, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !d_rgbw || !d_m2) return NORI_ERR_INVALID_ARGUMENT;
    if (!d_rgb_out || !d_var_out || !d_wsum) { ctx->error = "render_adaptive_denoised: needs buffers for the denoised frame, its variance and its weight sums"; return NORI_ERR_INVALID_ARGUMENT; }
    if (pass_spp == 0) { ctx->error = "render_adaptive_denoised: pass_spp must be at least 1"; return NORI_ERR_INVALID_ARGUMENT; }
    if (!(target_tile_err >= 0.0f)) { ctx->error = "render_adaptive_denoised: the target error must be a number >= 0"; return NORI_ERR_INVALID_ARGUMENT; }
    if (params->tile_mod != 1) { ctx->error = "render_adaptive_denoised: renders whole frames (tile_mod 1): the loop shares the tiles out itself"; return NORI_ERR_INVALID_ARGUMENT; }
    RC_TRY(check_tiles_params(ctx, params, nullptr));
    DenoiseLaunch dl;
    const std::string bad = denoise_plan(denoise_params, dl);
    if (!bad.empty()) { ctx->error = bad; return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t) params->stream;
    FilmTiles &T = ctx->tiles;
    const uint32_t n_frame = frame_tiles(ctx);
    const size_t n_pixels = (size_t) ctx->host.camera.width * (size_t) ctx->host.camera.height;
    {      /* the active set starts as all tiles */
        std::vector<uint32_t> all(n_frame);
        for (uint32_t i = 0; i < n_frame; ++i) all[i] = i;
        const std::string err = film_tiles_upload(T, all.data(), n_frame, n_frame, s);
        if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
    }
    HIP_TRY(ctx, hipMemsetAsync(T.tile_spp, 0, (size_t) n_frame * sizeof(uint32_t), s));
    HIP_TRY(ctx, hipMemsetAsync(d_rgb_out, 0, n_pixels * 3 * sizeof(float), s));
    HIP_TRY(ctx, hipMemsetAsync(d_var_out, 0, n_pixels * 3 * sizeof(float), s));
    HIP_TRY(ctx, hipMemsetAsync(d_wsum, 0, n_pixels * sizeof(float), s));
    auto tile_errors = [&]() -> int {      /* of the outputs as they stand, into T.tile_err */
        const std::string err = denoised_tile_errors(ctx->host.camera.width, ctx->host.camera.height, (const float *) d_rgb_out, (const float *) d_var_out,
                                                     (const float *) d_wsum, T.tile_err, s);
        if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
        return NORI_OK;
    };
    nori_render_stats total; memset(&total, 0, sizeof(total));
    uint32_t done = 0, passes = 0;
    while (done < params->spp_count && T.n > 0) {
        nori_render_params p = *params;
        p.spp_begin = params->spp_begin + done; p.spp_count = std::min(pass_spp, params->spp_count - done);
        nori_render_stats st;
        RC_TRY(render_impl(ctx, &p, d_rgbw, &st, nullptr, (float *) d_m2, &T));
        add_stats(total, st);
        film_tiles_add_spp(T, T.tile_spp, p.spp_count, s);
        done += p.spp_count; ++passes;
        if (passes >= 2) {      /* (one pass of few samples has no variance to speak of) */
            /* guide records of the whole frame, the filter over the active tiles alone: the list as the selection left it on the device */
            RC_TRY(denoise_var_run(ctx, dl, d_rgbw, d_m2, d_albedo, d_normal, d_depth, T.list[T.cur], T.n, d_rgb_out, d_var_out, d_wsum, s));
            RC_TRY(tile_errors());
            const std::string err = film_tiles_select(T, T.tile_err, target_tile_err, n_frame, s);
            if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
        }
    }
    /* the outputs: the whole frame once more -- the neighbours of a retired tile have changed since it was last filtered */
    RC_TRY(denoise_var_run(ctx, dl, d_rgbw, d_m2, d_albedo, d_normal, d_depth, nullptr, 0, d_rgb_out, d_var_out, d_wsum, s));
    if (out) {
        memset(out, 0, sizeof(*out));
        uint32_t n_unconverged = T.n;
        if (passes < 2) {      /* no evaluation was made: the final frame is measured once, without retiring anything */
            RC_TRY(tile_errors());
            std::vector<float> te(n_frame);
            HIP_TRY(ctx, hipMemcpyAsync(te.data(), T.tile_err, (size_t) n_frame * sizeof(float), hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            n_unconverged = 0;
            for (uint32_t i = 0; i < n_frame; ++i) n_unconverged += !(te[i] <= target_tile_err) ? 1u : 0u;
        }
        std::vector<uint32_t> spp(n_frame);
        HIP_TRY(ctx, hipMemcpyAsync(spp.data(), T.tile_spp, (size_t) n_frame * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        out->passes = passes; out->n_tiles = n_frame; out->n_unconverged = n_unconverged;
        out->spp_min = *std::min_element(spp.begin(), spp.end()); out->spp_max = *std::max_element(spp.begin(), spp.end());
        RC_TRY(nori_hip_denoised_error_map(ctx, d_rgb_out, d_var_out, d_wsum, nullptr, target_tile_err, &out->frame, params->stream));
    }
    if (d_tile_spp) HIP_TRY(ctx, hipMemcpyAsync(d_tile_spp, T.tile_spp, (size_t) n_frame * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (stats) *stats = total;
    return NORI_OK;
}

int nori_hip_render_adaptive_denoised_host(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t pass_spp, float target_tile_err,
                                           const nori_denoise_params *denoise_params, float *rgbw, float *m2, const float *albedo, const float *normal,
                                           const float *depth, float *rgb_out, float *var_out, float *wsum, float *err, uint32_t *tile_spp,
                                           nori_adaptive_summary *out, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !rgbw || !rgb_out) return NORI_ERR_INVALID_ARGUMENT;
    const size_t fb = frame_bytes(ctx), pb = pixel_bytes(ctx);
    /* parts 0 .. 9 = rgbw, m2, albedo, normal, depth, rgb_out, var_out, wsum, err, tile_spp */
    return host_twin(ctx, true, {{fb, nullptr, rgbw}, {fb, nullptr, m2}, {fb, albedo, nullptr}, {fb, normal, nullptr}, {fb, depth, nullptr}, {3 * pb, nullptr, rgb_out},
                                 {3 * pb, nullptr, var_out}, {pb, nullptr, wsum}, {pb, nullptr, err}, {(size_t) frame_tiles(ctx) * sizeof(uint32_t), nullptr, tile_spp}}, [&](char **d) -> int {
        RC_TRY(nori_hip_render_adaptive_denoised(ctx, params, pass_spp, target_tile_err, denoise_params, d[0], d[1], albedo ? d[2] : nullptr, normal ? d[3] : nullptr,
                                                 depth ? d[4] : nullptr, d[5], d[6], d[7], d[9], out, stats));
        if (err) { RC_TRY(nori_hip_denoised_error_map(ctx, d[5], d[6], d[7], d[8], target_tile_err, nullptr, params->stream)); HIP_TRY(ctx, hipStreamSynchronize((hipStream_t) params->stream)); }
        return NORI_OK;
    });
}

/* ---- sample levels per tile from a pilot (film_alloc.h): nori_hip_allocate_tiles, nori_hip_render_allocated ---- */

static int check_allocate(nori_hip_ctx *ctx, const char *what, const nori_allocate_params *ap, uint32_t spp_count, AllocLevels &lv) {
    const std::string w(what);
    if (!ap) { ctx->error = w + ": no nori_allocate_params"; return NORI_ERR_INVALID_ARGUMENT; }
    if (ap->pilot_spp < 2u) { ctx->error = w + ": pilot_spp must be at least 2 (one sample has no variance)"; return NORI_ERR_INVALID_ARGUMENT; }
    if (ap->max_rounds < 1u) { ctx->error = w + ": max_rounds must be at least 1"; return NORI_ERR_INVALID_ARGUMENT; }
    if (!(ap->target_tile_err >= 0.0f)) { ctx->error = w + ": the target error must be a number >= 0"; return NORI_ERR_INVALID_ARGUMENT; }
    if (!(ap->headroom >= 1.0f)) { ctx->error = w + ": headroom must be a number >= 1"; return NORI_ERR_INVALID_ARGUMENT; }
    if (ap->metric != 0 && ap->metric != 1) { ctx->error = w + ": metric must be 0 (raw) or 1 (denoised)"; return NORI_ERR_INVALID_ARGUMENT; }
    if (!alloc_levels(ap->pilot_spp, spp_count, lv)) { ctx->error = w + ": spp_count (the most a pixel may get) must be at least pilot_spp"; return NORI_ERR_INVALID_ARGUMENT; }
    return NORI_OK;
}

int nori_hip_allocate_tiles(nori_hip_ctx *ctx, const nori_allocate_params *alloc, uint32_t spp_count, const void *d_tile_err,
                            uint32_t *level, uint32_t *done, uint32_t *tiles_out, uint32_t *bucket_begin) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    if (!d_tile_err || !level || !done || !tiles_out || !bucket_begin) { ctx->error = "allocate_tiles: needs the tile errors, levels, done flags, a list and bucket_begin to fill"; return NORI_ERR_INVALID_ARGUMENT; }
    AllocLevels lv;
    RC_TRY(check_allocate(ctx, "allocate_tiles", alloc, spp_count, lv));
    const uint32_t n_frame = frame_tiles(ctx);
    for (uint32_t t = 0; t < n_frame; ++t)
        if (level[t] > lv.J) { ctx->error = "allocate_tiles: tile " + std::to_string(t) + " is at level " + std::to_string(level[t]) + ", the top level is " + std::to_string(lv.J); return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    FilmAlloc &A = ctx->alloc;
    const std::string err0 = film_alloc_reserve(A, n_frame);
    if (!err0.empty()) { ctx->error = err0; return NORI_ERR_OUT_OF_MEMORY; }
    std::vector<uint32_t> flags(n_frame);
    for (uint32_t t = 0; t < n_frame; ++t) flags[t] = done[t] ? 1u : 0u;
    const size_t words = (size_t) n_frame * sizeof(uint32_t);
    HIP_TRY(ctx, hipMemcpy(A.level, level, words, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(A.done, flags.data(), words, hipMemcpyHostToDevice));
    uint32_t begin[kAllocMaxBuckets + 1];
    const std::string err = film_alloc_round(A, (const float *) d_tile_err, alloc->target_tile_err, alloc->headroom, lv, n_frame, begin, nullptr);
    if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
    HIP_TRY(ctx, hipMemcpy(level, A.level, words, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(done, A.done, words, hipMemcpyDeviceToHost));
    const uint32_t n_moving = begin[kAllocMaxBuckets];
    if (n_moving) HIP_TRY(ctx, hipMemcpy(tiles_out, A.list, (size_t) n_moving * sizeof(uint32_t), hipMemcpyDeviceToHost));
    memcpy(bucket_begin, begin, sizeof(begin));
    return NORI_OK;
}

int nori_hip_render_allocated(nori_hip_ctx *ctx, const nori_render_params *params, const nori_allocate_params *alloc,
                              const nori_denoise_params *denoise_params, void *d_rgbw, void *d_m2, const void *d_albedo, const void *d_normal,
                              const void *d_depth, void *d_rgb_out, void *d_var_out, void *d_wsum, void *d_tile_spp, void *d_level_log,
                              nori_adaptive_summary *out, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !d_rgbw || !d_m2) return NORI_ERR_INVALID_ARGUMENT;
    AllocLevels lv;
    RC_TRY(check_allocate(ctx, "render_allocated", alloc, params->spp_count, lv));
    const bool denoised = alloc->metric == 1;
    if (denoised && (!d_rgb_out || !d_var_out || !d_wsum)) { ctx->error = "render_allocated: metric 1 needs buffers for the denoised frame, its variance and its weight sums"; return NORI_ERR_INVALID_ARGUMENT; }
    if (params->tile_mod != 1) { ctx->error = "render_allocated: renders whole frames (tile_mod 1): the loop shares the tiles out itself"; return NORI_ERR_INVALID_ARGUMENT; }
    RC_TRY(check_tiles_params(ctx, params, nullptr));
    DenoiseLaunch dl;
    if (denoised) {
        const std::string bad = denoise_plan(denoise_params, dl);
        if (!bad.empty()) { ctx->error = bad; return NORI_ERR_INVALID_ARGUMENT; }
    }
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t) params->stream;
    FilmTiles &T = ctx->tiles;
    FilmAlloc &A = ctx->alloc;
    const uint32_t n_frame = frame_tiles(ctx);
    const size_t words = (size_t) n_frame * sizeof(uint32_t);
    const size_t n_pixels = (size_t) ctx->host.camera.width * (size_t) ctx->host.camera.height;
    {
        std::string err = film_tiles_reserve(T, n_frame);      /* the inverse table and the tile errors are the context's */
        if (err.empty()) err = film_alloc_reserve(A, n_frame);
        if (!err.empty()) { ctx->error = err; return NORI_ERR_OUT_OF_MEMORY; }
    }
    HIP_TRY(ctx, hipMemsetAsync(A.level, 0, words, s));
    HIP_TRY(ctx, hipMemsetAsync(A.done, 0, words, s));
    if (denoised) {
        HIP_TRY(ctx, hipMemsetAsync(d_rgb_out, 0, n_pixels * 3 * sizeof(float), s));
        HIP_TRY(ctx, hipMemsetAsync(d_var_out, 0, n_pixels * 3 * sizeof(float), s));
        HIP_TRY(ctx, hipMemsetAsync(d_wsum, 0, n_pixels * sizeof(float), s));
    }
    auto log_levels = [&](uint32_t row) -> int {
        if (d_level_log) HIP_TRY(ctx, hipMemcpyAsync((uint32_t *) d_level_log + (size_t) row * n_frame, A.level, words, hipMemcpyDeviceToDevice, s));
        return NORI_OK;
    };
    /* the tile errors of the frames as they are, into T.tile_err; metric 1: step A, then the filter over d_list (null: the whole frame) */
    auto evaluate = [&](const uint32_t *d_list, uint32_t n_list) -> int {
        std::string err;
        if (denoised) {
            RC_TRY(denoise_var_run(ctx, dl, d_rgbw, d_m2, d_albedo, d_normal, d_depth, d_list, n_list, d_rgb_out, d_var_out, d_wsum, s));
            err = denoised_tile_errors(ctx->host.camera.width, ctx->host.camera.height, (const float *) d_rgb_out, (const float *) d_var_out, (const float *) d_wsum, T.tile_err, s);
        } else
            err = film_tile_errors(ctx->dev, (const float *) d_rgbw, (const float *) d_m2, T.tile_err, s);
        if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
        return NORI_OK;
    };
    nori_render_stats total; memset(&total, 0, sizeof(total));
    uint32_t passes = 0, rounds = 0;
    {      /* the pilot: every tile, level 0 */
        nori_render_params p = *params;
        p.spp_count = lv.spp[0];
        nori_render_stats st;
        RC_TRY(render_impl(ctx, &p, d_rgbw, &st, nullptr, (float *) d_m2));
        add_stats(total, st);
        ++passes;
        RC_TRY(log_levels(0));
    }
    uint32_t n_active = n_frame;      /* tiles not done: all of them, then the tiles the last round moved (A.list, whole) */
    bool fresh = false;               /* T.tile_err is of the frames as they are */
    while (rounds < alloc->max_rounds) {
        RC_TRY(evaluate(rounds == 0 ? nullptr : A.list, rounds == 0 ? 0u : n_active));
        uint32_t begin[kAllocMaxBuckets + 1];
        const std::string err = film_alloc_round(A, T.tile_err, alloc->target_tile_err, alloc->headroom, lv, n_frame, begin, s);
        if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
        n_active = begin[kAllocMaxBuckets];
        fresh = !denoised;      /* (metric 1: only the tiles not done were filtered) */
        if (n_active == 0) break;
        for (uint32_t i = 0; i < lv.J; ++i)
            for (uint32_t j = i + 1; j <= lv.J; ++j) {
                const uint32_t b = alloc_bucket(lv.J, i, j), n_b = begin[b + 1] - begin[b];
                if (n_b == 0) continue;
                const std::string ierr = film_alloc_inverse(A, begin[b], n_b, T.inverse, n_frame, s);
                if (!ierr.empty()) { ctx->error = ierr; return NORI_ERR_INTERNAL; }
                FilmTiles view;      /* the bucket's slice as a render's current list; owns nothing */
                view.list[0] = A.list + begin[b]; view.inverse = T.inverse; view.capacity = T.capacity; view.cur = 0; view.n = n_b;
                nori_render_params p = *params;
                p.spp_begin = params->spp_begin + lv.spp[i]; p.spp_count = lv.spp[j] - lv.spp[i];
                nori_render_stats st;
                RC_TRY(render_impl(ctx, &p, d_rgbw, &st, nullptr, (float *) d_m2, &view));
                add_stats(total, st);
                ++passes;
            }
        T.n = 0;      /* the context's own list does not describe the inverse table any more */
        fresh = false;
        ++rounds;
        RC_TRY(log_levels(rounds));
    }
    for (uint32_t r = rounds + 1; r <= alloc->max_rounds; ++r) RC_TRY(log_levels(r));      /* rounds that did not run: the levels as they were left */
    /* one more evaluation for the summary (metric 1: the filter over the whole frame, so the outputs are denoise_var of the frames as they are left) */
    if (denoised || (out && !fresh)) RC_TRY(evaluate(nullptr, 0));
    if (d_tile_spp) {
        const std::string err = film_alloc_tile_spp(A, lv, (uint32_t *) d_tile_spp, n_frame, s);
        if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
    }
    if (out) {
        memset(out, 0, sizeof(*out));
        std::vector<float> te(n_frame);
        std::vector<uint32_t> level(n_frame);
        HIP_TRY(ctx, hipMemcpyAsync(te.data(), T.tile_err, (size_t) n_frame * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipMemcpyAsync(level.data(), A.level, words, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        uint32_t n_unconverged = 0;
        for (uint32_t i = 0; i < n_frame; ++i) n_unconverged += !(te[i] <= alloc->target_tile_err) ? 1u : 0u;
        out->passes = passes; out->n_tiles = n_frame; out->n_unconverged = n_unconverged;
        out->spp_min = lv.spp[*std::min_element(level.begin(), level.end())]; out->spp_max = lv.spp[*std::max_element(level.begin(), level.end())];
        if (denoised) RC_TRY(nori_hip_denoised_error_map(ctx, d_rgb_out, d_var_out, d_wsum, nullptr, alloc->target_tile_err, &out->frame, params->stream));
        else RC_TRY(nori_hip_error_map(ctx, d_rgbw, d_m2, nullptr, alloc->target_tile_err, &out->frame, params->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (stats) *stats = total;
    return NORI_OK;
}

int nori_hip_render_allocated_host(nori_hip_ctx *ctx, const nori_render_params *params, const nori_allocate_params *alloc,
                                   const nori_denoise_params *denoise_params, float *rgbw, float *m2, const float *albedo, const float *normal,
                                   const float *depth, float *rgb_out, float *var_out, float *wsum, float *err, uint32_t *tile_spp,
                                   uint32_t *level_log, nori_adaptive_summary *out, nori_render_stats *stats) {
    REQUIRE_ACCEL(ctx);
    if (!params || !rgbw || !alloc) return NORI_ERR_INVALID_ARGUMENT;
    const bool denoised = alloc->metric == 1;
    if (denoised && !rgb_out) { ctx->error = "render_allocated: metric 1 needs a buffer for the denoised frame"; return NORI_ERR_INVALID_ARGUMENT; }
    const size_t fb = frame_bytes(ctx), pb = pixel_bytes(ctx), tb = (size_t) frame_tiles(ctx) * sizeof(uint32_t);
    const size_t dn = denoised ? 1 : 0;      /* (metric 0: the denoiser's parts are empty) */
    /* parts 0 .. 10 = rgbw, m2, albedo, normal, depth, rgb_out, var_out, wsum, err, tile_spp, level_log */
    return host_twin(ctx, true, {{fb, nullptr, rgbw}, {fb, nullptr, m2}, {dn * fb, dn ? albedo : nullptr, nullptr}, {dn * fb, dn ? normal : nullptr, nullptr},
                                 {dn * fb, dn ? depth : nullptr, nullptr}, {dn * 3 * pb, nullptr, dn ? rgb_out : nullptr}, {dn * 3 * pb, nullptr, dn ? var_out : nullptr},
                                 {dn * pb, nullptr, dn ? wsum : nullptr}, {pb, nullptr, err}, {tb, nullptr, tile_spp},
                                 {level_log ? ((size_t) alloc->max_rounds + 1) * tb : 0, nullptr, level_log}}, [&](char **d) -> int {
        RC_TRY(nori_hip_render_allocated(ctx, params, alloc, denoise_params, d[0], d[1], dn && albedo ? d[2] : nullptr, dn && normal ? d[3] : nullptr,
                                         dn && depth ? d[4] : nullptr, dn ? d[5] : nullptr, dn ? d[6] : nullptr, dn ? d[7] : nullptr, d[9], level_log ? d[10] : nullptr, out, stats));
        if (err) {
            if (denoised) RC_TRY(nori_hip_denoised_error_map(ctx, d[5], d[6], d[7], d[8], alloc->target_tile_err, nullptr, params->stream));
            else RC_TRY(nori_hip_error_map(ctx, d[0], d[1], d[8], alloc->target_tile_err, nullptr, params->stream));
            HIP_TRY(ctx, hipStreamSynchronize((hipStream_t) params->stream));
        }
        return NORI_OK;
    });
}

int nori_hip_block_acc_floats(nori_hip_ctx *ctx, size_t *n_floats) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    if (!n_floats) return NORI_ERR_INVALID_ARGUMENT;
    *n_floats = film_block_acc_floats(ctx->dev);
    return NORI_OK;
}

int nori_hip_render_block_rows(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t row_begin, uint32_t row_count,
                               void *d_block_acc, nori_render_stats *stats) {
    FilmBlockRows share;
    share.row_begin = row_begin; share.row_count = row_count; share.block_acc = (float *) d_block_acc;
    return render_impl(ctx, params, nullptr, stats, &share);
}

int nori_hip_resolve_blocks(nori_hip_ctx *ctx, const void *d_block_acc, void *d_rgbw, void *stream) {
    if (!ctx || !ctx->have_scene) return NORI_ERR_NOT_READY;
    if (!d_block_acc || !d_rgbw) return NORI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    const std::string err = film_resolve_blocks(ctx->film, ctx->dev, (const float *) d_block_acc, (float *) d_rgbw, (hipStream_t) stream);
    if (!err.empty()) { ctx->error = err; return NORI_ERR_INTERNAL; }
    return NORI_OK;
}

} // extern "C"
