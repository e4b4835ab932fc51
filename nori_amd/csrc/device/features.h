/*
 * features.h -- first-hit feature frames: albedo, shading normal and depth of the first surface a camera sample sees
 * (include/nori_hip.h, nori_hip_render_features).  What a denoiser is guided by; no counterpart in the reference.
 *
 * A pass of its own, in a translation unit of its own (features.hip): one closest-hit ray per camera sample, the camera
 * sample being the one render_kernel and first_vertex draw.  Nothing of the path tracer's kernels is touched -- their
 * registers, LDS and bits stay what they are.
 *   feature_pass_kernel   one 256-thread workgroup per (tile ordinal, chunk of samples); thread = pixel_in_tile in
 *                         film_tile_pixel's 8x8-quad numbering, so a wave traces an 8x8 pixel quad (coherent rays).  The
 *                         thread loops over the samples of its chunk: pcg32 -> pixelSample -> camera_sample_ray -> the generic
 *                         traverse<false> (rt_trace.h: 64-B BVH2 nodes or wide nodes, either builder) over an LDS stack sized
 *                         to the tree (16 / 24 / 32 / 64 entries), then first_hit_features below.  pos and the requested
 *                         planes go to the film store's index (ordinal * n_spp + s) * 256 + pixel: consecutive lanes write
 *                         consecutive addresses (8 B pos, 12 B per plane).  Pixels of edge tiles outside the frame trace and
 *                         write nothing, as in render_kernel: the film's gathers never read their slots.
 * The film is the existing one: per requested feature film_gather runs on a VIEW of the context's FilmStore whose L names
 * that feature's plane and whose tile_acc names that feature's accumulator set (the device of FilmMoments), then
 * film_resolve adds each set into that feature's frame.  The planes and accumulator sets are the context's FeatureStore.
 */
#pragma once
#include <string>

#include "film.h"
#include "rt_sampling.h"
#include "rt_texture.h"
#include "rt_trace.h"

namespace nrt {

constexpr uint32_t kFeatureAlbedo = 1u, kFeatureNormal = 2u, kFeatureDepth = 4u, kFeatureAll = 7u;      /* nori_feature */
constexpr int kFeatureCount = 3;      /* plane / accumulator set f belongs to bit 1 << f */

/* The three values of one camera sample whose closest-hit query gave `hit` (found: something was hit); float32, no FMA
 * contraction.  include/nori_hip.h states the same, operation by operation.
 *   albedo  miss (0, 0, 0); mirror and dielectric (1, 1, 1); else the mesh's bsdf.albedo (diffuse: albedo, microfacet: kd), or
 *           -- a textured mesh -- texture_lookup at the hit's uv, exactly as path_on_closest reads it.  An emitter is a mesh
 *           like any other.
 *   normal  0.5f * n + 0.5f per component of the shading normal n (its.shFrame.n: what nori_hip_intersect returns as sh_n);
 *           miss (0.5, 0.5, 0.5).  Encoded because the film's isValid() guard drops samples with a negative component.
 *   depth   (t, float32(t * t), 1) with t the hit's distance; miss (0, 0, 0).  The third channel is coverage. */
NORI_HD void first_hit_features(const DevScene &sc, const Hit &hit, bool found, uint32_t mask, P3 &albedo, P3 &normal, P3 &depth) {
    albedo.x = albedo.y = albedo.z = 0.0f;
    normal.x = normal.y = normal.z = 0.5f;
    depth.x = depth.y = depth.z = 0.0f;
    if (!found) return;
    const MeshRec &m = sc.meshes[hit.mesh];
    if (mask & kFeatureAlbedo) {
        f3 a = mk3(1.0f);
        if (m.bsdf_type != 1 && m.bsdf_type != 2) {      /* not NORI_BSDF_MIRROR, NORI_BSDF_DIELECTRIC */
            a = mk3(m.albedo[0], m.albedo[1], m.albedo[2]);
            if (m.flags & kMeshTextured) a = texture_lookup(sc.textures[m.pad[0] - 1u], sc.texels, hit_uv(sc, m.flags, hit));
        }
        albedo.x = a.x; albedo.y = a.y; albedo.z = a.z;
    }
    if (mask & kFeatureNormal) {
        Surface sf;
        surface_fill(sc, hit, sf, nullptr, nullptr);
        normal.x = 0.5f * sf.ns.x + 0.5f; normal.y = 0.5f * sf.ns.y + 0.5f; normal.z = 0.5f * sf.ns.z + 0.5f;
    }
    if (mask & kFeatureDepth) { depth.x = hit.t; depth.y = hit.t * hit.t; depth.z = 1.0f; }
}

/* What a context holds for feature frames beside its FilmStore (which a plain render uses as before): one sample plane and
   one set of tile accumulators (layout of FilmStore::tile_acc) per feature, allocated when the feature is first asked for. */
struct FeatureStore {
    P3 *plane[kFeatureCount] = {nullptr, nullptr, nullptr};
    size_t capacity[kFeatureCount] = {0, 0, 0};       /* samples */
    float *tile_acc[kFeatureCount] = {nullptr, nullptr, nullptr};
    size_t acc_floats[kFeatureCount] = {0, 0, 0};
};

struct FeatureLaunch {
    uint32_t spp_begin, spp_count;      /* the samples of THIS launch: the store holds spp_count per pixel */
    uint32_t tile_mod, tile_rem, tiles_x;
    uint32_t n_sel_tiles;
    uint32_t n_chunks, chunk_spp;       /* workgroups per tile, samples per workgroup (plan_chunks, nori_hip.hip) */
    uint32_t mask;                      /* planes to store */
};

/* after film_prepare of the same call: (re)allocates the planes of `mask` for n_samples and its accumulator sets for the
   view's n_parts, and zeroes those sets.  "" or an error. */
std::string feature_store_prepare(FeatureStore &fs, uint32_t mask, const FilmStore &view, size_t n_samples, size_t n_sel_tiles, int tile_w, void *stream);
void feature_store_release(FeatureStore &fs);
/* the view of `film` that gathers and resolves feature f */
inline FilmStore feature_view(const FilmStore &film, const FeatureStore &fs, int f) {
    FilmStore v = film; v.L = fs.plane[f]; v.tile_acc = fs.tile_acc[f];
    return v;
}
/* LDS of one workgroup of the pass for a tree that needs `stack_need` stack entries */
uint32_t feature_pass_lds_bytes(uint32_t stack_need);
/* one launch of the pass: pos into film.pos, the planes of fl.mask into fs; stats[0] += camera samples, stats[1] += closest-hit rays */
hipError_t feature_pass_launch(const DevScene &sc, const FeatureLaunch &fl, uint32_t stack_need, const FilmStore &film, const FeatureStore &fs,
                               unsigned long long *d_stats, void *stream);

} // namespace nrt
