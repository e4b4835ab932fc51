/*
 * nori_hip.h -- C ABI of the MI355X (gfx950) hot path of the Nori renderer.
 *
 * This is the drop-in boundary: the host keeps Nori's
 * NoriObject/XML object graph, flattens it into the POD `nori_scene_desc`
 * below, and drives everything that Nori does per sample -- Accel build and
 * rayIntersect, Mesh::rayIntersect, Integrator::Li, BSDF::sample/eval/pdf,
 * Warp::*, Independent/pcg32, PerspectiveCamera::sampleRay, ImageBlock::put --
 * through the entry points declared here.  Plain pointers and sizes only; no
 * C++ types, no torch types.  Every function returns 0 on success or a
 * negative `nori_status`; nothing throws across the boundary.  A context is
 * bound to one GPU and is not thread safe (one host thread per context).  A
 * context owns every device buffer it uses -- scene, tree, the wavefront
 * engine's path-state pool and streams, the film's sample store -- so any
 * number of contexts may live in one process (one per GPU, or several on one
 * GPU) without sharing or freeing each other's memory; nori_hip_destroy frees
 * exactly its context's.
 *
 * Each entry point cites the reference interface it replaces
 * (paths relative to the wjakob/nori tree).
 *
 * The same POD structs are consumed by the CPU oracle (oracle/oracle.h), which
 * is test infrastructure only and is never linked into this library.
 */
#ifndef NORI_HIP_H
#define NORI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The structs below that the LIBRARY writes (nori_render_stats, nori_accel_info) grow with the library: they carry no size
 * field, the library fills sizeof(its own struct).  Header and library must therefore be of ONE version: a caller compares
 * nori_hip_abi_version() -- what the loaded library was built from -- with the NORI_HIP_ABI_VERSION it was compiled against
 * before its first call that passes such a struct, and refuses to go on if they differ (the host library and the Python
 * bindings of this repository do).  Bumped whenever a struct of this header changes size or layout, an enum value changes
 * meaning, or an entry point changes its signature. */
#define NORI_HIP_ABI_VERSION 8      /* textures: nori_texture_desc, nori_scene_desc.{n_textures, textures}, nori_mesh_desc.albedo_texture, nori_hip_texture_eval */
int nori_hip_abi_version(void);

/* ------------------------------------------------------------------ enums */

typedef enum nori_status {
    NORI_OK = 0,
    NORI_ERR_INVALID_ARGUMENT = -1,
    NORI_ERR_NO_DEVICE = -2,       /* no HIP device / HIP runtime error      */
    NORI_ERR_OUT_OF_MEMORY = -3,
    NORI_ERR_NOT_READY = -4,       /* e.g. render before build_accel         */
    NORI_ERR_UNSUPPORTED = -5,
    NORI_ERR_INTERNAL = -6
} nori_status;

/* BSDF plugin names: src/diffuse.cpp:90, src/mirror.cpp:50,
 * src/dielectric.cpp:49, src/microfacet.cpp:90 (NORI_REGISTER_CLASS) */
typedef enum nori_bsdf_type {
    NORI_BSDF_DIFFUSE = 0,
    NORI_BSDF_MIRROR = 1,
    NORI_BSDF_DIELECTRIC = 2,
    NORI_BSDF_MICROFACET = 3
} nori_bsdf_type;

/* Integrator plugin names used by scenes/pa1..pa5 (no implementation ships
 * in the reference; behaviour spec: DESIGN.md §Integrators) */
typedef enum nori_integrator_type {
    NORI_INTEGRATOR_NORMALS = 0,
    NORI_INTEGRATOR_AO = 1,
    NORI_INTEGRATOR_SIMPLE = 2,
    NORI_INTEGRATOR_WHITTED = 3,
    NORI_INTEGRATOR_PATH_MATS = 4,
    NORI_INTEGRATOR_PATH_EMS = 5,
    NORI_INTEGRATOR_PATH_MIS = 6
} nori_integrator_type;

/* src/rfilter.cpp:110-113 */
typedef enum nori_rfilter_type {
    NORI_RFILTER_GAUSSIAN = 0,
    NORI_RFILTER_MITCHELL = 1,
    NORI_RFILTER_TENT = 2,
    NORI_RFILTER_BOX = 3
} nori_rfilter_type;

/* include/nori/common.h:179-183 (EMeasure) */
typedef enum nori_measure {
    NORI_MEASURE_UNKNOWN = 0,
    NORI_MEASURE_SOLID_ANGLE = 1,
    NORI_MEASURE_DISCRETE = 2
} nori_measure;

/* include/nori/warp.h:18-57; numbering follows src/warptest.cpp:79-82 */
typedef enum nori_warp_type {
    NORI_WARP_SQUARE = 0,
    NORI_WARP_TENT = 1,
    NORI_WARP_DISK = 2,
    NORI_WARP_UNIFORM_SPHERE = 3,
    NORI_WARP_UNIFORM_HEMISPHERE = 4,
    NORI_WARP_COSINE_HEMISPHERE = 5,
    NORI_WARP_BECKMANN = 6
} nori_warp_type;

/* How the pcg32 stream of a camera sample is seeded.
 *  PER_SAMPLE : seed(initstate = y*width + x, initseq = sample index) before
 *               every camera sample -- order independent, what a GPU can
 *               reproduce; the mode in which device and oracle images are
 *               compared sample for sample.
 *  NORI_BLOCK : the reference's scheme, src/independent.cpp:36-41 -- one
 *               stream per 32x32 block seeded with (offset.x, offset.y) and
 *               consumed serially over y, x, sample.  On the device this runs
 *               one lane per block (whole frames from sample 0 only; slow by
 *               design): every camera sample then carries exactly the
 *               radiance of a render with the reference's own sampler. */
typedef enum nori_seed_mode {
    NORI_SEED_PER_SAMPLE = 0,
    NORI_SEED_NORI_BLOCK = 1
} nori_seed_mode;

typedef enum nori_accel_builder {
    NORI_ACCEL_HOST_SAH = 0,   /* binned SAH on the host, uploaded            */
    NORI_ACCEL_GPU_LBVH = 1,   /* built on the device: Morton order + radix tree (1.5 ms per million triangles)   */
    NORI_ACCEL_AUTO = 2,       /* GPU_PLOC; HOST_SAH if the device's tree comes out deeper than the traversal stack */
    NORI_ACCEL_GPU_PLOC = 3    /* built on the device: triangles whose boxes are several times the scene's typical one and hold other
                                  geometry enter as several parts (spatial splits up front), Morton order, nearest-neighbour
                                  clustering (PLOC, 3 ms per million triangles), treelet restructuring (a wave per treelet, 2 - 3 ms
                                  per million triangles and sweep), parallel re-insertion (1 ms per million candidates).
                                  wf_extend against HOST_SAH's tree: Cornell box +0.8 %, pa5 table +0.7 %, AO scene +-1 %, terrain of
                                  10 M triangles +2.7 %; built in 19 / 28 / 33 / 144 ms against 30 / 56 / 90 / 2 400 */
} nori_accel_builder;

/* Albedo textures (no counterpart in the reference, which has no Texture class; src/accel.cpp:73 computes the texture
 * coordinates "if provided by the mesh" and nothing reads them).  See nori_texture_desc. */
typedef enum nori_texture_type {
    NORI_TEXTURE_IMAGE = 0,
    NORI_TEXTURE_CHECKERBOARD = 1
} nori_texture_type;
typedef enum nori_texture_filter { NORI_FILTER_NEAREST = 0, NORI_FILTER_BILINEAR = 1 } nori_texture_filter;
typedef enum nori_texture_wrap { NORI_WRAP_REPEAT = 0, NORI_WRAP_CLAMP = 1 } nori_texture_wrap;

/* ------------------------------------------------------ scene description */

/* BSDF parameters; defaults as in the reference constructors
 * (src/diffuse.cpp:18-20, src/dielectric.cpp:17-23, src/microfacet.cpp:17-36).
 * `albedo` holds Diffuse::m_albedo or Microfacet::m_kd. */
typedef struct nori_bsdf_desc {
    int32_t type;       /* nori_bsdf_type */
    float albedo[3];
    float alpha;
    float int_ior;
    float ext_ior;
    float ks;           /* 1 - max(kd), src/microfacet.cpp:35 */
} nori_bsdf_desc;

/* One <mesh>: the buffers of include/nori/mesh.h:160-163 (m_V, m_N, m_UV, m_F;
 * column-major 3xN == xyz interleaved per vertex), already in world space
 * (src/obj.cpp:52,62 applies toWorld at load), plus its BSDF and optional
 * area emitter (mesh.h:128-134). */
typedef struct nori_mesh_desc {
    uint32_t n_vertices;
    uint32_t n_triangles;
    const float *positions;    /* 3 * n_vertices                           */
    const float *normals;      /* 3 * n_vertices or NULL                   */
    const float *texcoords;    /* 2 * n_vertices or NULL                   */
    const uint32_t *indices;   /* 3 * n_triangles                          */
    nori_bsdf_desc bsdf;
    int32_t is_emitter;        /* <emitter type="area">                    */
    float radiance[3];
    uint32_t albedo_texture;   /* 1-based index into nori_scene_desc::textures that replaces bsdf.albedo; 0 = none.
                                  Diffuse BSDFs only */
} nori_mesh_desc;

/* A texture that gives a diffuse BSDF its albedo at the hit's uv (nori_intersection::uv: the mesh's interpolated texture
 * coordinates, or the barycentric (u, v) where it has none -- src/accel.cpp:38,73-77).  The lookup, in float32 without FMA
 * contraction, in this order:
 *   s = u * uscale + uoffset, t = v * vscale + voffset; a non-finite s or t becomes 0.
 *   CHECKERBOARD: ps = floor(s) - 2 floor(s / 2), pt likewise: color0 if ps == pt, else color1.
 *   IMAGE:  wrap  -- REPEAT: s -= floor(s) (may round to 1); CLAMP: s = clamp(s, 0, 1); t the same; then t = 1 - t (v = 1 is
 *                    the top row, row 0 of `texels`)
 *           NEAREST  -- texel (min((int) (s W), W - 1), min((int) (t H), H - 1))
 *           BILINEAR -- x = s W - 0.5, x0 = floor(x), fx = x - x0; columns (int) x0 and (int) x0 + 1, reduced modulo W into
 *                       [0, W) for REPEAT, clamped to [0, W - 1] for CLAMP; rows from y = t H - 0.5 the same way; blended
 *                       with lerp(a, b, f) = a + f (b - a) along x in both rows, then along y (a constant image returns its
 *                       texel's value exactly).
 * No mip-mapping: one lookup per shaded hit. */
typedef struct nori_texture_desc {
    int32_t type;              /* nori_texture_type */
    uint32_t width, height;    /* IMAGE: 1 .. 16384 each; ignored for CHECKERBOARD */
    const float *texels;       /* IMAGE: 3 * width * height floats, linear RGB, row-major, row 0 = the top row of the image */
    int32_t filter;            /* nori_texture_filter */
    int32_t wrap;              /* nori_texture_wrap */
    float uscale, vscale;      /* 1 for an unscaled texture */
    float uoffset, voffset;
    float color0[3], color1[3];/* CHECKERBOARD */
} nori_texture_desc;

/* src/perspective.cpp:22-39; to_world is row-major 4x4 (camera -> world). */
typedef struct nori_camera_desc {
    int32_t width, height;
    float fov;                 /* horizontal, degrees */
    float near_clip, far_clip;
    float to_world[16];
} nori_camera_desc;

/* src/rfilter.cpp constructors. radius is ignored for tent (1) and box (.5) */
typedef struct nori_rfilter_desc {
    int32_t type;              /* nori_rfilter_type */
    float radius;
    float stddev;              /* gaussian */
    float B, C;                /* mitchell */
} nori_rfilter_desc;

typedef struct nori_integrator_desc {
    int32_t type;              /* nori_integrator_type */
    float position[3];         /* simple: point light position             */
    float energy[3];           /* simple: point light power                */
} nori_integrator_desc;

typedef struct nori_scene_desc {
    uint32_t n_meshes;
    const nori_mesh_desc *meshes;
    nori_camera_desc camera;
    nori_rfilter_desc rfilter;
    nori_integrator_desc integrator;
    int32_t sample_count;      /* Independent::m_sampleCount               */
    uint32_t n_textures;       /* referenced by nori_mesh_desc::albedo_texture */
    const nori_texture_desc *textures;
} nori_scene_desc;

/* ------------------------------------------------------- per-query records */

/* include/nori/ray.h:30-34 without dRcp (recomputed on the device). 32 B. */
typedef struct nori_ray {
    float o[3];
    float d[3];
    float mint, maxt;
} nori_ray;

/* include/nori/mesh.h:23-35.  mesh = index into nori_scene_desc::meshes,
 * 0xFFFFFFFF when nothing was hit (Intersection::mesh == nullptr).
 * `tri` is the triangle index inside that mesh (the `f` of accel.cpp:25). */
typedef struct nori_intersection {
    float p[3];
    float t;
    float uv[2];
    float sh_s[3], sh_t[3], sh_n[3];
    float geo_s[3], geo_t[3], geo_n[3];
    uint32_t mesh;
    uint32_t tri;
} nori_intersection;

#define NORI_NO_HIT 0xFFFFFFFFu

/* What to render: the frame is cut into fixed tiles (NORI_TILE_SIZE^2 px,
 * the device analogue of NORI_BLOCK_SIZE, include/nori/block.h:17).  A call
 * renders the tiles whose raster index i satisfies i % tile_mod == tile_rem,
 * with camera samples [spp_begin, spp_begin+spp_count) per pixel, and ADDS the
 * weighted samples into the caller's RGBW accumulation buffer, laid out like
 * the full-frame ImageBlock of src/main.cpp:67: (height+2b) rows x
 * (width+2b) columns x 4 floats, b = nori_hip_border_size().  Summing the
 * buffers of several calls / ranks is exactly ImageBlock::put(ImageBlock&)
 * (src/block.cpp:93-102). */
typedef struct nori_render_params {
    uint32_t spp_begin;
    uint32_t spp_count;
    uint32_t tile_mod;      /* >= 1 */
    uint32_t tile_rem;      /* <  tile_mod */
    int32_t seed_mode;      /* nori_seed_mode */
    int32_t count_traversal;/* != 0: also count node/triangle tests (slower) */
    int32_t time_kernels;   /* != 0: HIP events around every kernel launch, summed per
                               kernel class into nori_render_stats.*_ms          */
    void *stream;           /* hipStream_t or NULL for the default stream   */
} nori_render_params;

#define NORI_TILE_SIZE 16

/* Work counters of one render call.  Ray queries are counted where the
 * reference would pass through Scene::rayIntersect (include/nori/scene.h:63
 * closest hit, :82 shadow). */
typedef struct nori_render_stats {
    uint64_t n_camera_samples;
    uint64_t n_closest_rays;
    uint64_t n_shadow_rays;
    uint64_t n_node_tests;   /* only when count_traversal != 0 */
    uint64_t n_tri_tests;    /* only when count_traversal != 0 */
    uint64_t n_invalid;      /* samples dropped by the isValid() guard,
                                src/block.cpp:63-67 */
    float kernel_ms;         /* HIP-event time of the render kernel on the
                                stream it was launched on */
    uint32_t n_workgroups;   /* launch geometry of the render kernel: one
                                workgroup per (tile, spp chunk)              */
    uint32_t lds_bytes;      /* dynamic LDS per workgroup                    */
    /* time_kernels != 0: summed HIP-event durations, on the launch stream, of
       the ray-query kernels (wf_extend; render_kernel for the megakernel, which
       also shades), the Li kernels (wf_shade, wf_finish) and the film kernels */
    float trace_ms, shade_ms, film_ms;
    uint32_t n_trace_launches;
    uint32_t engine;         /* what rendered this call: 0 = megakernel (render_kernel), 1 = wavefront (wf_extend / wf_shade),
                                2 = the block-serial kernel of NORI_SEED_NORI_BLOCK, 3 = the first-hit feature pass
                                (nori_hip_render_features: feature_pass_kernel).  The option "engine" is a request: "auto"
                                picks by job size, and trees with wide nodes are walked by the wavefront engine only */
    uint32_t trace_cus;      /* CUs the ray-query kernels ran on: all of the device's */
    float tail_ms;           /* time_kernels != 0: summed durations of the wf_finish launches that ran BESIDE the next batch's kernels, on
                                their own `tail_cus` CUs (wavefront engine, calls of two or more batches); not part of shade_ms */
    uint32_t tail_cus;
    uint32_t wf_record;      /* NORI_WF_RECORD_*: the per-path record the wavefront engine kept this call's paths in -- the compact one
                                (88 B: no pcg32 state, no eta, L + Ld summed by the storing pass) for all-diffuse scenes under
                                path_mats / path_ems / path_mis, the full one (100 B) otherwise and for every scene with
                                NORI_HIP_WF_RECORD=full; 0: another engine.  (Appended in the struct's tail padding: its size and the
                                offsets of the fields before it are those of before.) */
} nori_render_stats;
#define NORI_WF_RECORD_NONE 0
#define NORI_WF_RECORD_FULL 1
#define NORI_WF_RECORD_COMPACT 2

typedef struct nori_accel_info {
    uint32_t n_triangles;
    uint32_t n_nodes;
    uint32_t n_leaves;
    uint32_t max_depth;
    uint32_t node_bytes;     /* size of one node record as laid out */
    uint32_t tri_bytes;      /* size of one leaf triangle record     */
    uint64_t total_bytes;    /* nodes + leaf triangles in HBM        */
    float build_ms;
    float sah_cost;
    uint32_t node_children;  /* boxes one node record holds: 2 (BVH2) or 4 (wide nodes, quantised boxes) */
    uint32_t node_records_32b;  /* 1: the tree also exists as 32-B node records (two children's boxes as 16-bit planes on one
                                grid + the links), which the wavefront engine's hand-written node loop walks when the tree's
                                traversal stack fits LDS (depth <= 16); BVH2 trees without unbounded boxes only */
    uint32_t built_on_device;   /* 1: the tree was built by HIP kernels (lbvh.hip), 0: by the host's SAH builder and uploaded */
    uint32_t n_references;      /* device builder: (triangle, box) references the tree holds -- the triangles, plus the parts of those that
                                   were split; 0: built on the host */
} nori_accel_info;

typedef struct nori_hip_ctx nori_hip_ctx;

/* ------------------------------------------------------------ life cycle */

/* Bind a context to HIP device `device`. */
int nori_hip_create(int device, nori_hip_ctx **out);
void nori_hip_destroy(nori_hip_ctx *ctx);
/* Message of the last failing call on this context (or on creation when
 * ctx == NULL).  Stands in for NoriException::what(), common.h:135-140. */
const char *nori_hip_last_error(const nori_hip_ctx *ctx);

/* Copy the scene into HBM (SoA vertex/index buffers, material and emitter
 * tables, textures, camera, filter table).  NORI_ERR_INVALID_ARGUMENT (with a message) for a texture index out of range, a
 * texture on a mesh whose BSDF is not diffuse, an image of zero or more than 16384 texels in a dimension, or an image
 * without texels.  Replaces the load-time half of
 * Scene::addChild / Accel::addMesh (src/scene.cpp:48-52, src/accel.cpp:12-17),
 * the ImageBlock filter tabulation (src/block.cpp:18-27) and
 * PerspectiveCamera::activate (src/perspective.cpp:41-74). */
int nori_hip_upload_scene(nori_hip_ctx *ctx, const nori_scene_desc *scene);

/* Evaluate texture `texture` (1-based, as nori_mesh_desc::albedo_texture) of the uploaded scene at n points uv (2n floats,
 * HOST memory) on the device, with the lookup the shading uses; rgb: 3n floats. */
int nori_hip_texture_eval(nori_hip_ctx *ctx, uint32_t texture, const float *uv, size_t n, float *rgb);

/* Accel::build (src/accel.cpp:19-21 -- a no-op in the reference, a BVH here) */
int nori_hip_build_accel(nori_hip_ctx *ctx, int builder /* nori_accel_builder */);
int nori_hip_accel_info(const nori_hip_ctx *ctx, nori_accel_info *out);

/* Diagnostics of the arithmetic the device substitutes for the reference's `/`, `1 / x` and std::sqrt (Eigen's
 * operator/ and normalized() in src/common.cpp:248-257, include/nori/frame.h, the BSDFs): out[0..2] = operands that left
 * the domain on which the short reciprocal / quotient / square-root sequences are verified bit-identical to the IEEE
 * operations, out[3] = results that came out NaN or infinite (rt_types.h), since the last reset.  Only the
 * build with -DNORI_COUNT_EXCURSIONS (libnori_hip_count.so) counts; the product build returns NORI_ERR_UNSUPPORTED. */
int nori_hip_debug_excursions(nori_hip_ctx *ctx, unsigned long long out[4], int reset);

/* Tuning / engine selection (no reference counterpart).  Keys:
 *   "engine"          "auto" (default: wavefront for >= 2^19 camera samples per call -- 2^24 for the `normals`
 *                     integrator --, else megakernel) | "megakernel" | "wavefront"
 *   "wavefront_paths" paths in flight in the wavefront engine: records of its state pool (default 2^29, 216 B of HBM each;
 *                     bounded by 85 % of the free memory)
 *   "wavefront_samples" camera samples per batch: what the film's sample store holds at a time, 20 B each (twice when a call
 *                     has several batches).  "0" (default): as many as wavefront_paths -- a batch starts all its samples in its
 *                     first pass, the fastest schedule.  A batch bigger than the pool starts its samples pass by pass in the
 *                     slots finished paths leave (regeneration): same frame, bit for bit, at +2 .. 4 % for half to a quarter of the
 *                     pool (more below that); it is what lets an out-of-memory retry shrink the pool and keep the frame, and
 *                     film_order = reference run on any pool
 *   "accel_layout"    node layout of the NEXT nori_hip_build_accel: "bvh2" (64-B node = two full-precision child
 *                     boxes; the wavefront engine walks a second, 32-B form of them, see nori_accel_info) | "bvh4q"
 *                     (64-B node = four child boxes quantised to 8 bits: half the node fetches, for trees that do
 *                     not fit the caches) | "auto" (default: bvh4q from 2^20 triangles)
 *   "film_order"      "fast" (default: the film adds a pixel's samples round by round in LDS tiles) | "reference" (the
 *                     samples are added in the order of renderBlock / ImageBlock::put / BlockGenerator,
 *                     src/main.cpp:33-53, src/block.cpp:62-152: whole frames -- or whole rows of 32x32 blocks through
 *                     nori_hip_render_block_rows --, slower; the frame is then bit-identical to a single-threaded
 *                     render of the same samples by the reference's loops)
 * Unknown keys return NORI_ERR_INVALID_ARGUMENT. */
int nori_hip_set_option(nori_hip_ctx *ctx, const char *key, const char *value);
/* The current value of an option as set_option would take it ("engine", "wavefront_paths", "wavefront_samples", "film_order", "accel_layout"),
 * NUL-terminated into value[capacity]; NORI_ERR_INVALID_ARGUMENT for unknown keys or a buffer too small. */
int nori_hip_get_option(const nori_hip_ctx *ctx, const char *key, char *value, size_t capacity);

/* ImageBlock::m_borderSize for the uploaded filter (src/block.cpp:20). */
int nori_hip_border_size(const nori_hip_ctx *ctx);

/* --------------------------------------------------- operator-level twins */

/* Accel::rayIntersect(ray, its, shadowRay) (src/accel.cpp:23-99) for a batch
 * of n rays held in HOST memory.  shadow_ray != 0: only `mesh` is meaningful
 * (0 = some occluder, NORI_NO_HIT = none), as the reference returns early. */
int nori_hip_intersect(nori_hip_ctx *ctx, const nori_ray *rays,
                       nori_intersection *its, size_t n, int shadow_ray);

/* Same on DEVICE buffers (rays: n x nori_ray, its: n x nori_intersection),
 * asynchronous on `stream`. */
int nori_hip_intersect_device(nori_hip_ctx *ctx, const void *d_rays,
                              void *d_its, size_t n, int shadow_ray,
                              void *stream);

/* PerspectiveCamera::sampleRay (src/perspective.cpp:76-97) for n film
 * positions (pixel_samples: 2n floats, fractional pixel coordinates). */
int nori_hip_sample_rays(nori_hip_ctx *ctx, const float *pixel_samples,
                         size_t n, nori_ray *rays);

/* ------------------------------------------- Thin-lens camera: depth of field
 *
 * No counterpart in the reference, whose PerspectiveCamera draws the aperture sample and discards it (src/perspective.cpp:78).
 * A lens is a state of the context's camera, set after the upload: radius R >= 0 and focus distance F, both in camera space
 * (F is a depth along the optical axis, not a distance along a ray).  R == 0 is the pinhole and NOT the arithmetic below with a
 * zero in it: every kernel branches on R > 0, uniformly over a launch, and takes the code it ran before there was a lens -- a
 * pinhole scene renders the bits it always rendered.
 *
 * For R > 0, a camera sample with film position pixelSample and apertureSample a = (a.x, a.y) -- the second pair of floats every
 * camera sample draws (renderBlock, src/main.cpp:41-46); no random number is added, the streams keep their alignment -- gives,
 * in float32 without FMA contraction, with the operations of the pinhole (division, reciprocal and square root correctly rounded;
 * the sine and cosine of squareToUniformDisk are the pinned ones of nori_hip_warp):
 *   nearP  = sampleToCamera * (pixelSample.x / width, pixelSample.y / height, 0);  d = normalized(nearP)     as nori_hip_sample_rays
 *   invZ   = 1 / d.z
 *   pf     = d * (F * invZ)                          the point of the pinhole ray on the plane z = F (one product, then three)
 *   (lx, ly) = squareToUniformDisk(a)                (NORI_WARP_UNIFORM_DISK);  l = (R * lx, R * ly, 0)
 *   dl     = normalized(pf - l)
 *   ray.o  = cameraToWorld * l     (a point: the affine product and the division by w, as the pinhole's origin)
 *   ray.d  = cameraToWorld * dl    (a vector)
 *   invZl  = 1 / dl.z;   ray.mint = nearClip * invZl;   ray.maxt = farClip * invZl
 * All rays of one film position meet at pf, so what lies at depth F is sharp; a point at depth z is spread over a circle of
 * diameter 2 R |z - F| / z on the plane z = F.
 *
 * Who uses it: nori_hip_render on both engines (the megakernel's camera sample; the wavefront engine's first vertex, in its first
 * extend and its first shade), nori_hip_render_features (feature frames are blurred like the beauty frame they guide) and
 * nori_hip_sample_rays_lens.  Everything built on those kernels inherits the lens with no code of its own:
 * nori_hip_render_moments, nori_hip_render_tiles, nori_hip_render_to_error, nori_hip_render_adaptive (and _denoised),
 * nori_hip_render_allocated, film_order = reference and its block rows, the device group.  The exception is
 * NORI_SEED_NORI_BLOCK, which exists for parity with the reference's sampler: a render in that mode with R > 0 returns
 * NORI_ERR_UNSUPPORTED with a message and leaves the context as it was.
 *
 * nori_hip_set_lens        the lens of the uploaded scene, from the next launch on.  NORI_ERR_NOT_READY without a scene;
 *                          NORI_ERR_INVALID_ARGUMENT for a radius that is negative or not finite, and, when radius > 0, for a
 *                          focus distance that is not finite or not positive (with radius == 0 the focus distance is kept as
 *                          given and has no effect).  nori_hip_upload_scene resets to the pinhole (0, 0).
 * nori_hip_get_lens        what was set (either pointer may be NULL).
 * nori_hip_sample_rays_lens  the operator-level twin: the ray of the statement above for n pairs (pixel_samples, aperture_samples:
 *                          2n floats each), with the context's lens.  With radius == 0 the bits of nori_hip_sample_rays, which
 *                          stays the pinhole's twin whatever the lens. */
int nori_hip_set_lens(nori_hip_ctx *ctx, float radius, float focus_distance);
int nori_hip_get_lens(const nori_hip_ctx *ctx, float *radius, float *focus_distance);
int nori_hip_sample_rays_lens(nori_hip_ctx *ctx, const float *pixel_samples, const float *aperture_samples,
                              size_t n, nori_ray *rays);

/* Integrator::Li (include/nori/integrator.h:42) for n rays; path k draws its
 * random numbers from pcg32.seed(seed_state[k], seed_seq[k]).  rgb: 3n. */
int nori_hip_li(nori_hip_ctx *ctx, const nori_ray *rays, size_t n,
                const uint64_t *seed_state, const uint64_t *seed_seq,
                float *rgb);

/* BSDF::sample / eval / pdf (include/nori/bsdf.h:59,70,87) in the local
 * frame.  wi, wo: 3n floats; sample: 2n; weight, value: 3n; eta, pdf: n. */
int nori_hip_bsdf_sample(nori_hip_ctx *ctx, const nori_bsdf_desc *bsdf,
                         const float *wi, const float *sample, size_t n,
                         float *wo, float *weight, float *eta,
                         int32_t *measure);
int nori_hip_bsdf_eval(nori_hip_ctx *ctx, const nori_bsdf_desc *bsdf,
                       const float *wi, const float *wo, size_t n,
                       float *value);
int nori_hip_bsdf_pdf(nori_hip_ctx *ctx, const nori_bsdf_desc *bsdf,
                      const float *wi, const float *wo, size_t n, float *pdf);

/* Warp::squareToX / squareToXPdf (include/nori/warp.h:18-57).  sample: 2n.
 * out: 3n (2D warps leave z = 0).  pdf takes points in the same 3n layout. */
int nori_hip_warp(nori_hip_ctx *ctx, int warp /* nori_warp_type */,
                  float param, const float *sample, size_t n, float *out);
int nori_hip_warp_pdf(nori_hip_ctx *ctx, int warp, float param,
                      const float *points, size_t n, float *pdf);

/* The device's own arithmetic, element by element: out[k] = op(a[k], b[k]) through the functions the kernels call
 * (rt_types.h: exact_rcp, exact_div, the shared-reciprocal quotient of f3 / float, exact_sqrt; rt_trace.h: slab_rcp;
 * rt_math.h: det_sincosf, det_logf, det_expf), compiled with the product's flags.  They have no CPU twin that says
 * anything about them (the CPU builds use the plain operators), so this is where tests/test_gpu_arith.py holds them
 * against IEEE arithmetic.  b is read by the two quotients only and may be NULL otherwise.  In libnori_hip_count.so the
 * calls count into nori_hip_debug_excursions like any other.  No scene is needed. */
typedef enum nori_arith_op {
    NORI_ARITH_RCP = 0,           /* exact_rcp(a) */
    NORI_ARITH_DIV = 1,           /* exact_div(a, b) */
    NORI_ARITH_DIV_SHARED = 2,    /* x of (f3) {a, a, a} / b: one exact_rcp_raw(b), exact_div_by per component */
    NORI_ARITH_SQRT = 3,          /* exact_sqrt(a) */
    NORI_ARITH_SLAB_RCP = 4,      /* slab_rcp(a) */
    NORI_ARITH_SIN = 5,           /* det_sincosf(a): the sine */
    NORI_ARITH_COS = 6,           /*                 the cosine */
    NORI_ARITH_LOG = 7,           /* det_logf(a) */
    NORI_ARITH_EXP = 8            /* det_expf(a) */
} nori_arith_op;
int nori_hip_debug_arith(nori_hip_ctx *ctx, int op /* nori_arith_op */,
                         const float *a, const float *b, size_t n, float *out);

/* The emitter pick itself: for n samples (xiE, xiT, xi1, xi2) -- samples[4 k ..] -- the mesh index of the emitter that
 * emitter_pick (rt_path.h) selects, the triangle within that mesh and the point p[3 k ..] that emitter_point places on it:
 * the functions sample_direct calls, 256 threads per workgroup, one sample per thread.  `reader` names how the kernel reads
 * the scene's small tables (mesh records, emitter list, triangle CDFs), one for each way the render kernels do
 * (shade_tables.h).  NORI_TABLES_LDS returns NORI_ERR_UNSUPPORTED for a scene whose tables do not fit the LDS copy (more
 * than 32 meshes or 960 CDF entries): wf_shade reads those from global memory.  An unknown reader or a scene without
 * emitters is NORI_ERR_INVALID_ARGUMENT.  Samples are expected in [0, 1], ends included.  Needs a scene, no tree. */
typedef enum nori_tables_reader {
    NORI_TABLES_GLOBAL = 0,       /* SceneTables through DevScene's pointers: li_kernel, wf_shade of a scene that does not fit */
    NORI_TABLES_REDIRECTED = 1,   /* shade_tables_to_lds, then SceneTables on the redirected pointers: render_kernel, wf_finish
                                     (global memory when the tables do not fit) */
    NORI_TABLES_LDS = 2           /* shade_tables_copy + LdsTables: wf_shade of a scene that fits */
} nori_tables_reader;
int nori_hip_debug_emitter_sample(nori_hip_ctx *ctx, int reader /* nori_tables_reader */, const float *samples, size_t n,
                                  uint32_t *mesh, uint32_t *tri, float *p);

/* The tables those samples are drawn from, read back from device memory: counts = {n_meshes, n_emitters, n_cdf}; then,
 * where the pointer is not NULL, the emitter list (n_emitters mesh indices), per mesh its cdf_offset, n_triangles and
 * inv_area (n_meshes each; cdf_offset and inv_area mean something for emitters only) and the CDF entries (n_cdf floats: per
 * emitter n_triangles + 1, from 0 to 1).  Call it with NULL arrays first to size them. */
int nori_hip_debug_emitter_tables(nori_hip_ctx *ctx, uint32_t counts[3], uint32_t *emitters, uint32_t *cdf_offset,
                                  uint32_t *n_triangles, float *inv_area, float *cdf);

/* The tree as the kernels see it, read back from device memory after a device synchronise -- whichever builder made it
 * (NORI_ACCEL_HOST_SAH: the uploaded copy).  *root = the root's child-link code; counts = {n_nodes, n_pairs, wide, records_32b}:
 * node records in device memory (0: the root is a leaf), pair records (a wide tree's reserved pair 0 included), 1 if the nodes
 * are WIDE nodes, 1 if the tree also exists as 32-B records.  Then, where the pointer is not NULL: nodes (16 floats per node
 * record, rt_types.h), nodes32 (8 dwords per 32-B record, rt_nodeq.h) with grid = (mn[3], scale[3]) -- both left untouched
 * without such records --, pairs (24 floats per pair record).  Call it with NULL arrays first to size them.
 * Needs a built tree: NORI_ERR_INVALID_ARGUMENT before nori_hip_build_accel succeeded; the context stays usable. */
int nori_hip_debug_tree(nori_hip_ctx *ctx, int32_t *root, uint32_t counts[4], float *nodes, uint32_t *nodes32, float grid[6], float *pairs);

/* The per-tile candidate lists of the wavefront engine's first pass (first_lists.h), built on the device and read back: one launch
 * of wf_first_build -- the kernel a render launches, unchanged -- over the 16 x 16 tile grid a render of the context's camera uses
 * (tiles_x = ceil(width / 16), tiles_y = ceil(height / 16), tile = ty tiles_x + tx), with the cap K, into buffers of this call's
 * own, which are copied out and freed.  The lists the engine keeps for its renders are neither read nor touched, and the
 * NORI_HIP_WF_FIRST* switches are not read: the call answers for any K whatever a render of this process would do.
 * count[tile] (tiles_x tiles_y words) is the kernel's own encoding: the number of pair records in the tile's list, or 0xffffffff
 * for an overflow tile (more than K pairs, or no pyramid); pairs[tile max(K, 1) + k], k < count[tile], are the indices of those pair
 * records in the tree's pair array (nori_hip_debug_tree), in the order the walk found them; the other slots are 0.
 * K > 64 (the most a list may hold) and a context without a built tree are NORI_ERR_INVALID_ARGUMENT with a message; the context
 * stays usable.  A lens, a wide tree and a root that is a leaf are not refused: first_camera gives such a scene ok = 0, so every
 * tile comes back as overflow -- as K = 0 does.  Synchronous, on the default stream, after a device synchronise. */
int nori_hip_debug_first_lists(nori_hip_ctx *ctx, uint32_t K, uint32_t *count, uint32_t *pairs);

/* wf_extend -- the traversal kernel of the wavefront engine -- on n rays of the caller's choosing, all arrays in HOST memory.
 * Slot k is a stored path vertex as wf_shade would have left it: origin origins[3 k ..] (both rays start there, with the mint every
 * stored ray has, 1e-4), a continuation ray dir_a[3 k ..] (slot A: closest hit, maxt = inf) and / or a shadow ray dir_b[4 k ..] =
 * (d.xyz, maxt) (slot B: any hit), as flags[k] says: 0 (empty slot: nothing is traced), 1 (A), 2 | 4 (B, the path ends on it) or
 * 1 | 2 (B, then A, by the same lane).  The directions of a slot the flags do not name are not read.  The records go into the
 * context's path-state pool and ONE launch over stored paths is made, with the kernel variant, stack, persistent grid, thresholds
 * and NORI_HIP_WF_* knobs a render of this scene would use.
 * hits[4 k ..] = (t, u, v, hit word) as the kernel wrote them: the closest hit of A -- (inf, 0, 0) without one, or without A --, the
 * word's low 31 bits the GLOBAL triangle index (a mesh's triangles follow those of the meshes before it) or 0x7fffffff, bit 31 =
 * B was occluded.  An empty slot keeps the four words NORI_EXTEND_SENTINEL the array is filled with before the launch.
 * counts = {closest-hit queries, shadow queries, node tests, triangle tests}; the last two are counted with count_traversal != 0,
 * by the kernels a render with nori_render_params::count_traversal runs.
 * NORI_ERR_INVALID_ARGUMENT, before anything is launched: n larger than the option "wavefront_paths" (or than the 2^29 records a
 * pool can index), a flag word other than those four, a non-finite origin, direction component or maxt (maxt = +inf is a valid
 * value) or a direction of all zeros in a slot the flags name.  n == 0 launches nothing.  Needs an acceleration structure. */
#define NORI_EXTEND_SENTINEL 0xcdcdcdcdu
int nori_hip_debug_extend(nori_hip_ctx *ctx, const float *origins, const float *dir_a, const float *dir_b, const uint32_t *flags, size_t n,
                          int count_traversal, float *hits, unsigned long long counts[4]);

/* pcg32::nextFloat stream (Independent::next1D, src/independent.cpp:46-48):
 * out[k*count + j] = j-th float of pcg32.seed(seed_state[k], seed_seq[k]). */
int nori_hip_pcg32_floats(nori_hip_ctx *ctx, const uint64_t *seed_state,
                          const uint64_t *seed_seq, size_t n, uint32_t count,
                          float *out);
/* The same streams `skip` draws further (pcg32::advance): out[k*count + j] = float number
 * skip + j of pcg32.seed(seed_state[k], seed_seq[k]).  This is how the host's Independent sampler
 * continues ONE stream seeded by prepare(block) = seed(offset.x, offset.y)
 * (src/independent.cpp:36-41) across refills of its buffer. */
int nori_hip_pcg32_floats_at(nori_hip_ctx *ctx, const uint64_t *seed_state,
                             const uint64_t *seed_seq, uint64_t skip, size_t n,
                             uint32_t count, float *out);

/* ImageBlock::put(pos, value) (src/block.cpp:62-91) of n samples into the
 * full-frame RGBW buffer `rgbw` (HOST memory, layout as in
 * nori_render_params; accumulated into). positions: 2n, values: 3n. */
int nori_hip_splat(nori_hip_ctx *ctx, const float *positions,
                   const float *values, size_t n, float *rgbw);

/* ----------------------------------------------------------- the hot path */

/* renderBlock + render (src/main.cpp:27-119) for the tiles / samples named in
 * `params`, accumulating into the DEVICE buffer d_rgbw (see
 * nori_render_params).  Asynchronous on params->stream unless `stats` is
 * non-NULL, in which case the call synchronises the stream and fills it. */
int nori_hip_render(nori_hip_ctx *ctx, const nori_render_params *params,
                    void *d_rgbw, nori_render_stats *stats);

/* ------------------------------------------- second moments, error map, render to a target error
 *
 * No counterpart in the reference, which has no measure of a frame's noise.
 *
 * nori_hip_render_moments is nori_hip_render, and the same samples' SECOND MOMENTS ADDED into d_m2, a DEVICE buffer with the
 * layout of d_rgbw.  For every sample the film accepts and every pixel it reaches with tap weight w = wx wy (as the fast
 * film forms it), the RGBW pixel receives (L w, w) and the moment pixel (float32(L_c L_c) w, float32(w w)): the square is
 * rounded to float32 first, then fma(square, w, sum) like the beauty channels (a radiance above 1.8e19, whose square is
 * not finite, enters as FLT_MAX).  Samples the isValid() guard rejects (src/block.cpp:63-67) reach neither frame.  The RGBW frame has
 * the bits nori_hip_render gives with the same parameters and options; stats count the samples once.  All engines and
 * seed modes; film_order must be "fast" (NORI_ERR_UNSUPPORTED otherwise -- nori_hip_render_block_rows keeps no moments
 * either).  Moment frames of disjoint shares (tiles, sample ranges) add like RGBW frames.
 * nori_hip_render_moments_host: both frames to zeroed HOST buffers, as nori_hip_render_host. */
int nori_hip_render_moments(nori_hip_ctx *ctx, const nori_render_params *params,
                            void *d_rgbw, void *d_m2, nori_render_stats *stats);
int nori_hip_render_moments_host(nori_hip_ctx *ctx, const nori_render_params *params,
                                 float *rgbw, float *m2, nori_render_stats *stats);

/* The error map: per pixel of the frame WITHOUT the border, the relative standard error of the pixel's mean under the
 * plug-in weighted variance.  With S the RGBW pixel and M the moment pixel, in float32 without FMA contraction, IEEE
 * division and square root, in this order:
 *   if !(S.w > 0): err = 0 and the pixel counts as empty; else
 *   r = 1 / S.w;  k = (M.w * r) * r                               (1 / k = (sum w)^2 / sum w^2, the effective sample count)
 *   num = 0; den = 0
 *   for c in r, g, b:  mu = S.c * r;  q = M.c * r;  v = q - mu * mu;  if !(v > 0) v = 0
 *                      num = num + sqrt(v * k);  den = den + |mu|
 *   err = num / (den + 0.03f)
 * Limits: below two samples per pixel the map means nothing (one sample has v = 0); the plug-in variance is biased low by
 * the factor 1 - k; under filters with negative lobes (Mitchell) weights are not probabilities, the formula is applied
 * as it stands, v clamped at 0 and pixels of W <= 0 counted as empty.
 * d_err: height * width floats on the DEVICE, row-major, or NULL.  out: the summary, or NULL (one of the two must be
 * given).  The summary is reduced on the device without floating-point atomics, in a fixed order -- sum_err in binary64,
 * max_err and the counts exact -- so two calls on the same frames return the same bytes.  With out != NULL the call
 * synchronises `stream`; otherwise it is asynchronous on it, uses nothing of the context's and may run on several
 * streams at once.  (Like every call, a summary call must not overlap another call on the same context from a second
 * thread.)  n_above counts frame pixels only, whatever the sign of `threshold`. */
typedef struct nori_error_summary {
    double   sum_err;      /* sum of err over the frame's pixels */
    float    max_err;
    float    threshold;    /* as passed in */
    uint64_t n_pixels, n_empty, n_above;   /* n_above: err > threshold */
} nori_error_summary;
int nori_hip_error_map(nori_hip_ctx *ctx, const void *d_rgbw, const void *d_m2,
                       void *d_err /* height*width floats, may be NULL */,
                       float threshold, nori_error_summary *out, void *stream);
/* Convenience: the same for frames and a map in HOST memory (copied to scratch device buffers and back; synchronous). */
int nori_hip_error_map_host(nori_hip_ctx *ctx, const float *rgbw, const float *m2, float *err /* may be NULL */,
                            float threshold, nori_error_summary *out);

/* Render until the frame is good enough: samples [spp_begin, spp_begin + spp_count) -- spp_count is the most the call may
 * spend -- in passes of pass_spp (the last may be shorter) through nori_hip_render_moments, ADDING into d_rgbw and d_m2.
 * From the second pass on the error map is evaluated after each pass (threshold = target_mean_err); the call stops when
 * sum_err / n_pixels <= target_mean_err or the samples are spent.  Sampling is uniform over the frame.  *spp_done = samples
 * per pixel rendered; *last = the summary of the frames as they are left (evaluated once at the end if no pass did);
 * stats: counters and times summed over the passes, the rest as of the last pass.  Any of the three may be NULL.
 * params->tile_mod must be 1, pass_spp >= 1, target_mean_err >= 0 (NORI_ERR_INVALID_ARGUMENT).  Synchronous. */
int nori_hip_render_to_error(nori_hip_ctx *ctx, const nori_render_params *params /* spp_count = the most it may spend */,
                             uint32_t pass_spp, float target_mean_err,
                             void *d_rgbw, void *d_m2, uint32_t *spp_done,
                             nori_error_summary *last, nori_render_stats *stats);

/* Convenience, as nori_hip_render_host: the same loop into scratch device frames; the RGBW frame, and where the pointers are not
 * NULL the moment frame and the error map (height * width floats) of the frames as they are left, to HOST buffers (overwritten). */
int nori_hip_render_to_error_host(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t pass_spp, float target_mean_err,
                                  float *rgbw, float *m2, float *err, uint32_t *spp_done,
                                  nori_error_summary *last, nori_render_stats *stats);

/* ------------------------------------------- tile lists, tile errors, selection, adaptive sampling
 *
 * No counterpart in the reference, whose BlockGenerator hands out every block once.
 *
 * nori_hip_render_tiles renders samples [spp_begin, spp_begin + spp_count) of exactly the listed NORI_TILE_SIZE^2 tiles and ADDS
 * them into d_rgbw -- and, where d_m2 is not NULL, their second moments into d_m2 -- exactly as nori_hip_render /
 * nori_hip_render_moments do for a progression: a list that equals {tile_rem + k tile_mod} gives the frames, moment frames and
 * counters of that call, bit for bit.  tiles: n_tiles raster ids ty * tiles_x + tx in HOST memory, strictly ascending (so no
 * tile twice); NORI_ERR_INVALID_ARGUMENT, with a message, for an id outside the frame or a list that is not strictly
 * ascending.  params->tile_mod must be 1 and tile_rem 0.  n_tiles == 0 succeeds and touches nothing.  Both engines ("auto"
 * picks by the list's camera samples); film_order must be "fast" and seed_mode NORI_SEED_PER_SAMPLE (NORI_ERR_UNSUPPORTED
 * otherwise: reference order and the block-serial sampler render whole frames).  The list is copied to device memory of the
 * context's: the call synchronises params->stream once before it renders.  Frames of disjoint lists add like the frames
 * of disjoint shares.
 * nori_hip_render_tiles_host: into zeroed HOST frames (m2 may be NULL), as nori_hip_render_host. */
int nori_hip_render_tiles(nori_hip_ctx *ctx, const nori_render_params *params,
                          const uint32_t *tiles /* HOST */, uint32_t n_tiles,
                          void *d_rgbw, void *d_m2 /* may be NULL */, nori_render_stats *stats);
int nori_hip_render_tiles_host(nori_hip_ctx *ctx, const nori_render_params *params, const uint32_t *tiles, uint32_t n_tiles,
                               float *rgbw, float *m2 /* may be NULL */, nori_render_stats *stats);

/* The tile errors: per tile t = ty * tiles_x + tx of the frame (tiles_x = ceil(width / 16), tiles_y likewise), the mean of the
 * error map over the tile's pixels inside the frame.  One workgroup of 256 threads per tile:
 *   thread ly * 16 + lx:  e = err of frame pixel (16 tx + lx, 16 ty + ly) by the formula of nori_hip_error_map (the same device
 *                         function), 0 for a pixel outside the frame (and for an empty one, as there)
 *   the 256 values, converted to binary64, are added in a fixed tree: for off = 128, 64, ..., 1: lane t < off takes lane t + off
 *   tile_err = (float) (sum / n),  n = the tile's pixels inside the frame (binary64 division, then rounded to float32)
 * No atomics: the same frames give the same bytes.  d_tile_err: tiles_x * tiles_y floats on the DEVICE.  Asynchronous on
 * `stream`; reads the context's frame geometry and writes nothing of the context's, so it may run on several streams at once.  nori_hip_tile_errors_host: frames and the array in HOST memory; synchronous. */
int nori_hip_tile_errors(nori_hip_ctx *ctx, const void *d_rgbw, const void *d_m2,
                         void *d_tile_err /* tiles_x*tiles_y floats */, void *stream);
int nori_hip_tile_errors_host(nori_hip_ctx *ctx, const float *rgbw, const float *m2, float *tile_err);

/* Selection: tiles_out = the tiles t of tiles_in (HOST, strictly ascending, checked as for nori_hip_render_tiles) with
 * !(d_tile_err[t] <= target), in the order of tiles_in -- a tile whose error is NaN stays in --, *n_out their number
 * (tiles_out holds up to n_in entries).  d_tile_err: DEVICE, as nori_hip_tile_errors fills it.  On the device this is a stable
 * compaction by prefix sum, not an atomic append: the order is part of the result, and two calls return the same bytes.  The
 * adaptive loop below runs the same kernels on its list in device memory; this twin exists so that they can be driven without a
 * render.  Synchronous; replaces the context's current tile list. */
int nori_hip_select_tiles(nori_hip_ctx *ctx, const void *d_tile_err, float target,
                          const uint32_t *tiles_in, uint32_t n_in,
                          uint32_t *tiles_out, uint32_t *n_out);

/* Adaptive sampling: nori_hip_render_to_error with the samples steered by the tile errors.  The active set starts as all
 * tiles.  Pass k = 0, 1, ... renders samples [spp_begin + k pass_spp, spp_begin + (k + 1) pass_spp) -- the last pass may be
 * shorter: params->spp_count is the most a pixel may get -- of the ACTIVE tiles through the tile-list render with moments,
 * ADDING into d_rgbw and d_m2, and adds that count to tile_spp of the active tiles.  From the second pass on, the tile errors of
 * the whole frame are then evaluated and the active set is replaced by its members with !(tile_err <= target_tile_err).  A
 * retired tile never returns -- the set only shrinks, even where taps of a neighbour raise a retired tile's error again --, so all
 * active tiles share one sample range and the result can be replayed from outside: pass k is nori_hip_render_tiles of
 * {t : tile_spp[t] > k pass_spp}.  The loop stops when the set is empty or the samples are spent.
 * d_tile_spp: tiles_x * tiles_y uint32 on the DEVICE, overwritten, or NULL.  out (may be NULL): the passes rendered, the tiles of
 * the frame, the tiles still active when the call stopped (after the last evaluation; if the samples were spent in one pass,
 * the tiles above the target in a measurement made for the summary alone), the least and most samples a tile received, and the
 * error-map summary of the frames as they are left (threshold = target_tile_err).  stats (may be NULL): counters and times
 * summed over the passes, the rest as of the last pass.  Arguments are checked as for nori_hip_render_to_error (tile_mod 1,
 * pass_spp >= 1, target_tile_err >= 0) and nori_hip_render_tiles (fast film, NORI_SEED_PER_SAMPLE).  Synchronous.
 * Limits.  The stopping rule looks at the samples it stops on, so a tile that stops early does so on an estimate of its
 * variance that is biased low -- as in every such scheme; the mean stays a mean of independent samples per pixel, but the
 * number of them depends on their values.  A retired tile's edge pixels still receive taps from active neighbours: pixels are
 * normalised by their weight, so this is consistent.  Granularity is a tile: one noisy pixel keeps 256 sampling.
 * nori_hip_render_adaptive_host: the same loop into scratch device frames; the RGBW frame, and where the pointers are not NULL
 * the moment frame, the error map (height * width floats) and tile_spp of the frames as they are left, to HOST buffers. */
typedef struct nori_adaptive_summary {
    uint32_t passes, n_tiles, n_unconverged;   /* tiles still above the target when the call stopped */
    uint32_t spp_min, spp_max;                 /* over the tiles */
    nori_error_summary frame;                  /* of the frames as they are left, threshold = target */
} nori_adaptive_summary;
int nori_hip_render_adaptive(nori_hip_ctx *ctx, const nori_render_params *params /* spp_count = the most a pixel may get */,
                             uint32_t pass_spp, float target_tile_err, void *d_rgbw, void *d_m2,
                             void *d_tile_spp /* tiles_x*tiles_y uint32, may be NULL; overwritten */,
                             nori_adaptive_summary *out, nori_render_stats *stats);
int nori_hip_render_adaptive_host(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t pass_spp, float target_tile_err,
                                  float *rgbw, float *m2, float *err, uint32_t *tile_spp,
                                  nori_adaptive_summary *out, nori_render_stats *stats);

/* ------------------------------------------- first-hit feature frames: albedo, shading normal, depth
 *
 * No counterpart in the reference.  What a denoiser is guided by: per camera sample the albedo, the shading normal and the
 * distance of the FIRST surface the sample's camera ray meets, filtered into frames laid out like the beauty frame.  A pass of
 * its own (features.h): one closest-hit ray per camera sample, no path; the kernels of nori_hip_render are not involved and
 * render the same bits before and after a call.
 *
 * The camera sample (px, py, s) is the one nori_hip_render draws (NORI_SEED_PER_SAMPLE), in float32 without FMA contraction:
 *   pcg32.seed(py * width + px, s);  j = (nextFloat, nextFloat);  pixelSample = (px + j.x, py + j.y)
 *   a second pair of floats is drawn for the aperture (src/perspective.cpp:78): unused by the pinhole, the lens's apertureSample
 *   ray = PerspectiveCamera::sampleRay(pixelSample)                      (src/perspective.cpp:76-97; nori_hip_sample_rays;
 *                                                                         with a lens set: nori_hip_sample_rays_lens, "Thin-lens camera")
 *   its = the closest hit of ray in [mint, maxt]                         (Accel::rayIntersect; nori_hip_intersect)
 * and the sample's three values are
 *   albedo  miss: (0, 0, 0).  Hit on mesh m: NORI_BSDF_MIRROR and NORI_BSDF_DIELECTRIC give (1, 1, 1); NORI_BSDF_DIFFUSE and
 *           NORI_BSDF_MICROFACET give bsdf.albedo (the microfacet's kd), a textured mesh (albedo_texture != 0) the texture
 *           lookup stated under nori_texture_desc at its.uv instead -- the value the shading multiplies with.  An emitter is a
 *           mesh like any other: the albedo of its BSDF, not its radiance.
 *   normal  ENCODED: e_c = 0.5f * n_c + 0.5f per component (one multiply, exact; one add, rounded) of the shading normal
 *           n = its.shFrame.n (nori_intersection::sh_n).  Miss: (0.5, 0.5, 0.5).  Encoded because the film's isValid() guard
 *           (src/block.cpp:63-67) gives weight 0 to a sample with a negative component: a signed normal would be dropped.
 *   depth   hit: (t, float32(t * t), 1) with t = nori_intersection::t; miss: (0, 0, 0).  The third channel is coverage, the
 *           second lets a consumer form the variance of the distance.
 * No other special cases: a value the guard rejects (not finite, negative) is dropped like any radiance and counted in n_invalid.
 *
 * Each requested feature's samples are ADDED into that feature's frame, a DEVICE buffer with the RGBW layout and size of
 * nori_hip_render's, by the fast film (film_order is not consulted: a feature frame has no reference order): (value w, w) per
 * tap of weight w, so the W channel of every feature frame has the bits of the W channel nori_hip_render's megakernel engine
 * gives with the same parameters (while no sample is rejected).  spp_begin, spp_count, tile_mod, tile_rem, stream and
 * time_kernels mean what they mean to nori_hip_render; frames of disjoint shares add like RGBW frames.  count_traversal is
 * ignored (n_node_tests = n_tri_tests = 0).  Asynchronous on params->stream unless `stats` is non-NULL.
 * features: a mask of nori_feature; the frame of a feature that is not requested is not touched and may be NULL.
 * Decode, per pixel, each quotient 0 where its divisor is <= 0:
 *   albedo = rgb / W
 *   normal = 2 * rgb / W - 1            (a filtered mean of unit vectors: NOT renormalised; normalise if unit length is wanted)
 *   depth:  coverage c = B / W;  mean distance over the hits = R / B;  mean squared distance over the hits = G / B
 * Errors: NORI_ERR_INVALID_ARGUMENT for features == 0, unknown bits or a requested frame that is NULL; NORI_ERR_UNSUPPORTED
 * (with a message) for NORI_SEED_NORI_BLOCK and for a filter border above 8; NORI_ERR_NOT_READY without an acceleration
 * structure.  Stats: n_camera_samples; n_closest_rays (one per camera sample inside the frame); n_shadow_rays = 0; n_invalid
 * summed over the gathers that ran (one per requested feature); kernel_ms, trace_ms (the pass), film_ms as for the
 * megakernel; engine = 3.  Limits: whole frames or tile_mod shares on one context -- no tile lists, no device groups.
 * nori_hip_render_features_host: the requested frames to zeroed HOST buffers, as nori_hip_render_host. */
typedef enum nori_feature { NORI_FEATURE_ALBEDO = 1, NORI_FEATURE_NORMAL = 2, NORI_FEATURE_DEPTH = 4 } nori_feature;
int nori_hip_render_features(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t features,
                             void *d_albedo, void *d_normal, void *d_depth, nori_render_stats *stats /* may be NULL */);
int nori_hip_render_features_host(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t features,
                                  float *albedo, float *normal, float *depth, nori_render_stats *stats /* may be NULL */);

/* ------------------------------------------- the denoiser: feature- and variance-guided NL-means
 *
 * No counterpart in the reference.  The consumer of the moment frame (nori_hip_render_moments) and of the feature frames
 * (nori_hip_render_features): the NL-means of Rousselle et al. with variance cancellation, its patch distance formed from the
 * per-pixel variance of the mean, with one cross-bilateral term per feature under a single exponential.  A translation unit
 * of its own (denoise.h); the kernels of the renders are not involved and render the same bits before and after a call.
 *
 * All frames have the bordered RGBW layout of nori_hip_render; only the height x width pixels inside the border are read.
 * Everything below is float32 without FMA contraction, every `/` an IEEE division, in the order written.
 *
 * Step A, the guide record of a frame pixel: 16 floats  mu[3], var[3], albedo[3], normal[3], z, cov, valid, 0.
 * With S the RGBW pixel and M the moment pixel (the terms of nori_hip_error_map):
 *   if !(S.w > 0): valid = 0, mu = var = 0; else valid = 1 and
 *   r = 1 / S.w;  k = (M.w * r) * r
 *   for c in r, g, b:  mu_c = S.c * r;  q = M.c * r;  v = q - mu_c * mu_c;  if !(v > 0) v = 0;  var_c = v * k
 * (var is the plug-in variance of the pixel's mean.)  With A, N, D the pixels of the albedo, normal and depth frames -- the
 * decode stated under nori_hip_render_features, a quotient a / b being 0 unless b > 0:
 *   albedo_c = A.c / A.w;   normal_c = 2 * (N.c / N.w) - 1 (0 unless N.w > 0);   cov = D.b / D.w;   z = D.r / D.b
 * whether or not the pixel is valid.  A feature frame passed as NULL leaves its fields 0 and switches its term off in step B.
 *
 * Step B, the filter (nori_denoise_params; min(a, b) below is a < b ? a : b).  Per pixel p:
 *   if valid_p == 0: out = (0, 0, 0), wsum = 0.  Otherwise num = (0, 0, 0), wsum = 0 and, dy = -R .. R the outer and dx = -R .. R
 *   the inner loop, q = p + (dx, dy); a tap with q outside the frame or valid_q == 0 contributes nothing; else
 *   1  the colour distance of a pair (p', q'):  delta = 0;  for c in r, g, b:
 *        t = mu_p'c - mu_q'c;  nume = t * t - alpha * (var_p'c + min(var_q'c, var_p'c))
 *        deno = 1e-10f + (k_c * k_c) * (var_p'c + var_q'c);  delta = delta + nume / deno
 *   2  the patch:  acc = 0, cnt = 0;  oy = -F .. F the outer and ox = -F .. F the inner loop, p' = p + o, q' = q + o: if both
 *      are inside the frame and valid, acc = acc + delta(p', q') and cnt += 1 (o = 0 always qualifies).
 *      d = acc / (3.0f * (float) cnt);  if !(d > 0) d = 0
 *   3  the exponent:  e = d;  each sum s below starts at 0 and runs s = s + t * t over the three components in order
 *        with albedo:  t = albedo_pc - albedo_qc;  e = e + s / tau_albedo
 *        with normal:  t = normal_pc - normal_qc;  e = e + s / tau_normal
 *        with depth:   t = z_p - z_q;  g = (k_depth * k_depth) * (z_p * z_p + z_q * z_q) + 1e-12f;  e = e + (t * t) / g
 *                      u = cov_p - cov_q;  e = e + (u * u) / tau_cov
 *   4  the weight:  w = exp(-e) if e <= 87.0f, else 0 -- exp as NORI_ARITH_EXP (nori_hip_debug_arith) evaluates it, the pinned
 *      function of the render path; the cut-off keeps subnormal weights and a NaN exponent out
 *   5  num_c = num_c + w * mu_qc;  wsum = wsum + w
 *   and after the loop out_c = num_c / wsum (the centre tap has e = 0, w = 1: wsum >= 1).
 *
 * nori_hip_denoise_guides runs step A and writes height * width * 16 floats to d_guides; nori_hip_denoise runs both steps
 * (its guide records live in a buffer of the context, one per stream) and writes d_rgb_out, height * width * 3 floats in the
 * layout of nori_hip_develop, and -- unless NULL -- d_wsum, height * width floats.  params == NULL: the defaults.  d_albedo,
 * d_normal, d_depth may each be NULL; d_rgbw and d_m2 may not.  All DEVICE memory.  Asynchronous on `stream`, nothing of the
 * context's but the frame geometry is read, no atomics: the same frames give the same bytes, and calls on different streams
 * may run at once.  Errors: NORI_ERR_NOT_READY without an uploaded scene; NORI_ERR_INVALID_ARGUMENT (with a message) for a
 * NULL required pointer, radius outside 1 .. 8, patch outside 0 .. 2, k_c, tau_albedo, tau_normal, tau_cov or k_depth not above
 * 0, alpha below 0.  The _host twins take HOST frames and buffers and are synchronous, as nori_hip_error_map_host.
 * Limits: below about 16 samples per pixel the variance estimates are too noisy to guide the weights; a firefly has a large
 * variance of its own and passes unchanged. */
typedef struct nori_denoise_params {
    uint32_t radius;         /* R: the window is (2R + 1)^2 taps, 1 .. 8 */
    uint32_t patch;          /* F: patches are (2F + 1)^2 pixels, 0 .. 2 */
    float k_c;               /* the colour distance's sensitivity */
    float alpha;             /* strength of the variance cancellation */
    float tau_albedo, tau_normal;
    float k_depth;           /* relative depth tolerance */
    float tau_cov;
} nori_denoise_params;
#define NORI_DENOISE_PARAMS_DEFAULT { 5u, 1u, 1.0f, 1.0f, 0.02f, 0.1f, 0.1f, 0.05f }
int nori_hip_denoise_guides(nori_hip_ctx *ctx, const void *d_rgbw, const void *d_m2, const void *d_albedo /* may be NULL */,
                            const void *d_normal /* may be NULL */, const void *d_depth /* may be NULL */, void *d_guides, void *stream);
int nori_hip_denoise(nori_hip_ctx *ctx, const nori_denoise_params *params /* NULL: the defaults */, const void *d_rgbw, const void *d_m2,
                     const void *d_albedo, const void *d_normal, const void *d_depth, void *d_rgb_out, void *d_wsum /* may be NULL */,
                     void *stream);
int nori_hip_denoise_guides_host(nori_hip_ctx *ctx, const float *rgbw, const float *m2, const float *albedo, const float *normal,
                                 const float *depth, float *guides);
int nori_hip_denoise_host(nori_hip_ctx *ctx, const nori_denoise_params *params, const float *rgbw, const float *m2, const float *albedo,
                          const float *normal, const float *depth, float *rgb_out, float *wsum /* may be NULL */);

/* ------------------------------------------- the denoiser with the variance of its output; adaptive sampling that stops on it
 *
 * No counterpart in the reference.  The last link of moments -> error map -> tile lists -> feature frames -> denoiser: an estimate
 * of how good the DENOISED frame is, so that the adaptive loop can retire tiles on the error of what the user will look at.  A
 * translation unit of its own (denoise_error.h); the kernels of nori_hip_denoise, of the renders, the film and the tile lists are
 * not involved and give the same bits before and after a call.
 *
 * nori_hip_denoise_var is nori_hip_denoise with three more accumulators in step B.  Per pixel p, vnum = (0, 0, 0) beside num and
 * wsum, and in step 5 of every contributing tap, after wsum = wsum + w:
 *   ww = w * w;  for c in r, g, b, in that order:  vnum_c = vnum_c + ww * var_qc          (var_q: step A's var of the tap's pixel)
 * and after the loop  var_out_c = (vnum_c / wsum) / wsum.  A pixel with valid_p == 0 gives var_out = (0, 0, 0).  float32 without
 * contraction, IEEE division, in the order written, as the rest of step B.  d_rgb_out and d_wsum have the bits nori_hip_denoise
 * gives on the same frames; d_var_out is height * width * 3 floats in d_rgb_out's layout.  var_out is the variance of the output
 * under FIXED weights and independent pixel means: sum_q w_q^2 var_q / (sum_q w_q)^2.
 * tiles: n_tiles raster ids of NORI_TILE_SIZE^2 tiles in HOST memory, strictly ascending -- checked and refused as for
 * nori_hip_render_tiles --, or NULL: the whole frame.  With a list only the pixels of the listed tiles are written (one workgroup
 * per listed tile; guide records are made for the whole frame, because windows reach into neighbouring tiles), and they have the
 * bits of the whole-frame call.  The list is copied to device memory of the context's: the call synchronises `stream` once for
 * the upload and replaces the context's current tile list, as nori_hip_select_tiles does.  tiles != NULL with n_tiles == 0
 * succeeds and touches nothing.  Otherwise as nori_hip_denoise: asynchronous on `stream`, the same errors, and
 * NORI_ERR_INVALID_ARGUMENT for d_var_out == NULL.
 *
 * The error of a denoised pixel, with rgb, var, wsum as nori_hip_denoise_var wrote them -- the form of nori_hip_error_map's
 * formula, so a target means the same thing for the raw and the denoised frame:
 *   if !(wsum > 0): err = 0 and the pixel counts as empty; else num = 0, den = 0 and
 *   for c in r, g, b:  num = num + sqrt(var_c);  den = den + |rgb_c|
 *   err = num / (den + 0.03f)
 * nori_hip_denoised_error_map writes err per pixel to d_err (height * width floats, or NULL) and the summary to out (or NULL; one
 * of the two must be given), reduced in the fixed order of nori_hip_error_map's summary, with its synchronisation rules: with out
 * the call synchronises `stream`, without it is asynchronous and uses nothing of the context's.  nori_hip_denoised_tile_errors is
 * nori_hip_tile_errors for this error: one 256-thread workgroup per tile, thread ly * 16 + lx, 0 outside the frame, the binary64
 * tree off = 128 .. 1, tile_err = (float) (sum / n); asynchronous on `stream`.  No atomics anywhere.  The _host twins take HOST
 * buffers and are synchronous.
 *
 * nori_hip_render_adaptive_denoised is nori_hip_render_adaptive with the tiles retired on the denoised tile errors.  The active set
 * starts as all tiles; d_rgb_out, d_var_out and d_wsum are zeroed.  Pass k renders its sample range of the active tiles with
 * moments, ADDING into d_rgbw and d_m2, and adds to tile_spp, exactly as nori_hip_render_adaptive.  From the second pass on each
 * pass is followed by step A over the whole frame, the variance filter over the ACTIVE tiles only (the list as the selection left
 * it in device memory), nori_hip_denoised_tile_errors of the outputs, and the selection: the active set is replaced by its members
 * with !(tile_err <= target_tile_err).  A retired tile never returns.  The loop stops when the set is empty or the samples are
 * spent; then step A and the filter run once over the WHOLE frame (the neighbours of a retired tile have changed since it was last
 * filtered), so the outputs are nori_hip_denoise_var of the frames as they are left.  The retiring can be replayed from outside:
 * the active tiles' filtered pixels are those of a whole-frame nori_hip_denoise_var of the frames after that pass.
 * d_albedo, d_normal, d_depth: feature frames the caller rendered (nori_hip_render_features), each may be NULL.  denoise_params
 * NULL: the defaults.  d_tile_spp may be NULL.  out (may be NULL): as nori_adaptive_summary says, frame being the summary of the
 * denoised error map of the outputs (threshold = target); n_unconverged = the tiles active when the loop stopped, or, if only one
 * pass ran, the tiles whose final denoised tile error is not <= target.  Arguments are checked as for nori_hip_render_adaptive and
 * nori_hip_denoise, with the same codes.  Synchronous.  The _host twin renders into zeroed scratch frames, takes the feature frames
 * from HOST memory and writes rgbw, rgb_out and, where not NULL, m2, var_out, wsum, err (the denoised error map) and tile_spp.
 * Limits.  The estimate holds the weights fixed -- they are functions of the same noisy means -- and takes the pixels' means as
 * independent; it carries no bias term, so what the filter blurs away is not counted.  Under pixel filters wider than the box
 * neighbouring pixels share samples and the estimate is low.  Below about 16 samples per pixel the weights themselves are
 * unreliable.  One device only.  Not built: a dual-buffer (cross-filtered) estimate. */
int nori_hip_denoise_var(nori_hip_ctx *ctx, const nori_denoise_params *params /* NULL: the defaults */, const void *d_rgbw, const void *d_m2,
                         const void *d_albedo, const void *d_normal, const void *d_depth,
                         const uint32_t *tiles /* HOST, strictly ascending, or NULL: the whole frame */, uint32_t n_tiles,
                         void *d_rgb_out, void *d_var_out, void *d_wsum /* may be NULL */, void *stream);
int nori_hip_denoise_var_host(nori_hip_ctx *ctx, const nori_denoise_params *params, const float *rgbw, const float *m2, const float *albedo,
                              const float *normal, const float *depth, const uint32_t *tiles, uint32_t n_tiles,
                              float *rgb_out, float *var_out, float *wsum /* may be NULL */);
int nori_hip_denoised_error_map(nori_hip_ctx *ctx, const void *d_rgb, const void *d_var, const void *d_wsum,
                                void *d_err /* height*width floats, may be NULL */, float threshold, nori_error_summary *out, void *stream);
int nori_hip_denoised_error_map_host(nori_hip_ctx *ctx, const float *rgb, const float *var, const float *wsum, float *err /* may be NULL */,
                                     float threshold, nori_error_summary *out);
int nori_hip_denoised_tile_errors(nori_hip_ctx *ctx, const void *d_rgb, const void *d_var, const void *d_wsum,
                                  void *d_tile_err /* tiles_x*tiles_y floats */, void *stream);
int nori_hip_denoised_tile_errors_host(nori_hip_ctx *ctx, const float *rgb, const float *var, const float *wsum, float *tile_err);
int nori_hip_render_adaptive_denoised(nori_hip_ctx *ctx, const nori_render_params *params /* spp_count = the most a pixel may get */,
                                      uint32_t pass_spp, float target_tile_err, const nori_denoise_params *denoise_params /* NULL: the defaults */,
                                      void *d_rgbw, void *d_m2, const void *d_albedo, const void *d_normal, const void *d_depth /* each may be NULL */,
                                      void *d_rgb_out, void *d_var_out, void *d_wsum,
                                      void *d_tile_spp /* tiles_x*tiles_y uint32, may be NULL; overwritten */,
                                      nori_adaptive_summary *out, nori_render_stats *stats);
int nori_hip_render_adaptive_denoised_host(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t pass_spp, float target_tile_err,
                                           const nori_denoise_params *denoise_params, float *rgbw, float *m2, const float *albedo,
                                           const float *normal, const float *depth, float *rgb_out, float *var_out, float *wsum,
                                           float *err, uint32_t *tile_spp, nori_adaptive_summary *out, nori_render_stats *stats);

/* ------------------------------------------- rendering to a target error in few passes: tile sample levels from a pilot
 *
 * No counterpart in the reference.  The two adaptive loops above make up to budget / pass_spp passes, most of them over few tiles,
 * and every pass pays the render's fixed price.  The error they stop on is a standard error of a mean and falls as 1 / sqrt(N), so
 * after a pilot each tile's need can be predicted and rendered in ONE long call per group of tiles.  A translation unit of its own
 * (film_alloc.h); no kernel of the renders, the film, the tile lists, the feature frames or the denoiser changes.
 *
 * Levels.  spp_j = pilot_spp << j for j = 0 .. J, J = min(7, floor(log2(spp_count / pilot_spp))), spp_count = params->spp_count: spp_J is
 * the most a pixel gets.  Every tile of the frame has a level l and a done flag.  The pilot renders samples [spp_begin, spp_begin +
 * spp_0) of ALL tiles with moments; all tiles start at level 0, not done.
 * A round evaluates the tile errors E_t of the frames as they are (metric 0: nori_hip_tile_errors; metric 1: see below) and then, one
 * thread per tile that is not done, in float32 without contraction and with IEEE division:
 *   if (E <= target) done
 *   else  r = E / target
 *         need = (headroom * (float) spp_l) * (r * r)
 *         j = l;  while (j < J && !((float) spp_j >= need)) ++j
 *         if (j == l) done        (it sits at the top level: unconverged)
 *         else the tile moves l -> j
 * So a NaN error moves the tile to J (as nori_hip_select_tiles keeps a NaN in), target == 0 sends every tile with an error above zero
 * to J, and a done tile never returns.  The moving tiles are grouped by pair (i, j), i < j: bucket b = i J - i (i - 1) / 2 + (j - i - 1)
 * -- ascending in i, then j; J (J + 1) / 2 <= 28 buckets --, ascending tile id inside a bucket, into one array with
 * bucket_begin[0 .. n_buckets] (a stable compaction by prefix sum: per-256-tile counts per bucket, one scan, a ranked scatter; no
 * atomics, the same inputs give the same bytes).  The moves of a round are rendered bucket by bucket in that order, empty buckets
 * skipped: each is one tile-list render with moments of samples [spp_begin + spp_i, spp_begin + spp_j) of the bucket's tiles, ADDING
 * into d_rgbw and d_m2 -- what nori_hip_render_tiles does with that list.  The loop ends when a round moves nothing or after
 * max_rounds rounds; one more evaluation then fills the summary.  The host reads bucket_begin (29 words) once per round; the lists
 * never leave device memory.  At most 1 + J (J + 1) / 2 render calls per round, each over every tile that shares the move.
 *
 * metric 1 stops on the error of the DENOISED frame: an evaluation is step A over the whole frame, nori_hip_denoise_var's filter over
 * the tiles not yet done (in the first round all tiles, later the tiles the previous round moved -- every other tile is done), whose
 * pixels have the bits of a whole-frame call, then nori_hip_denoised_tile_errors.  d_rgb_out, d_var_out and d_wsum are zeroed at the
 * start; at the end step A and the filter run once over the WHOLE frame, exactly as nori_hip_render_adaptive_denoised finishes, so
 * the outputs are nori_hip_denoise_var of the frames as they are left.  metric 0 ignores the denoiser's arguments (all may be NULL).
 *
 * nori_hip_allocate_tiles drives the classification and the grouping without a render, as nori_hip_select_tiles drives the
 * selection: level and done (HOST, one uint32 per tile of the frame, in and out; level <= J, done zero or not), d_tile_err on the
 * DEVICE; tiles_out (HOST, room for every tile of the frame) receives the grouped array, bucket_begin (HOST, 29 words) the offsets:
 * entries n_buckets .. 28 hold the number of moving tiles.  Only pilot_spp, target_tile_err and headroom steer it; all of alloc is
 * checked.  Synchronous on the default stream.
 *
 * nori_hip_render_allocated.  d_tile_spp (tiles_x * tiles_y uint32, may be NULL): spp_l of every tile's final level.  d_level_log
 * ((max_rounds + 1) * tiles_x * tiles_y uint32, may be NULL): row 0 the levels after the pilot (all 0), row k the levels after round
 * k; rows of rounds that did not run repeat the last levels.  The loop can be replayed from the log: the tiles with
 * log[k-1][t] = i and log[k][t] = j are bucket (i, j) of round k.  out (may be NULL): nori_adaptive_summary with passes = the render
 * calls made (the pilot included), spp_min / spp_max over the tiles, n_unconverged = the tiles with !(E_t <= target) in the final
 * evaluation, frame = the summary of the error map (metric 1: the denoised error map) of what is left, threshold = target.  stats: as
 * for nori_hip_render_adaptive.  Errors, with the existing codes: NORI_ERR_INVALID_ARGUMENT for pilot_spp < 2, max_rounds < 1, a target
 * that is not a number >= 0, headroom that is not a number >= 1, a metric other than 0 and 1, spp_count < pilot_spp, tile_mod != 1,
 * metric 1 without its three output buffers, and denoiser parameters out of range; NORI_ERR_UNSUPPORTED for film_order = reference and
 * NORI_SEED_NORI_BLOCK, as nori_hip_render_tiles.  Synchronous.  The _host twin renders into zeroed scratch frames and writes rgbw and,
 * where not NULL, m2, err (the error map of the metric), tile_spp, level_log, and for metric 1 rgb_out (required), var_out, wsum.
 * Limits.  The pilot's variance estimate is biased low where it stops tiles, and a tile's need is under-predicted from few samples:
 * the later rounds and headroom are the remedy.  Levels are powers of two, so a tile may receive up to twice its need.  Granularity is
 * a tile.  One device only. */
typedef struct nori_allocate_params {
    uint32_t pilot_spp;       /* >= 2 */
    uint32_t max_rounds;      /* >= 1 */
    float    target_tile_err; /* >= 0 */
    float    headroom;        /* >= 1 */
    int32_t  metric;          /* 0 raw, 1 denoised */
} nori_allocate_params;
int nori_hip_allocate_tiles(nori_hip_ctx *ctx, const nori_allocate_params *alloc, uint32_t spp_count /* the budget: sets J */,
                            const void *d_tile_err /* tiles_x*tiles_y floats, DEVICE */,
                            uint32_t *level /* HOST, in and out */, uint32_t *done /* HOST, in and out */,
                            uint32_t *tiles_out /* HOST, tiles_x*tiles_y */, uint32_t *bucket_begin /* HOST, 29 */);
int nori_hip_render_allocated(nori_hip_ctx *ctx, const nori_render_params *params /* spp_count = the most a pixel may get */,
                              const nori_allocate_params *alloc, const nori_denoise_params *denoise_params /* NULL: the defaults */,
                              void *d_rgbw, void *d_m2, const void *d_albedo, const void *d_normal, const void *d_depth /* each may be NULL */,
                              void *d_rgb_out, void *d_var_out, void *d_wsum /* metric 1; metric 0: ignored */,
                              void *d_tile_spp /* may be NULL */, void *d_level_log /* may be NULL */,
                              nori_adaptive_summary *out, nori_render_stats *stats);
int nori_hip_render_allocated_host(nori_hip_ctx *ctx, const nori_render_params *params, const nori_allocate_params *alloc,
                                   const nori_denoise_params *denoise_params, float *rgbw, float *m2, const float *albedo,
                                   const float *normal, const float *depth, float *rgb_out, float *var_out, float *wsum,
                                   float *err, uint32_t *tile_spp, uint32_t *level_log,
                                   nori_adaptive_summary *out, nori_render_stats *stats);

/* film_order = "reference" shared out over devices or ranks.  The reference adds a 32x32 block's samples consecutively
 * into the block's own ImageBlock (renderBlock, src/main.cpp:27-55) and the blocks into the frame in BlockGenerator's order
 * (src/block.cpp:93-152): the smallest share that keeps the order is a block, the one handed out here is a ROW of blocks.
 * nori_hip_render_block_rows renders block rows [row_begin, row_begin + row_count) (clipped to the frame) with samples
 * [spp_begin, spp_begin + spp_count) and writes the bordered accumulators of THOSE blocks into d_block_acc, the array for
 * ALL blocks of the frame: nori_hip_block_acc_floats floats, block b = by * blocks_x + bx at b * (32 + 2 border)^2 * 4,
 * zeroed by the caller.  The arrays of disjoint shares sum exactly in any order (x + 0 = x), e.g. by one ncclReduce;
 * nori_hip_resolve_blocks then ADDS the blocks into the RGBW frame in BlockGenerator's order -- the bits of the frame one
 * device renders with film_order = reference, whatever the number of shares.  params: tile_mod 1, tile_rem 0,
 * NORI_SEED_PER_SAMPLE; the context's film_order must be "reference". */
int nori_hip_block_acc_floats(nori_hip_ctx *ctx, size_t *n_floats);
int nori_hip_render_block_rows(nori_hip_ctx *ctx, const nori_render_params *params, uint32_t row_begin, uint32_t row_count,
                               void *d_block_acc, nori_render_stats *stats);
int nori_hip_resolve_blocks(nori_hip_ctx *ctx, const void *d_block_acc, void *d_rgbw, void *stream);

/* Convenience: zero a host RGBW buffer, render into a scratch device buffer
 * and copy back (synchronous). */
int nori_hip_render_host(nori_hip_ctx *ctx, const nori_render_params *params,
                         float *rgbw, nori_render_stats *stats);

/* ImageBlock::toBitmap (src/block.cpp:45-51): rgb = rgbw.rgb / w (0 if w==0)
 * without the border, on the device.  d_rgb: height*width*3 floats. */
int nori_hip_develop(nori_hip_ctx *ctx, const void *d_rgbw, void *d_rgb,
                     void *stream);

/* ------------------------------------------------------ all GPUs of one node
 *
 * render() of the reference spreads the image blocks over TBB workers (src/main.cpp:85-113) and merges every worker's
 * block into the frame under a mutex, ImageBlock::put(ImageBlock&) (src/block.cpp:93-102).  A group does the same over
 * the GPUs of a node: one context and one host thread per device, every device renders its share of the frame into its
 * own RGBW buffer, ONE merge on the first device (RCCL over xGMI), the merged frame to the caller's host buffer.
 * Shares: NORI_SPLIT_TILE = 16x16 tiles round-robin over the devices, NORI_SPLIT_SAMPLE = a range of the per-pixel
 * sample indices each.  Merges: NORI_MERGE_REDUCE = ncclReduce(sum) of the whole frames, NORI_MERGE_GATHER (tile split,
 * tile columns divisible by the device count) = every device sends only the column strips its tiles touched.
 * A device list that names a device more than once is served without RCCL (peer copies) -- for tests on one GPU; so is a
 * node whose librccl cannot be loaded (nori_hip_group_warning says so).  A fresh RCCL group proves its communicators before
 * nori_hip_group_create returns, on a buffer the size of a 2052^2 frame (67 MB): a sum-reduce of a known pattern, then the
 * gather merge's grouped ncclSend / ncclRecv, both checked on the device.  With film_order = reference on its contexts a
 * group hands out rows of 32x32 blocks instead (whatever `split` says), merges the blocks' accumulators (a reduce of disjoint
 * arrays: exact) and adds them into the frame in BlockGenerator's order on the first device: the frame has the bits of the
 * one-device frame for any number of devices.  NORI_SEED_NORI_BLOCK renders whole frames on one device: a group of more
 * than one refuses it. */
typedef struct nori_hip_group nori_hip_group;
typedef enum nori_group_split { NORI_SPLIT_TILE = 0, NORI_SPLIT_SAMPLE = 1 } nori_group_split;
typedef enum nori_group_merge { NORI_MERGE_REDUCE = 0, NORI_MERGE_GATHER = 1 } nori_group_merge;

/* NORI_ERR_NO_DEVICE when a listed device does not exist ("device 1 not found ...", nori_hip_group_last_error(NULL)) */
int nori_hip_group_create(const int *devices, int n_devices, nori_hip_group **out);
void nori_hip_group_destroy(nori_hip_group *group);
int nori_hip_group_size(const nori_hip_group *group);
/* context of device i of the list (owned by the group): options, accel_info, the batch operators */
nori_hip_ctx *nori_hip_group_ctx(nori_hip_group *group, int i);
const char *nori_hip_group_last_error(const nori_hip_group *group);
/* "rccl" or "copy" */
const char *nori_hip_group_transport(const nori_hip_group *group);
/* "" or why the group merges over peer copies although RCCL was wanted (librccl not loadable on this box) */
const char *nori_hip_group_warning(const nori_hip_group *group);
/* nori_render_stats::engine of every device's share of the last frame ("auto" picks by the size of a share, so the devices
 * may differ); returns the number of entries written (<= capacity) or a negative nori_status */
int nori_hip_group_engines(const nori_hip_group *group, uint32_t *engines, int capacity);
/* nori_hip_upload_scene + nori_hip_build_accel on every device, side by side (Scene::activate per device) */
int nori_hip_group_upload_scene(nori_hip_group *group, const nori_scene_desc *scene, int builder /* nori_accel_builder */);
/* nori_hip_set_lens on every device's context (the upload resets it, as on one context) */
int nori_hip_group_set_lens(nori_hip_group *group, float radius, float focus_distance);
/* The render loop of src/main.cpp:78-119 over the group: samples [spp_begin, spp_begin + spp_count) of every pixel of the
 * width x height frame (params->tile_mod must be 1: the group shares the tiles out itself), merged into the HOST buffer
 * `rgbw` (layout of nori_render_params; overwritten).  stats: counters summed over the devices, times = the slowest
 * device's; merge_ms: HIP-event time of the merge on the first device's stream. */
int nori_hip_group_render_host(nori_hip_group *group, const nori_render_params *params, int split, int merge,
                               int width, int height, float *rgbw, nori_render_stats *stats, float *merge_ms);

/* ------------------------------------------- Environment-map emitter
 *
 * No counterpart in the reference, which lights a scene with area emitters on meshes only (Scene::addChild(EEmitter) throws).
 * An environment is a state of the context, set after the upload like the lens and reset by the next upload; no struct of the
 * scene description grows.  Without one every kernel is the kernel it was: the path integrators have a second set of
 * instantiations (rt_path.h, kEnvLit) that only scenes with an environment run -- "every BSDF, textures, environment", and on
 * the wavefront engine the full path record.  path_mats, path_ems and path_mis use it; normals, ao and simple ignore it as they
 * ignore area emitters; whitted samples emitters and has no variant: NORI_ERR_UNSUPPORTED.  NORI_SEED_NORI_BLOCK renders
 * refuse an environment (NORI_ERR_UNSUPPORTED): the mode exists for parity with the reference's sampler.  The feature pass is
 * unchanged: a camera ray that leaves the scene has coverage 0.
 *
 * The map is OCTAHEDRAL, N x N texels of linear RGB, nearest lookup.  Everything below is float32 without FMA contraction;
 * every / is the correctly rounded quotient, every sqrt the correctly rounded root; dot(a, b) = a.x b.x + (a.y b.y + a.z b.z);
 * sgn(x) = +1 for x >= 0 (either zero), -1 otherwise; M = to_world, row-major.
 *
 *   Direction -> texel.   l = (dot(column 0 of M, d), dot(column 1, d), dot(column 2, d))                  (M^T d)
 *                         s = (|l.x| + |l.y|) + |l.z|;   q = l / s              the point of the octahedron |x|+|y|+|z| = 1
 *                         (px, py) = (q.x, q.y);  if q.z < 0:  (px, py) = ((1 - |q.y|) sgn(q.x), (1 - |q.x|) sgn(q.y))
 *                         u = px 0.5 + 0.5;   v = py 0.5 + 0.5
 *                         i = min((int) (u N), N - 1);   j = min((int) (v N), N - 1)          column i of row j  (and >= 0,
 *                                                                                             which only a direction that is not finite needs)
 *                         Le(d) = texels[3 (j N + i) + c] scale[c]
 *   Tables.               texel centre: u = (i + 0.5) / N, v = (j + 0.5) / N;  px = u 2 - 1, py = v 2 - 1,
 *                         pz = (1 - |px|) - |py|;  if pz < 0 the fold above on (px, py);  c = (px, py, pz)
 *                         lum(r, g, b) = (r 0.212671 + g 0.715160) + b 0.072169              (Color3f::getLuminance)
 *                         weight(i, j) = lum(Le of the texel) / cube(c),   cube(x) = n sqrt(n),  n = dot(x, x)     (|x|^3)
 *                         Row j's CDF over its columns: cdf[0] = 0, cdf[i + 1] = cdf[i] + weight(i, j) in index order; the row's
 *                         sum is cdf[N]; if it is > 0 every entry is divided by it (a row of zeros keeps its zeros).  The CDF
 *                         over the rows is made the same way from the row sums (DiscretePDF::append / normalize, dpdf.h).
 *   Density.              pdf(d) = (((rows[j+1] - rows[j]) (cols_j[i+1] - cols_j[i])) ((N N) 0.25)) cube(q), with q, i, j of d:
 *                         the probability of d's texel, over the texel's area 4 / N^2 in the square, times the Jacobian |q|^3.
 *   Sample(xi).           j = DiscretePDF::sample(rows, xi.y), i = DiscretePDF::sample(cols_j, xi.x) (std::lower_bound: the entry
 *                         before the first cdf >= xi, clamped to [0, N - 1]); the sample is reused inside the texel:
 *                         t = (xi - cdf[k]) / (cdf[k+1] - cdf[k]), or 0.5 where that difference is 0 (an entry of probability
 *                         zero, which only xi = 0 selects);  u = (i + tx) / N, v = (j + ty) / N;  px = u 2 - 1, py = v 2 - 1,
 *                         pz = (1 - |px|) - |py|;  if pz < 0 the fold;  l = normalized(px, py, pz);  d = M l (dot of M's rows).
 *                         The Le and pdf returned are those of "Direction -> texel" and "Density" for this d: the sampled
 *                         path and the BSDF-sampled path agree on the density of a direction, also at texel borders.
 *   In Li (path_mats / path_ems / path_mis).  The number of lights is n_emitters + 1 in the emitter pick (index n_emitters is
 *                         the environment), in pdfPick = 1 / n_lights and in the MIS term of an emitter hit.  An emitter
 *                         sample still draws four numbers (xiE, xiT, xi): the environment takes its direction from xi, leaves
 *                         xiT unused, has pdf_em = pdf(d) pdfPick, Ld = f Le (cosX / pdf_em) and a shadow ray with
 *                         maxt = inf; a sample of density 0 adds nothing.  A ray that leaves the scene adds T Le(d) wMat with
 *                         the wMat an emitter hit has: 1 for path_mats; for path_ems 1 after a discrete bounce (and for the
 *                         camera ray), else 0; for path_mis pdf_mat / (pdf_mat + pdf(d) pdfPick) after a bounce that is not
 *                         discrete.  A scene without area emitters samples the environment alone.
 *
 * nori_hip_set_environment   env == NULL: no environment (the kernels and bits of before).  Else the map is copied, its tables
 *                            are built on the device (three kernels, no atomics: the same map gives the same tables) and it is
 *                            used from the next launch on.  Synchronous.  NORI_ERR_NOT_READY before an upload;
 *                            NORI_ERR_UNSUPPORTED for the whitted integrator; NORI_ERR_INVALID_ARGUMENT, with a message, for
 *                            size 0 or above 4096, NULL texels, a texel or scale that is negative or not finite, a map whose
 *                            scaled luminance is 0 everywhere, a to_world whose rows are not orthonormal within 1e-4.  A failed
 *                            call leaves the context's environment as it was.
 * nori_hip_get_environment   the size N of the environment set, 0: none.
 * nori_hip_env_eval          Le (rgb: 3n) and, unless pdf is NULL, the density (n) of n world directions (dirs: 3n, unit length).
 * nori_hip_env_sample        Sample for n pairs xi (2n): directions (3n), Le (3n), densities (n).
 * nori_hip_debug_env_tables  the tables as the device holds them: row_cdf N + 1, col_cdf N (N + 1) row after row,
 *                            texel_weight N N; any pointer may be NULL.
 * The last three return NORI_ERR_NOT_READY, with a message, while no environment is set. */
typedef struct nori_env_desc {
    uint32_t size;         /* N: the map is N x N texels, 1 .. 4096 */
    const float *texels;   /* 3*N*N floats, linear RGB, row-major, octahedral layout (above); finite, >= 0 */
    float scale[3];        /* multiplies every texel */
    float to_world[9];     /* row-major rotation: world = M * local */
} nori_env_desc;
int nori_hip_set_environment(nori_hip_ctx *ctx, const nori_env_desc *env);
int nori_hip_get_environment(const nori_hip_ctx *ctx, uint32_t *size);
int nori_hip_env_eval(nori_hip_ctx *ctx, const float *dirs, size_t n, float *rgb, float *pdf);
int nori_hip_env_sample(nori_hip_ctx *ctx, const float *xi, size_t n, float *dirs, float *rgb, float *pdf);
int nori_hip_debug_env_tables(nori_hip_ctx *ctx, float *row_cdf, float *col_cdf, float *texel_weight);
/* nori_hip_set_environment on every device's context (the upload resets it, as on one context) */
int nori_hip_group_set_environment(nori_hip_group *group, const nori_env_desc *env);

/* ------------------------------------------- Homogeneous participating medium
 *
 * No counterpart in the reference, whose class enum names EMedium and EPhaseFunction (include/nori/object.h:25,27) and ships neither.
 * There is ONE medium per context and it fills all space; the camera is inside it.  It is a state of the context, set after the
 * upload like the lens and the environment and reset by the next upload; no struct of the scene description grows.  Without one
 * every kernel is the kernel it was: the path integrators have a third set of instantiations (rt_path.h, kMedium) that only
 * contexts with a medium run -- "every BSDF, textures, medium", and on the wavefront engine the full path record.  path_mats,
 * path_ems and path_mis render it; every other integrator refuses it (NORI_ERR_UNSUPPORTED), and so do a context with an
 * environment map (a medium that fills all space has zero transmittance to infinity; nori_hip_set_environment refuses likewise
 * while a medium is set) and NORI_SEED_NORI_BLOCK renders.  The feature pass is unchanged: it reports the first SURFACE a camera
 * ray meets, whatever lies between.
 *
 * Parameters: a scalar (grey) extinction sigma_t, a single-scattering albedo[3], the Henyey-Greenstein asymmetry g (g > 0 scatters
 * forward, along the ray's direction of travel).  A grey sigma_t makes the weights of distance sampling cancel exactly: a
 * scattering vertex multiplies the throughput by albedo and by nothing else, reaching a surface multiplies it by 1.
 *
 * Everything below is float32 without FMA contraction; every / is the correctly rounded quotient, every sqrt the correctly rounded
 * root; log, exp, sin and cos are the pinned ones; dot(a, b) = a.x b.x + (a.y b.y + a.z b.z).
 *
 *   Derived once.         g2 = g g;  A = 1 - g2;  B = 1 + g2;  G2 = 2 g;  C = 1 - g.  A g with |g| < 1e-3 is stored as exactly 0.
 *   Density.              HG(c) = (kInvFourPi A) / (k sqrt(k)),  k = B - G2 c;  with g = 0 this is kInvFourPi exactly.
 *   Transmittance.        Tr(dist) = exp(-(sigma_t dist)).
 *   Distance.             s(xi) = (-log(1 - xi)) / sigma_t + 0   (the addition changes one value: xi = 0 gives +0, not -0).
 *   Phase sample(d, xi).  g = 0: local = squareToUniformSphere(xi).  Otherwise sq = A / (C + G2 xi.x);  c = (B - sq sq) / G2, clamped
 *                         to [-1, 1];  r = sqrt(max(0, 1 - c c));  (sn, cs) = sincos((2 kPi) xi.y);  local = (r cs, r sn, c).
 *                         wo = Frame(d).toWorld(local), not renormalised;  pdf = HG(dot(d, wo)), RE-EVALUATED from the final
 *                         direction: sampling and emitter sampling agree on the density of a direction.
 *   In Li (path_mats / path_ems / path_mis).  When the answer of a closest-hit query for the ray (o, d) is consumed, before
 *                         anything else: one number xi_d is drawn (camera rays and continuation rays alike, so it follows the
 *                         camera sample's four draws) and s = s(xi_d).  The vertex is a MEDIUM vertex iff nothing was hit or
 *                         s < hit.t; otherwise it is the surface vertex of before.
 *     Surface vertex.     As without a medium, with one change: the emitter sample's Ld is the product of before, then
 *                         multiplied per component by Tr(dist), dist being the distance to the sampled point (before - kEpsilon).
 *                         Weights and densities are unchanged: the balance-heuristic weights ignore Tr in both strategies and
 *                         still sum to 1 per path.
 *     Medium vertex at p = o + d s  (per component: multiply, then add).  In this order:
 *                         1. T = T albedo; if T is zero in every component the path ends here and draws nothing more.
 *                         2. Russian roulette at depth >= 3 exactly as at a surface: one draw, p = min(max3(T) eta^2, 0.99).
 *                         3. path_ems / path_mis: an emitter sample, always four draws (xiE, xiT, xi); the pick and the point
 *                            as at a surface; dvec, dist2, dist, dir, cosY as there, rejected unless cosY > 0;
 *                            ph = HG(dot(d, dir));  pdfA = inv_area pdfPick;  pdf_em = (pdfA dist2) / cosY;  pdf_bsdf = ph;
 *                            Ld_c = ((ph rad_c) (cosY / (dist2 pdfA))) Tr(dist);  what the unoccluded shadow ray adds is
 *                            (T Ld) w, w = pdf_em / (pdf_em + ph) under path_mis and 1 under path_ems.  The shadow ray starts
 *                            at p with mint = kEpsilon and maxt = dist - kEpsilon.
 *                         4. a phase sample with two draws; pdf_mat = its pdf, the measure is solid angle, eta and T are
 *                            unchanged, depth += 1.
 *                         5. the next queries leave p with mint = kEpsilon, the shadow ray first, as at a surface.
 *                         An emitter hit after a medium vertex takes the wMat of before, with pdf_mat the phase density.
 *
 * nori_hip_set_medium           medium == NULL: no medium (the kernels and bits of before).  Else it is used from the next launch on;
 *                               nothing is allocated or launched.  NORI_ERR_NOT_READY before an upload; NORI_ERR_INVALID_ARGUMENT,
 *                               with a message, for a sigma_t that is not finite or outside [1e-4, 1e4], an albedo component that
 *                               is not finite or outside [0, 1], |g| > 0.99 (the bounds keep every quotient above inside the
 *                               verified domain of the device's division); NORI_ERR_UNSUPPORTED, with a message, for an
 *                               integrator other than the three path integrators and for a context with an environment map.  A
 *                               failed call leaves the context's medium as it was.
 * nori_hip_get_medium           1 and the medium as stored (g: 0 where |g| < 1e-3) if one is set, 0 if none, or a negative status.
 * nori_hip_medium_distance      s(xi) of n samples.
 * nori_hip_medium_transmittance Tr(dist) of n distances.
 * nori_hip_phase_eval           HG(dot(d, wo)) of n pairs of directions (d, wo: 3n each, unit length).
 * nori_hip_phase_sample         the phase sample of n directions d (3n) and pairs xi (2n): wo (3n) and pdf (n).
 * The last four return NORI_ERR_NOT_READY, with a message, while no medium is set. */
typedef struct nori_medium_desc {
    float sigma_t;         /* extinction, grey: 1e-4 .. 1e4 */
    float albedo[3];       /* single-scattering albedo, each 0 .. 1 */
    float g;               /* Henyey-Greenstein asymmetry, |g| <= 0.99; 0: isotropic */
} nori_medium_desc;
int nori_hip_set_medium(nori_hip_ctx *ctx, const nori_medium_desc *medium);
int nori_hip_get_medium(const nori_hip_ctx *ctx, nori_medium_desc *medium);
int nori_hip_medium_distance(nori_hip_ctx *ctx, const float *xi, size_t n, float *s);
int nori_hip_medium_transmittance(nori_hip_ctx *ctx, const float *dist, size_t n, float *tr);
int nori_hip_phase_eval(nori_hip_ctx *ctx, const float *d, const float *wo, size_t n, float *pdf);
int nori_hip_phase_sample(nori_hip_ctx *ctx, const float *d, const float *xi, size_t n, float *wo, float *pdf);
/* nori_hip_set_medium on every device's context (the upload resets it, as on one context) */
int nori_hip_group_set_medium(nori_hip_group *group, const nori_medium_desc *medium);

/* ------------------------------------------------------------------ Delta lights
 *
 * Lights without geometry: point, spot and directional.  No counterpart in the reference, whose only lamp without a mesh is the one
 * baked into the `simple` integrator.  They are a state of the context, set after the upload like the lens, the environment and
 * the medium and reset by the next upload; no struct of the scene description grows.  Without lights every kernel is the kernel it
 * was: path_ems and path_mis have three more sets of instantiations (rt_path.h, kDeltaLit) that only contexts with lights run --
 * "every BSDF, textures, lights", that with an environment, that with a medium; on the wavefront engine the full path record.
 * Every other integrator refuses lights (NORI_ERR_UNSUPPORTED): path_mats cannot reach a delta light.  A directional light and a
 * medium exclude each other (the medium fills all space, so the transmittance from infinity is 0): nori_hip_set_lights refuses the
 * light while a medium is set, nori_hip_set_medium refuses the medium while such a light is set.  NORI_SEED_NORI_BLOCK renders
 * refuse lights as they refuse a medium.  The feature pass and the first-hit frames are unchanged.
 *
 * Everything below is float32 without FMA contraction; every / is the correctly rounded quotient, every sqrt the correctly rounded
 * root; dot(a, b) = a.x b.x + (a.y b.y + a.z b.z); a vector / a scalar is three quotients.
 *
 *   The count and the pick.  nE = n_emitters + n_lights (+ 1 with an environment).  The emitter sample's first draw xiE selects
 *                         ei = min((uint32_t) (xiE (float) nE), nE - 1): [0, n_emitters) are the area emitters,
 *                         [n_emitters, n_emitters + n_lights) is delta light ei - n_emitters, n_emitters + n_lights is the
 *                         environment.  pdfPick = 1 / (float) nE.  The same nE enters the density of an emitter HIT
 *                         (inv_area / (float) nE), the environment's density on escape and the environment's own emitter sample.
 *                         A context with lights and no area emitter is valid: "no lights at all" is nE == 0.
 *   Draws.                A delta-light sample consumes the four draws of every emitter sample (xiE, xiT, xi); xiT and xi are unused.
 *   Incident(light, p).   What the twin returns as (dir, maxt, radiance); "no sample" is returned as zeros in all seven.
 *     POINT               dvec = position - p;  dist2 = dot(dvec, dvec);  dist2 == 0: no sample;  dist = sqrt(dist2);
 *                         dir = dvec / dist;  R = intensity;  maxt = dist - kEpsilon (1e-4).
 *     SPOT                as POINT, then c = dot(direction, -dir).  c <= cos_outer: no sample.  c >= cos_inner: R = intensity.
 *                         Otherwise t = (c - cos_outer) / (cos_inner - cos_outer);  fall = (t t) (3 - (2 t));  R = intensity fall.
 *                         cos_inner == cos_outer is a hard edge: one of the first two cases holds and no quotient is formed.
 *     DIRECTIONAL         dir = -direction;  R = intensity;  maxt = infinity.  There is no distance.
 *   At a surface vertex.  wo = toLocal(dir);  f = bsdf_eval(wi, wo);  f zero in every component: no sample.
 *                         POINT, SPOT: Ld = (f R) (wo.z / (dist2 pdfPick));  DIRECTIONAL: Ld = (f R) (wo.z / pdfPick) -- the area
 *                         light's expression with cosY = 1, pdfA = pdfPick and, for the directional light, dist2 = 1.  In a context
 *                         with a medium Ld is then multiplied by Tr(dist), as for an area light.
 *   At a medium vertex.   ph = HG(dot(d, dir));  Ld = ((ph R) (1 / (dist2 pdfPick))) Tr(dist).
 *   MIS.                  No BSDF or phase sample reaches a delta light: under path_mis its emitter sample carries the weight
 *                         exactly 1.0f, as under path_ems.  Nothing else in the weights changes but the count above.
 *   The shadow ray        starts at the vertex with mint = kEpsilon, direction dir and the maxt above.  It is traced, and counted in
 *                         n_shadow_rays, for every sample -- also where R or Ld is zero in every component (a black light, a
 *                         transmittance that underflowed).  A light nearer than 2 kEpsilon leaves maxt < mint (maxt < 0 for one
 *                         nearer than kEpsilon): the query is the query of every ray, a hit is a t with mint <= t <= maxt, there is
 *                         none, and the sample is added unoccluded.  The ray is still traced and counted.
 *
 * nori_hip_set_lights       n = 0 or lights == NULL: no lights (the kernels and bits of before).  Else the n lights replace the
 *                           stored ones and are used from the next launch on; directions are stored normalised (a / sqrt(dot(a, a)),
 *                           float32), fields a type does not use are stored as 0.  NORI_ERR_NOT_READY before an upload;
 *                           NORI_ERR_INVALID_ARGUMENT, with a message, for n above NORI_MAX_LIGHTS, an unknown type, a field in use
 *                           that is not finite, a negative intensity, a direction of zero length, a cone that does not satisfy
 *                           -1 <= cos_outer <= cos_inner <= 1; NORI_ERR_UNSUPPORTED, with a message, for an integrator other than
 *                           path_ems or path_mis and for a directional light in a context with a medium.  A failed call leaves the
 *                           stored lights as they were.
 * nori_hip_get_lights       *n = the number of lights stored; out[0 .. min(cap, *n)) = the lights as stored.  out may be NULL.
 * nori_hip_light_incident   Incident(light[k], p[3k ..]) of n pairs: dir (3n), maxt (n), radiance (3n).  NORI_ERR_NOT_READY while
 *                           no lights are set, NORI_ERR_INVALID_ARGUMENT for an index that is not below the number of lights. */
#define NORI_MAX_LIGHTS 4096
typedef enum nori_light_type { NORI_LIGHT_POINT = 0, NORI_LIGHT_SPOT = 1, NORI_LIGHT_DIRECTIONAL = 2 } nori_light_type;
typedef struct nori_light_desc {
    int32_t type;
    float position[3];     /* POINT, SPOT */
    float direction[3];    /* SPOT: the axis the light shines along; DIRECTIONAL: the direction the light travels.  Any non-zero length */
    float intensity[3];    /* POINT, SPOT: radiant intensity I (W/sr); DIRECTIONAL: irradiance E on a plane facing the light */
    float cos_inner, cos_outer;   /* SPOT: full intensity where c >= cos_inner, none where c <= cos_outer */
} nori_light_desc;
int nori_hip_set_lights(nori_hip_ctx *ctx, uint32_t n, const nori_light_desc *lights);
int nori_hip_get_lights(const nori_hip_ctx *ctx, uint32_t cap, nori_light_desc *out, uint32_t *n);
int nori_hip_light_incident(nori_hip_ctx *ctx, const uint32_t *light, const float *p, size_t n, float *dir, float *maxt, float *radiance);
/* nori_hip_set_lights on every device's context (the upload resets them, as on one context) */
int nori_hip_group_set_lights(nori_hip_group *group, uint32_t n, const nori_light_desc *lights);

/* ------------------------------------------------------------------ Grid medium
 *
 * A heterogeneous medium: ONE per context, as an alternative to the homogeneous one -- setting either replaces the other, and
 * nori_hip_set_medium with NULL unsets whichever is set.  An axis-aligned box [bmin, bmax] in world space holds nx ny nz voxels of
 * float32 density rho, x fastest (voxel (x, y, z) is rho[(z ny + y) nx + x]); a voxel's extinction is sigma = sigma_scale rho.  The
 * density is PIECEWISE CONSTANT (nearest voxel) and outside the box there is vacuum, so the optical depth along a ray is an exact
 * finite sum over the voxels a 3-D DDA visits: the free flight is sampled by analytic inversion (regular tracking) and the
 * transmittance is exp(-tau), deterministic.  Albedo and the Henyey-Greenstein g are the homogeneous medium's, and so is everything
 * after the distance and the transmittance: every closest-hit answer still draws exactly one number xi_d and every emitter sample
 * four, a medium vertex multiplies T by albedo and by nothing else, and its steps 1 - 5 are those of "Homogeneous participating
 * medium".  It is a state of the context set after the upload and reset by the next; path_mats, path_ems and path_mis render it
 * through sets of instantiations of their own (rt_path.h, kGridMedium: with and without delta lights), every other kernel is the
 * kernel it was.  A DIRECTIONAL light and a grid medium are allowed together (the box bounds the walk, the transmittance from
 * infinity is finite); an environment map is still refused -- no kernel set combines the two yet.
 *
 * Everything below is float32 without FMA contraction; 1 / x and a / b are the correctly rounded ones, log and exp the pinned ones
 * (DESIGN.md section 5).  min, max and clamps are selects on ONE comparison, written out here, so signed zeros take one way.
 *
 *   Derived once, on the host.  per axis a:  cell_a = (bmax_a - bmin_a) / (float) n_a;  inv_cell_a = (float) n_a / (bmax_a - bmin_a).
 *   walk(o, d, tmax, tau_stop).  t0 = 0;  t1 = tmax.  Per axis a, in the order x, y, z:
 *       PARALLEL iff |d_a| < 2^-40.  A parallel axis never steps (step_a = 0); the ray MISSES unless bmin_a <= o_a < bmax_a -- a
 *       point exactly on a plane belongs to the voxel ABOVE it, so o_a = bmax_a is outside.
 *       Otherwise inv_a = 1 / d_a;  step_a = d_a > 0 ? 1 : -1;  ta = (bmin_a - o_a) inv_a;  tb = (bmax_a - o_a) inv_a;
 *       tn = ta < tb ? ta : tb;  tf = ta < tb ? tb : ta;  t0 = tn > t0 ? tn : t0;  t1 = tf < t1 ? tf : t1.
 *     The ray misses, too, if all three axes are parallel or unless t0 < t1.  A miss: tau = 0, no event, 0 voxels.
 *     Entry voxel, per axis: p = o_a + d_a t0 (a parallel axis: p = o_a);  c = floor((p - bmin_a) inv_cell_a);
 *       c = c >= 0 ? c : 0;  c = c <= n_a - 1 ? c : n_a - 1;  i_a = (int) c.  Again a point on a plane belongs to the voxel above it,
 *       whichever way the ray travels: travelling down, its first segment is empty.
 *     t_cur = t0;  tau = 0.  Then at most nx + ny + nz trips (by construction: every trip but the last moves ONE index by one
 *     towards the face its axis leaves the box through, and the walk ends when an index leaves 0 .. n_a - 1):
 *       Plane crossings come from the INTEGER plane index, never from an accumulated step:  k_a = i_a + (step_a > 0 ? 1 : 0);
 *         t_a = ((bmin_a + (float) k_a cell_a) - o_a) inv_a;  a parallel axis: t_a = +inf.
 *       Ties step x, then y, then z:  sx = t_x <= t_y && t_x <= t_z;  sy = !sx && t_y <= t_z;  t_next = sx ? t_x : sy ? t_y : t_z.
 *       t_end = t_next < t1 ? t_next : t1;  sigma = sigma_scale rho[i];  len = t_end - t_cur;
 *       tau_new = tau + sigma (len > 0 ? len : 0).  The voxel counts as visited.
 *       EVENT iff sigma > 0 && tau_new >= tau_stop:  s = (t_cur + (tau_stop - tau) / sigma) + 0, and the walk ends (tau is the sum
 *         BEFORE this voxel).
 *       Else tau = tau_new;  the walk ends unless t_next < t1;  t_cur = t_next > t_cur ? t_next : t_cur;  the index of the stepping
 *       axis moves by its step;  the walk ends if it left its range.
 *   Distance(o, d, tmax, xi).     walk with tau_stop = -log(1 - xi):  s, or "no event" -- none before tmax or the box's far side.
 *   Transmittance(o, d, dist).    exp(-tau) of walk(o, d, dist, +inf).  dist may be +inf.
 *   In Li.                The closest-hit answer for the ray (o, d): xi_d is drawn as always;  walk with tmax = hit.t if something was
 *                         hit, else +inf.  MEDIUM vertex iff there is an event && (nothing was hit || s < hit.t), at p = o + d s.
 *                         No event and nothing hit: the path ends, like a miss without an environment.  An emitter sample's Ld is
 *                         multiplied by Transmittance(p, dir, dist) -- p the vertex, dist as for the homogeneous medium, +inf for a
 *                         directional light -- at surface and medium vertices alike; the MIS weights ignore it.
 *   Coincidence.          A 1 x 1 x 1 grid with rho = 1 whose box holds the origin and every hit of a closed scene gives the BITS of the
 *                         homogeneous medium with sigma_t = sigma_scale: t0 = 0, so s = (0 + q) + 0 with q = -log(1 - xi) / sigma_t,
 *                         the event test sigma hit.t >= tau_stop holds whenever q < hit.t, and tau = 0 + sigma_t dist.
 *   Domains.              Every divisor is a d_a with 2^-40 <= |d_a| (d is finite, |d_a| < 2^126) or a sigma in [1e-4, 1e4]: inside
 *                         the verified domain of the device's reciprocal.  o and tmax are finite or, tmax, +inf.
 *
 * nori_hip_set_grid_medium      medium == NULL: unsets a grid medium (a homogeneous one stays).  Else the voxels are copied to the
 *                               device and the medium is used from the next launch on, in place of any medium set before.
 *                               NORI_ERR_NOT_READY before an upload; NORI_ERR_INVALID_ARGUMENT, with a message, for nx, ny or nz
 *                               outside 1 .. 256, a box that is not finite with bmin < bmax on every axis, a sigma_scale that is not
 *                               finite or negative, albedo or g outside the homogeneous medium's bounds, and for the first voxel --
 *                               NAMED BY ITS INDEX -- whose rho is not finite or negative or whose sigma_scale rho is neither 0 nor
 *                               within [1e-4, 1e4]; NORI_ERR_UNSUPPORTED, with a message, for an integrator other than the three
 *                               path integrators and for a context with an environment map.  NORI_SEED_NORI_BLOCK renders refuse
 *                               it as they refuse the homogeneous medium.  A failed call leaves the context's medium as it was.
 * nori_hip_get_grid_medium      1 and the record as stored (rho NULL: the voxels are not read back; g: 0 where |g| < 1e-3) if a grid
 *                               medium is set, 0 if none, or a negative status.  nori_hip_get_medium returns 0 while a grid medium is
 *                               set, and this returns 0 while a homogeneous one is.
 * nori_hip_grid_medium_distance       Distance of n queries (o, d: 3n; tmax, xi: n); "no event" is returned as +inf.
 * nori_hip_grid_medium_transmittance  Transmittance of n queries.
 * nori_hip_grid_medium_optical_depth  tau and the number of voxels visited of walk(o, d, tmax, +inf), so a failing walk can be read.
 * The last three return NORI_ERR_NOT_READY, with a message, while no grid medium is set; nori_hip_medium_distance and
 * nori_hip_medium_transmittance do while one is (the phase twins serve both kinds of medium). */
typedef struct nori_grid_medium_desc {
    const float *rho;      /* nx ny nz densities, x fastest; each finite and >= 0 */
    int32_t nx, ny, nz;    /* each 1 .. 256 */
    float bmin[3], bmax[3];/* the box, world space; bmin < bmax per axis */
    float sigma_scale;     /* sigma = sigma_scale rho: 0, or 1e-4 .. 1e4 */
    float albedo[3];       /* single-scattering albedo, each 0 .. 1 */
    float g;               /* Henyey-Greenstein asymmetry, |g| <= 0.99; 0: isotropic */
} nori_grid_medium_desc;
int nori_hip_set_grid_medium(nori_hip_ctx *ctx, const nori_grid_medium_desc *medium);
int nori_hip_get_grid_medium(const nori_hip_ctx *ctx, nori_grid_medium_desc *medium);
int nori_hip_grid_medium_distance(nori_hip_ctx *ctx, const float *o, const float *d, const float *tmax, const float *xi, size_t n, float *s);
int nori_hip_grid_medium_transmittance(nori_hip_ctx *ctx, const float *o, const float *d, const float *dist, size_t n, float *tr);
int nori_hip_grid_medium_optical_depth(nori_hip_ctx *ctx, const float *o, const float *d, const float *tmax, size_t n, float *tau, int32_t *steps);
/* nori_hip_set_grid_medium on every device's context (the upload resets it, as on one context) */
int nori_hip_group_set_grid_medium(nori_hip_group *group, const nori_grid_medium_desc *medium);

#ifdef __cplusplus
}
#endif
#endif /* NORI_HIP_H */
