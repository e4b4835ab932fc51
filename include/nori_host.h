/*
 * nori_host.h -- C ABI of libnori_host.so, the C++ host that keeps Nori's
 * NoriObject / XML plugin surface (loadFromXML, src/parser.cpp:16).  It lets a
 * non-C++ caller (the Python tests and bench.py) load an unmodified Nori scene
 * file and obtain the flattened nori_scene_desc that include/nori_hip.h
 * consumes, or enumerate the contents of a <test> file.
 *
 * Load-time only; no per-sample work happens behind these calls.
 */
#ifndef NORI_HOST_H
#define NORI_HOST_H

#include "nori_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nori_host_root nori_host_root;

/* flags for nori_host_load_xml */
#define NORI_HOST_DEFER_TESTS 1   /* do not run <test> objects inside activate() */
#define NORI_HOST_QUIET 2         /* no "Configuration: ..." / OBJ loader chatter  */

/* Parse `path` (resources resolve relative to its directory, src/main.cpp:190).
 * Returns 0 or a negative nori_status; message via nori_host_last_error(). */
int nori_host_load_xml(const char *path, int flags, nori_host_root **out);
void nori_host_free(nori_host_root *root);
const char *nori_host_last_error(void);

/* NoriObject::EClassType of the root (0 = scene, 9 = test, ...) and its toString() */
int nori_host_root_type(const nori_host_root *root);
const char *nori_host_root_string(const nori_host_root *root);

/* Root is a <scene>: borrow its flattened description (valid until free). */
int nori_host_scene_desc(const nori_host_root *root, nori_scene_desc *out);

/* Root is a <scene>: the thin lens of its camera (apertureRadius, default 0 = the pinhole, and focusDistance, default 1, of
 * the <camera>'s property list).  Not part of nori_scene_desc: apply it with nori_hip_set_lens after the upload, as
 * nori_host_render does.  Either pointer may be NULL. */
int nori_host_lens(const nori_host_root *root, float *radius, float *focus);
/* Root is a <scene>: its environment map (<emitter type="envmap">), resampled to the octahedral layout nori_hip_set_environment
 * takes; the texels are borrowed (valid until free).  Returns 1 and fills *out if the scene has one, 0 if it has none (out->size = 0),
 * or a negative nori_status.  Not part of nori_scene_desc: apply it after the upload. */
int nori_host_environment(const nori_host_root *root, nori_env_desc *out);
/* Root is a <scene>: its medium (<medium type="homogeneous">, with its <phase> child's g), the record nori_hip_set_medium takes.
 * Returns 1 and fills *out if the scene has one, 0 if it has none, or a negative nori_status.  Not part of nori_scene_desc: apply
 * it after the upload. */
int nori_host_medium(const nori_host_root *root, nori_medium_desc *out);
/* Root is a <scene>: its grid medium (<medium type="grid">: a VOL file, sigmaScale, albedo, its <phase> child's g, boxMin / boxMax), the
 * record nori_hip_set_grid_medium takes; the voxels are borrowed (valid until free).  Returns 1 and fills *out if the scene has one,
 * 0 if it has none -- nori_host_medium returns 0 for a scene whose medium is a grid --, or a negative nori_status. */
int nori_host_grid_medium(const nori_host_root *root, nori_grid_medium_desc *out);
/* Root is a <scene>: its delta lights (<emitter type="point|spot|directional"> under the <scene>), the records nori_hip_set_lights
 * takes, in the file's order.  *n = their number; out[0 .. min(cap, *n)) is filled (out may be NULL).  Not part of nori_scene_desc:
 * apply them after the upload. */
int nori_host_lights(const nori_host_root *root, uint32_t cap, nori_light_desc *out, uint32_t *n);

/* Root is a <test>: kind 0 = ttest, 1 = chi2test. */
typedef struct nori_host_test_info {
    int32_t kind;
    float significance_level;
    int32_t sample_count;
    int32_t test_count;          /* chi2test */
    int32_t resolution;          /* chi2test: cos(theta) cells; phi cells = 2x */
    int32_t min_exp_frequency;   /* chi2test */
    uint32_t n_angles, n_references, n_bsdfs, n_scenes;
    const float *angles;
    const float *references;
} nori_host_test_info;
int nori_host_test_info_get(const nori_host_root *root, nori_host_test_info *out);
int nori_host_test_bsdf(const nori_host_root *root, uint32_t index, nori_bsdf_desc *out);
int nori_host_test_scene_desc(const nori_host_root *root, uint32_t index, nori_scene_desc *out);
/* Run the test on the GPU now (what activate() does when not deferred);
 * 0 = all passed, 1 = some failed (report on stdout), < 0 = error. */
int nori_host_test_run(nori_host_root *root);

/* render() of src/main.cpp:58-148 for a <scene> root on the GPU: fills the
 * caller's RGBW frame ((h+2b) x (w+2b) x 4 floats) and optional stats. */
int nori_host_render(nori_host_root *root, float *rgbw, nori_render_stats *stats);
/* Write rgb (h x w x 3 floats) as `<basename>.exr` and `<basename>.png`
 * (Bitmap::saveEXR / savePNG, src/bitmap.cpp:69-122). */
int nori_host_save_images(const char *basename, const float *rgb, int width, int height);
/* Read an OpenEXR file written by Nori / this library into rgb (caller frees
 * with nori_host_free_buffer). */
int nori_host_load_exr(const char *path, float **rgb, int *width, int *height);
void nori_host_free_buffer(void *p);

#ifdef __cplusplus
}
#endif
#endif
