/*
 * env_map.h -- the environment-map emitter (include/nori_hip.h, nori_env_desc, states every operation; tests/envmap_ref.py
 * restates it in numpy and the device is held to that bit for bit).
 *
 * The reference has no environment emitter (Scene::addChild(EEmitter) throws): nothing of this is pinned by it.  The map is
 * OCTAHEDRAL -- a direction is divided by its 1-norm and the lower half of the octahedron is folded over the upper one into the
 * square [-1, 1]^2 -- so that direction <-> texel needs + - x / |x| and a square root only, the operations this renderer has
 * pinned (rt_types.h: exact_div, exact_sqrt; float32, no contraction).  A latitude-longitude map would need atan2 and acos.
 *
 * Storage (device memory, made by env_map.hip when the environment is set): the N x N texels as they were given (3 floats, row
 * major, texel (i, j) = column i of row j covers u in [i/N, (i+1)/N), v in [j/N, (j+1)/N)), the CDF over the rows (N + 1 floats)
 * and one CDF over the columns per row (N x (N + 1) floats), and an EnvRec that names them.  DevScene::env points at the record;
 * null: no environment, and no kernel compiled without kEnvLit (rt_path.h) reads it.
 */
#pragma once
#include "rt_types.h"

namespace nrt {

constexpr uint32_t kEnvMaxSize = 4096u;

struct EnvRec {
    const float *texels;       /* 3 N N */
    const float *row_cdf;      /* N + 1: the CDF of the row sums */
    const float *col_cdf;      /* N (N + 1): row j's CDF over its columns at j (N + 1) */
    uint32_t size;             /* N */
    float scale[3];
    float m[9];                /* row-major rotation, world = M local */
};

/* src/common.cpp:247-249 (Color3f::getLuminance), left to right */
NORI_HD float env_luminance(f3 c) { return (c.x * 0.212671f + c.y * 0.715160f) + c.z * 0.072169f; }

/* the fold of the octahedron's lower half (pz < 0) over the square, which is its own inverse; sgn(0) = +1 */
NORI_HD void env_fold(float &px, float &py) {
    const float ox = px, oy = py;
    px = (1.0f - fabsf(oy)) * (ox >= 0.0f ? 1.0f : -1.0f);
    py = (1.0f - fabsf(ox)) * (oy >= 0.0f ? 1.0f : -1.0f);
}

/* world direction -> the point of the octahedron |x| + |y| + |z| = 1 it passes through (q, local frame, not folded) and its
   place (u, v) in the unit square */
NORI_HD void env_dir_to_uv(const EnvRec &e, f3 d, f3 &q, float &u, float &v) {
    const f3 l = mk3(dot(mk3(e.m[0], e.m[3], e.m[6]), d), dot(mk3(e.m[1], e.m[4], e.m[7]), d), dot(mk3(e.m[2], e.m[5], e.m[8]), d));      /* M^T d */
    const float s = (fabsf(l.x) + fabsf(l.y)) + fabsf(l.z);
    q = l / s;
    float px = q.x, py = q.y;
    if (q.z < 0.0f) env_fold(px, py);
    u = px * 0.5f + 0.5f;
    v = py * 0.5f + 0.5f;
}

NORI_HD void env_uv_to_texel(uint32_t n, float u, float v, uint32_t &i, uint32_t &j) {
    const int ii = (int) (u * (float) n), jj = (int) (v * (float) n), last = (int) n - 1;
    i = (uint32_t) (ii < 0 ? 0 : (ii < last ? ii : last));      /* (below 0: a direction that is not finite) */
    j = (uint32_t) (jj < 0 ? 0 : (jj < last ? jj : last));
}

NORI_HD f3 env_texel(const EnvRec &e, uint32_t i, uint32_t j) {
    const float *t = e.texels + ((size_t) j * e.size + i) * 3u;
    return mk3(t[0] * e.scale[0], t[1] * e.scale[1], t[2] * e.scale[2]);
}

/* |c|^3 of a point of the octahedron: n sqrt(n), n = c . c */
NORI_HD float env_cube_of_length(f3 c) { const float n = dot(c, c); return n * exact_sqrt(n); }

/* the solid-angle density of the direction whose octahedron point is q and whose texel is (i, j):
   P(row j) P(column i | row j) (N N / 4) |q|^3 */
NORI_HD float env_pdf_at(const EnvRec &e, f3 q, uint32_t i, uint32_t j) {
    const float fn = (float) e.size;
    const float *cc = e.col_cdf + (size_t) j * (e.size + 1u);
    const float p = (e.row_cdf[j + 1u] - e.row_cdf[j]) * (cc[i + 1u] - cc[i]);
    return (p * ((fn * fn) * 0.25f)) * env_cube_of_length(q);
}

/* Le(d) and, if asked for, pdf_omega(d) */
NORI_HD f3 env_eval(const EnvRec &e, f3 d, float *pdf) {
    f3 q; float u, v; uint32_t i, j;
    env_dir_to_uv(e, d, q, u, v);
    env_uv_to_texel(e.size, u, v, i, j);
    if (pdf) *pdf = env_pdf_at(e, q, i, j);
    return env_texel(e, i, j);
}

/* DiscretePDF::sample (include/nori/dpdf.h:106-111, std::lower_bound) on entries [0, n] of cdf, and the sample reused:
   (xi - cdf[k]) / (cdf[k+1] - cdf[k]); an entry of probability zero -- reached by xi = 0 only -- is entered at its middle */
NORI_HD uint32_t env_cdf_pick(const float *cdf, uint32_t n, float xi, float &reuse) {
    uint32_t lo = 0, len = n + 1u;
    while (len > 0u) {
        const uint32_t half = len >> 1, mid = lo + half;
        if (cdf[mid] < xi) { lo = mid + 1u; len -= half + 1u; }
        else len = half;
    }
    uint32_t k = lo > 0u ? lo - 1u : 0u;
    k = k < n - 1u ? k : n - 1u;
    const float den = cdf[k + 1u] - cdf[k];
    reuse = den > 0.0f ? exact_div(xi - cdf[k], den) : 0.5f;
    return k;
}

/* the direction the sample xi selects; Le and the density are those env_eval gives for that direction */
NORI_HD void env_sample(const EnvRec &e, f2 xi, f3 &d, f3 &le, float &pdf) {
    const float fn = (float) e.size;
    float ty, tx;
    const uint32_t j = env_cdf_pick(e.row_cdf, e.size, xi.y, ty);
    const uint32_t i = env_cdf_pick(e.col_cdf + (size_t) j * (e.size + 1u), e.size, xi.x, tx);
    const float u = exact_div((float) i + tx, fn), v = exact_div((float) j + ty, fn);
    float px = u * 2.0f - 1.0f, py = v * 2.0f - 1.0f;
    const float pz = (1.0f - fabsf(px)) - fabsf(py);
    if (pz < 0.0f) env_fold(px, py);
    const f3 l = normalized(mk3(px, py, pz));
    d = mk3(dot(mk3(e.m[0], e.m[1], e.m[2]), l), dot(mk3(e.m[3], e.m[4], e.m[5]), l), dot(mk3(e.m[6], e.m[7], e.m[8]), l));      /* M l */
    le = env_eval(e, d, &pdf);
}

/* the weight of texel (i, j) in the sampling tables: lum(texel scale) / |c|^3, c the octahedron point of the texel's centre */
NORI_HD float env_texel_weight(const EnvRec &e, uint32_t i, uint32_t j) {
    const float fn = (float) e.size;
    const float u = exact_div((float) i + 0.5f, fn), v = exact_div((float) j + 0.5f, fn);
    float px = u * 2.0f - 1.0f, py = v * 2.0f - 1.0f;
    const float pz = (1.0f - fabsf(px)) - fabsf(py);
    if (pz < 0.0f) env_fold(px, py);
    return exact_div(env_luminance(env_texel(e, i, j)), env_cube_of_length(mk3(px, py, pz)));
}

/* env_map.hip: the tables of a map already in device memory.  rec->texels / scale / size are set; the weights go to `weight`
   (N N), the CDFs to row_cdf / col_cdf.  Three launches on stream s, no atomics: the same map gives the same tables. */
struct EnvTables { float *weight, *row_cdf, *col_cdf; };
#if defined(__HIPCC__)
hipError_t env_build_tables(const EnvRec &rec, const EnvTables &t, hipStream_t s);
#endif

} // namespace nrt
