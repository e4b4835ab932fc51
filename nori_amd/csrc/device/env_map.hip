/*
 * env_map.hip -- the environment map's tables and operator twins, and the entry points that set it (include/nori_hip.h,
 * "Environment-map emitter"; env_map.h holds the per-lane code the path kernels share).
 *
 * The tables are built on the device with the arithmetic the path uses (exact_div, exact_sqrt), in three launches:
 *   env_weight_kernel    one lane per texel: lum(texel scale) / |c|^3
 *   env_row_cdf_kernel   one lane per ROW: the row's CDF in index order, a sequential float32 sum as DiscretePDF makes it -- a
 *                        parallel scan would add in another order and give other bits.  A lane walks its row from left to right,
 *                        so a wave reads 64 rows side by side (stride N floats): every 128-B line it touches is used for 32 trips
 *                        and stays in the CU's L1 meanwhile (64 lines = 8 KB per wave).  64-lane workgroups, so that a map of
 *                        4096 rows spreads over 64 CUs; the 16 M additions of such a map are a one-off of a few milliseconds.
 *   env_rows_kernel      one lane: the CDF of the N row sums, the same way
 * No atomics anywhere: the same map gives the same tables.
 */
#include "ctx.h"
#include "env_map.h"
#include <cmath>

namespace nrt {

namespace {

__global__ __launch_bounds__(256) void env_weight_kernel(EnvRec rec, float *weight) {
    const uint32_t n = rec.size;
    const size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (size_t) n * n) return;
    weight[k] = env_texel_weight(rec, (uint32_t) (k % n), (uint32_t) (k / n));
}

__global__ __launch_bounds__(64) void env_row_cdf_kernel(uint32_t n, const float *weight, float *col_cdf, float *row_sum) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const float *w = weight + (size_t) j * n;
    float *cdf = col_cdf + (size_t) j * (n + 1u);
    float acc = 0.0f;
    cdf[0] = 0.0f;
    for (uint32_t i = 0; i < n; ++i) { acc = acc + w[i]; cdf[i + 1u] = acc; }
    row_sum[j] = acc;
    if (acc > 0.0f)
        for (uint32_t i = 1; i <= n; ++i) cdf[i] = exact_div(cdf[i], acc);
}

__global__ void env_rows_kernel(uint32_t n, const float *row_sum, float *row_cdf) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float acc = 0.0f;
    row_cdf[0] = 0.0f;
    for (uint32_t j = 0; j < n; ++j) { acc = acc + row_sum[j]; row_cdf[j + 1u] = acc; }
    if (acc > 0.0f)
        for (uint32_t j = 1; j <= n; ++j) row_cdf[j] = exact_div(row_cdf[j], acc);
}

__global__ __launch_bounds__(256) void env_eval_kernel(const EnvRec *rec, const float *dirs, size_t n, float *rgb, float *pdf) {
    const size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const EnvRec e = *rec;
    float p;
    const f3 le = env_eval(e, mk3(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]), &p);
    rgb[3 * k] = le.x; rgb[3 * k + 1] = le.y; rgb[3 * k + 2] = le.z;
    if (pdf) pdf[k] = p;
}

__global__ __launch_bounds__(256) void env_sample_kernel(const EnvRec *rec, const float *xi, size_t n, float *dirs, float *rgb, float *pdf) {
    const size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const EnvRec e = *rec;
    f3 d, le; float p;
    env_sample(e, mk2(xi[2 * k], xi[2 * k + 1]), d, le, p);
    dirs[3 * k] = d.x; dirs[3 * k + 1] = d.y; dirs[3 * k + 2] = d.z;
    rgb[3 * k] = le.x; rgb[3 * k + 1] = le.y; rgb[3 * k + 2] = le.z;
    pdf[k] = p;
}

} // namespace

hipError_t env_build_tables(const EnvRec &rec, const EnvTables &t, hipStream_t s) {
    const uint32_t n = rec.size;
    const size_t texels = (size_t) n * n;
    /* the N row sums follow the N N weights: the caller allocates N N + N floats for `weight` */
    float *row_sum = t.weight + texels;
    hipLaunchKernelGGL(env_weight_kernel, dim3((unsigned) ((texels + 255) / 256)), dim3(256), 0, s, rec, t.weight);
    hipLaunchKernelGGL(env_row_cdf_kernel, dim3((n + 63u) / 64u), dim3(64), 0, s, n, (const float *) t.weight, t.col_cdf, row_sum);
    hipLaunchKernelGGL(env_rows_kernel, dim3(1), dim3(64), 0, s, n, (const float *) row_sum, t.row_cdf);
    return hipGetLastError();
}

} // namespace nrt

void env_release(nori_hip_ctx *ctx) {
    for (void *p : ctx->allocs_env) (void) hipFree(p);
    ctx->allocs_env.clear();
    ctx->dev.env = nullptr;
    ctx->env_size = 0; ctx->d_env_weight = nullptr;
}

namespace {

struct EnvAllocs {      /* freed unless they were handed to the context */
    std::vector<void *> p;
    ~EnvAllocs() { for (void *q : p) (void) hipFree(q); }
};

int env_alloc(nori_hip_ctx *ctx, EnvAllocs &a, size_t floats, float **out) {
    void *d = nullptr;
    HIP_TRY(ctx, hipMalloc(&d, std::max<size_t>(floats * sizeof(float), 16)));
    a.p.push_back(d);
    *out = (float *) d;
    return NORI_OK;
}

int env_check(nori_hip_ctx *ctx, const nori_env_desc *env) {
    if (env->size == 0 || env->size > kEnvMaxSize) { ctx->error = "set_environment: size must be 1 .. 4096 (got " + std::to_string(env->size) + ")"; return NORI_ERR_INVALID_ARGUMENT; }
    if (!env->texels) { ctx->error = "set_environment: texels is NULL"; return NORI_ERR_INVALID_ARGUMENT; }
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(env->scale[c]) || env->scale[c] < 0.0f) { ctx->error = "set_environment: scale must be finite and not negative"; return NORI_ERR_INVALID_ARGUMENT; }
    const size_t texels = (size_t) env->size * env->size;
    bool lit = false;
    for (size_t k = 0; k < texels; ++k) {
        const float *t = env->texels + 3 * k;
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(t[c]) || t[c] < 0.0f) {
                ctx->error = "set_environment: texel " + std::to_string(k) + " is negative or not finite (texels are linear RGB, finite, >= 0)";
                return NORI_ERR_INVALID_ARGUMENT;
            }
        if (!lit && env_luminance(mk3(t[0] * env->scale[0], t[1] * env->scale[1], t[2] * env->scale[2])) > 0.0f) lit = true;
    }
    if (!lit) { ctx->error = "set_environment: the map's scaled luminance is 0 everywhere (nothing to sample; pass NULL for no environment)"; return NORI_ERR_INVALID_ARGUMENT; }
    const float *m = env->to_world;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) {
            const double d = (double) m[3 * a] * m[3 * b] + (double) m[3 * a + 1] * m[3 * b + 1] + (double) m[3 * a + 2] * m[3 * b + 2];
            if (!(std::fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-4)) { ctx->error = "set_environment: to_world is not a rotation (its rows must be orthonormal within 1e-4)"; return NORI_ERR_INVALID_ARGUMENT; }
        }
    return NORI_OK;
}

int env_ready(nori_hip_ctx *ctx, const char *who) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene || !ctx->dev.env) { ctx->error = std::string(who) + ": no environment set"; return NORI_ERR_NOT_READY; }
    return NORI_OK;
}

} // namespace

extern "C" {

int nori_hip_set_environment(nori_hip_ctx *ctx, const nori_env_desc *env) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) { ctx->error = "set_environment: no scene uploaded"; return NORI_ERR_NOT_READY; }
    DeviceGuard g(ctx->device);
    if (!env) {
        HIP_TRY(ctx, hipDeviceSynchronize());      /* (a render still running reads the tables) */
        env_release(ctx);
        return NORI_OK;
    }
    if (ctx->host.integrator.type == NORI_INTEGRATOR_WHITTED) {
        ctx->error = "set_environment: the whitted integrator has no environment variant (it samples emitters and would need kernels of its own); use path_mats, path_ems or path_mis";
        return NORI_ERR_UNSUPPORTED;
    }
    if (ctx->dev.gmed.rho) {
        ctx->error = "set_environment: the context has a grid medium, and no kernel set combines a grid medium with an environment map yet; "
                     "unset the medium first (nori_hip_set_grid_medium with NULL)";
        return NORI_ERR_UNSUPPORTED;
    }
    if (ctx->dev.medium.on) {
        ctx->error = "set_environment: the context has a medium, and a medium that fills all space has zero transmittance to infinity; "
                     "unset the medium first (nori_hip_set_medium with NULL)";
        return NORI_ERR_UNSUPPORTED;
    }
    int rc = env_check(ctx, env);
    if (rc != NORI_OK) return rc;
    const uint32_t n = env->size;
    const size_t texels = (size_t) n * n;
    EnvAllocs a;
    float *d_texels, *d_weight, *d_rows, *d_cols, *d_rec;
    if ((rc = env_alloc(ctx, a, 3 * texels, &d_texels))) return rc;
    if ((rc = env_alloc(ctx, a, texels + n, &d_weight))) return rc;      /* the weights, then the row sums */
    if ((rc = env_alloc(ctx, a, n + 1u, &d_rows))) return rc;
    if ((rc = env_alloc(ctx, a, (size_t) n * (n + 1u), &d_cols))) return rc;
    if ((rc = env_alloc(ctx, a, (sizeof(EnvRec) + sizeof(float) - 1) / sizeof(float), &d_rec))) return rc;
    HIP_TRY(ctx, hipMemcpy(d_texels, env->texels, 3 * texels * sizeof(float), hipMemcpyHostToDevice));
    EnvRec rec;
    rec.texels = d_texels; rec.row_cdf = d_rows; rec.col_cdf = d_cols; rec.size = n;
    for (int c = 0; c < 3; ++c) rec.scale[c] = env->scale[c];
    for (int k = 0; k < 9; ++k) rec.m[k] = env->to_world[k];
    EnvTables t; t.weight = d_weight; t.row_cdf = d_rows; t.col_cdf = d_cols;
    HIP_TRY(ctx, env_build_tables(rec, t, 0));
    HIP_TRY(ctx, hipMemcpy(d_rec, &rec, sizeof(rec), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipDeviceSynchronize());
    env_release(ctx);
    ctx->allocs_env.swap(a.p);
    ctx->dev.env = reinterpret_cast<const EnvRec *>(d_rec);
    ctx->env_size = n; ctx->d_env_weight = d_weight;
    return NORI_OK;
}

int nori_hip_get_environment(const nori_hip_ctx *ctx, uint32_t *size) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return NORI_ERR_NOT_READY;      /* (the context is const: no message) */
    if (size) *size = ctx->dev.env ? ctx->env_size : 0u;
    return NORI_OK;
}

int nori_hip_env_eval(nori_hip_ctx *ctx, const float *dirs, size_t n, float *rgb, float *pdf) {
    const int ready = env_ready(ctx, "env_eval");
    if (ready != NORI_OK) return ready;
    if (n == 0) return NORI_OK;
    if (!dirs || !rgb) { ctx->error = "env_eval: null array"; return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    SCRATCH_IN(ctx, dd, dirs, n * 3 * sizeof(float));
    SCRATCH_OUT(ctx, dc, n * 3 * sizeof(float));
    SCRATCH_OUT(ctx, dp, n * sizeof(float));
    hipLaunchKernelGGL(env_eval_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, ctx->dev.env, (const float *) dd.p, n,
                       (float *) dc.p, pdf ? (float *) dp.p : (float *) nullptr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpy(rgb, dc.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (pdf) HIP_TRY(ctx, hipMemcpy(pdf, dp.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return NORI_OK;
}

int nori_hip_env_sample(nori_hip_ctx *ctx, const float *xi, size_t n, float *dirs, float *rgb, float *pdf) {
    const int ready = env_ready(ctx, "env_sample");
    if (ready != NORI_OK) return ready;
    if (n == 0) return NORI_OK;
    if (!xi || !dirs || !rgb || !pdf) { ctx->error = "env_sample: null array"; return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    SCRATCH_IN(ctx, dx, xi, n * 2 * sizeof(float));
    SCRATCH_OUT(ctx, dd, n * 3 * sizeof(float));
    SCRATCH_OUT(ctx, dc, n * 3 * sizeof(float));
    SCRATCH_OUT(ctx, dp, n * sizeof(float));
    hipLaunchKernelGGL(env_sample_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, ctx->dev.env, (const float *) dx.p, n,
                       (float *) dd.p, (float *) dc.p, (float *) dp.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpy(dirs, dd.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(rgb, dc.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(pdf, dp.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return NORI_OK;
}

int nori_hip_debug_env_tables(nori_hip_ctx *ctx, float *row_cdf, float *col_cdf, float *texel_weight) {
    const int ready = env_ready(ctx, "debug_env_tables");
    if (ready != NORI_OK) return ready;
    DeviceGuard g(ctx->device);
    const size_t n = ctx->env_size;
    EnvRec rec;
    HIP_TRY(ctx, hipMemcpy(&rec, ctx->dev.env, sizeof(rec), hipMemcpyDeviceToHost));
    if (row_cdf) HIP_TRY(ctx, hipMemcpy(row_cdf, rec.row_cdf, (n + 1) * sizeof(float), hipMemcpyDeviceToHost));
    if (col_cdf) HIP_TRY(ctx, hipMemcpy(col_cdf, rec.col_cdf, n * (n + 1) * sizeof(float), hipMemcpyDeviceToHost));
    if (texel_weight) HIP_TRY(ctx, hipMemcpy(texel_weight, ctx->d_env_weight, n * n * sizeof(float), hipMemcpyDeviceToHost));
    return NORI_OK;
}

} // extern "C"
