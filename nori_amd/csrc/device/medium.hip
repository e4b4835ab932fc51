/*
 * medium.hip -- the entry points that set the context's homogeneous medium, and the operator twins of its four operations
 * (include/nori_hip.h, "Homogeneous participating medium"; medium.h holds the per-lane code the path kernels share).
 *
 * The medium is 40 bytes of DevScene, by value: setting it allocates nothing and launches nothing.  The twins run the functions of
 * medium.h, one lane per element, in two small kernels:
 *   medium_scalar_kernel    free-flight distances from samples, or transmittances from distances
 *   medium_phase_kernel     the phase density of direction pairs, or a phase sample and its density
 */
#include "ctx.h"
#include "medium.h"
#include <cmath>

namespace {

using namespace nrt;

/* what 0: out[k] = medium_distance(in[k]);  1: out[k] = medium_tr(in[k])  (uniform over the launch) */
__global__ __launch_bounds__(256) void medium_scalar_kernel(MediumRec m, int what, const float *in, size_t n, float *out) {
    const size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    out[k] = what == 0 ? medium_distance(m, in[k]) : medium_tr(m, in[k]);
}

/* sample 0: pdf[k] = HG(dot(d, wo)) of the given wo (in: 3n);  1: wo = the phase sample of xi (in: 2n), pdf its density */
__global__ __launch_bounds__(256) void medium_phase_kernel(MediumRec m, int sample, const float *d, const float *in, size_t n, float *wo, float *pdf) {
    const size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const f3 dir = mk3(d[3 * k], d[3 * k + 1], d[3 * k + 2]);
    if (sample) {
        float p;
        const f3 w = hg_sample(m, dir, mk2(in[2 * k], in[2 * k + 1]), p);
        wo[3 * k] = w.x; wo[3 * k + 1] = w.y; wo[3 * k + 2] = w.z;
        pdf[k] = p;
    } else {
        pdf[k] = hg_eval(m, dot(dir, mk3(in[3 * k], in[3 * k + 1], in[3 * k + 2])));
    }
}

int medium_ready(nori_hip_ctx *ctx, const char *who) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene || !ctx->dev.medium.on) { ctx->error = std::string(who) + ": no medium set"; return NORI_ERR_NOT_READY; }
    return NORI_OK;
}

unsigned blocks_of(size_t n) { return (unsigned) ((n + 255) / 256); }

} // namespace

extern "C" {

int nori_hip_set_medium(nori_hip_ctx *ctx, const nori_medium_desc *medium) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) { ctx->error = "set_medium: no scene uploaded"; return NORI_ERR_NOT_READY; }
    if (!medium) {      /* (a render still running has its own copy of the record: kernel arguments) */
        DeviceGuard g(ctx->device);
        grid_medium_release(ctx);      /* no medium of either kind */
        ctx->dev.medium = MediumRec();
        return NORI_OK;
    }
    if (!(std::isfinite(medium->sigma_t) && medium->sigma_t >= 1e-4f && medium->sigma_t <= 1e4f)) {
        ctx->error = "set_medium: sigma_t must be finite and lie in [1e-4, 1e4] (got " + std::to_string(medium->sigma_t) + ")";
        return NORI_ERR_INVALID_ARGUMENT;
    }
    for (int c = 0; c < 3; ++c)
        if (!(std::isfinite(medium->albedo[c]) && medium->albedo[c] >= 0.0f && medium->albedo[c] <= 1.0f)) {
            ctx->error = "set_medium: every albedo component must be finite and lie in [0, 1] (got " + std::to_string(medium->albedo[c]) + ")";
            return NORI_ERR_INVALID_ARGUMENT;
        }
    if (!(std::fabs(medium->g) <= 0.99f)) {
        ctx->error = "set_medium: the Henyey-Greenstein asymmetry g must lie in [-0.99, 0.99] (got " + std::to_string(medium->g) + ")";
        return NORI_ERR_INVALID_ARGUMENT;
    }
    const int integ = ctx->host.integrator.type;
    if (integ != NORI_INTEGRATOR_PATH_MATS && integ != NORI_INTEGRATOR_PATH_EMS && integ != NORI_INTEGRATOR_PATH_MIS) {
        ctx->error = "set_medium: only path_mats, path_ems and path_mis render a medium (the other integrators have no variant for it)";
        return NORI_ERR_UNSUPPORTED;
    }
    if (ctx->dev.env) {
        ctx->error = "set_medium: the context has an environment map, and a medium that fills all space has zero transmittance to infinity; "
                     "unset the environment first (nori_hip_set_environment with NULL)";
        return NORI_ERR_UNSUPPORTED;
    }
    for (const LightRec &l : ctx->host_lights)
        if (l.type == kLightDirectional) {
            ctx->error = "set_medium: the context holds a directional light, and a medium that fills all space has zero transmittance from infinity; "
                         "unset the lights first (nori_hip_set_lights with n = 0)";
            return NORI_ERR_UNSUPPORTED;
        }
    {
        DeviceGuard g(ctx->device);
        grid_medium_release(ctx);      /* one medium per context: the homogeneous one replaces a grid (nori_hip_set_grid_medium) */
    }
    ctx->dev.medium = medium_record(medium->sigma_t, medium->albedo, medium->g);
    return NORI_OK;
}

int nori_hip_get_medium(const nori_hip_ctx *ctx, nori_medium_desc *medium) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return NORI_ERR_NOT_READY;      /* (the context is const: no message) */
    if (ctx->dev.gmed.rho) {      /* a grid medium is set (nori_hip_get_grid_medium reads it): none here */
        if (medium) *medium = nori_medium_desc();
        return 0;
    }
    const MediumRec &m = ctx->dev.medium;
    if (medium) {
        medium->sigma_t = m.sigma_t; medium->g = m.g;
        for (int c = 0; c < 3; ++c) medium->albedo[c] = m.albedo[c];
    }
    return m.on ? 1 : 0;
}

int nori_hip_medium_distance(nori_hip_ctx *ctx, const float *xi, size_t n, float *s) {
    const int ready = medium_ready(ctx, "medium_distance");
    if (ready != NORI_OK) return ready;
    if (ctx->dev.gmed.rho) { ctx->error = "medium_distance: the context's medium is a grid (nori_hip_grid_medium_distance)"; return NORI_ERR_NOT_READY; }
    if (n == 0) return NORI_OK;
    if (!xi || !s) { ctx->error = "medium_distance: null array"; return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    SCRATCH_IN(ctx, di, xi, n * sizeof(float));
    SCRATCH_OUT(ctx, dout, n * sizeof(float));
    hipLaunchKernelGGL(medium_scalar_kernel, dim3(blocks_of(n)), dim3(256), 0, 0, ctx->dev.medium, 0, (const float *) di.p, n, (float *) dout.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpy(s, dout.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return NORI_OK;
}

int nori_hip_medium_transmittance(nori_hip_ctx *ctx, const float *dist, size_t n, float *tr) {
    const int ready = medium_ready(ctx, "medium_transmittance");
    if (ready != NORI_OK) return ready;
    if (ctx->dev.gmed.rho) { ctx->error = "medium_transmittance: the context's medium is a grid (nori_hip_grid_medium_transmittance)"; return NORI_ERR_NOT_READY; }
    if (n == 0) return NORI_OK;
    if (!dist || !tr) { ctx->error = "medium_transmittance: null array"; return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    SCRATCH_IN(ctx, di, dist, n * sizeof(float));
    SCRATCH_OUT(ctx, dout, n * sizeof(float));
    hipLaunchKernelGGL(medium_scalar_kernel, dim3(blocks_of(n)), dim3(256), 0, 0, ctx->dev.medium, 1, (const float *) di.p, n, (float *) dout.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpy(tr, dout.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return NORI_OK;
}

int nori_hip_phase_eval(nori_hip_ctx *ctx, const float *d, const float *wo, size_t n, float *pdf) {
    const int ready = medium_ready(ctx, "phase_eval");
    if (ready != NORI_OK) return ready;
    if (n == 0) return NORI_OK;
    if (!d || !wo || !pdf) { ctx->error = "phase_eval: null array"; return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    SCRATCH_IN(ctx, dd, d, n * 3 * sizeof(float));
    SCRATCH_IN(ctx, dw, wo, n * 3 * sizeof(float));
    SCRATCH_OUT(ctx, dp, n * sizeof(float));
    hipLaunchKernelGGL(medium_phase_kernel, dim3(blocks_of(n)), dim3(256), 0, 0, ctx->dev.medium, 0, (const float *) dd.p, (const float *) dw.p, n,
                       (float *) nullptr, (float *) dp.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpy(pdf, dp.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return NORI_OK;
}

int nori_hip_phase_sample(nori_hip_ctx *ctx, const float *d, const float *xi, size_t n, float *wo, float *pdf) {
    const int ready = medium_ready(ctx, "phase_sample");
    if (ready != NORI_OK) return ready;
    if (n == 0) return NORI_OK;
    if (!d || !xi || !wo || !pdf) { ctx->error = "phase_sample: null array"; return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    SCRATCH_IN(ctx, dd, d, n * 3 * sizeof(float));
    SCRATCH_IN(ctx, dx, xi, n * 2 * sizeof(float));
    SCRATCH_OUT(ctx, dw, n * 3 * sizeof(float));
    SCRATCH_OUT(ctx, dp, n * sizeof(float));
    hipLaunchKernelGGL(medium_phase_kernel, dim3(blocks_of(n)), dim3(256), 0, 0, ctx->dev.medium, 1, (const float *) dd.p, (const float *) dx.p, n,
                       (float *) dw.p, (float *) dp.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpy(wo, dw.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(pdf, dp.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return NORI_OK;
}

} // extern "C"
