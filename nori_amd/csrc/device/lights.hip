/*
 * lights.hip -- the entry points that set the context's delta lights, and the operator twin of what a light sends towards a point
 * (include/nori_hip.h, "Delta lights"; lights.h holds the per-lane code the path kernels share).
 *
 * The lights are an array of 48-byte records in device memory that DevScene::lights points at; the setter checks every record,
 * normalises the directions and replaces the array.  The twin runs light_incident of lights.h, one lane per element:
 *   light_incident_kernel   (dir, maxt, radiance) of n pairs (light index, point)
 */
#include "ctx.h"
#include "lights.h"
#include <cmath>
#include <cstring>

namespace {

using namespace nrt;

__global__ __launch_bounds__(256) void light_incident_kernel(const LightRec *lights, const uint32_t *light, const float *p, size_t n,
                                                             float *dir, float *maxt, float *radiance) {
    const size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    f3 w, R; float hi, dist2, dist;
    const bool ok = light_incident(lights[light[k]], mk3(p[3 * k], p[3 * k + 1], p[3 * k + 2]), w, hi, R, dist2, dist);
    if (!ok) { w = mk3(0.0f); R = mk3(0.0f); hi = 0.0f; }      /* no sample: zeros */
    dir[3 * k] = w.x; dir[3 * k + 1] = w.y; dir[3 * k + 2] = w.z;
    radiance[3 * k] = R.x; radiance[3 * k + 1] = R.y; radiance[3 * k + 2] = R.z;
    maxt[k] = hi;
}

/* the record of a description, or why it has none */
std::string light_record(const nori_light_desc &l, uint32_t k, LightRec &r) {
    const std::string who = "set_lights: light " + std::to_string(k) + ": ";
    if (l.type != NORI_LIGHT_POINT && l.type != NORI_LIGHT_SPOT && l.type != NORI_LIGHT_DIRECTIONAL) return who + "unknown type " + std::to_string(l.type);
    const bool has_pos = l.type != NORI_LIGHT_DIRECTIONAL, has_dir = l.type != NORI_LIGHT_POINT, spot = l.type == NORI_LIGHT_SPOT;
    std::memset(&r, 0, sizeof(r));
    r.type = l.type;
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(l.intensity[c])) return who + "a component of the intensity is not finite";
        if (l.intensity[c] < 0.0f) return who + "a component of the intensity is negative (" + std::to_string(l.intensity[c]) + ")";
        r.intensity[c] = l.intensity[c];
        if (has_pos) {
            if (!std::isfinite(l.position[c])) return who + "a component of the position is not finite";
            r.position[c] = l.position[c];
        }
        if (has_dir && !std::isfinite(l.direction[c])) return who + "a component of the direction is not finite";
    }
    if (has_dir) {
        const f3 a = mk3(l.direction[0], l.direction[1], l.direction[2]);
        const float z = dot(a, a);
        if (!(z > 0.0f) || !std::isfinite(z)) return who + "the direction has zero length (or one whose square is not finite)";
        const f3 u = normalized(a);
        r.direction[0] = u.x; r.direction[1] = u.y; r.direction[2] = u.z;
    }
    if (spot) {
        if (!std::isfinite(l.cos_inner) || !std::isfinite(l.cos_outer)) return who + "a cosine of the cone is not finite";
        if (!(-1.0f <= l.cos_outer && l.cos_outer <= l.cos_inner && l.cos_inner <= 1.0f))
            return who + "the cone needs -1 <= cos_outer <= cos_inner <= 1 (got cos_inner " + std::to_string(l.cos_inner) + ", cos_outer " + std::to_string(l.cos_outer) + ")";
        r.cos_inner = l.cos_inner; r.cos_outer = l.cos_outer;
    }
    return std::string();
}

} // namespace

void lights_release(nori_hip_ctx *ctx) {
    if (ctx->d_lights) (void) hipFree(ctx->d_lights);
    ctx->d_lights = nullptr;
    ctx->host_lights.clear();
    ctx->dev.lights = nullptr;
    ctx->dev.n_lights = 0u;
}

extern "C" {

int nori_hip_set_lights(nori_hip_ctx *ctx, uint32_t n, const nori_light_desc *lights) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) { ctx->error = "set_lights: no scene uploaded"; return NORI_ERR_NOT_READY; }
    DeviceGuard g(ctx->device);
    if (n == 0 || !lights) {
        lights_release(ctx);
        return NORI_OK;
    }
    if (n > NORI_MAX_LIGHTS) {
        ctx->error = "set_lights: " + std::to_string(n) + " lights, at most " + std::to_string(NORI_MAX_LIGHTS);
        return NORI_ERR_INVALID_ARGUMENT;
    }
    std::vector<LightRec> recs(n);
    bool directional = false;
    for (uint32_t k = 0; k < n; ++k) {
        const std::string err = light_record(lights[k], k, recs[k]);
        if (!err.empty()) { ctx->error = err; return NORI_ERR_INVALID_ARGUMENT; }
        directional |= recs[k].type == kLightDirectional;
    }
    const int integ = ctx->host.integrator.type;
    if (integ != NORI_INTEGRATOR_PATH_EMS && integ != NORI_INTEGRATOR_PATH_MIS) {
        ctx->error = "set_lights: only path_ems and path_mis render delta lights (path_mats cannot reach one; the other integrators have no variant for them)";
        return NORI_ERR_UNSUPPORTED;
    }
    if (directional && ctx->dev.medium.on && !ctx->dev.gmed.rho) {      /* (a grid medium is bounded by its box: the transmittance from infinity is finite) */
        ctx->error = "set_lights: a directional light in a context with a medium: the medium fills all space, so the transmittance from infinity is 0; "
                     "unset the medium first (nori_hip_set_medium with NULL)";
        return NORI_ERR_UNSUPPORTED;
    }
    void *d = nullptr;
    HIP_TRY(ctx, hipMalloc(&d, n * sizeof(LightRec)));
    const hipError_t e = hipMemcpy(d, recs.data(), n * sizeof(LightRec), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void) hipFree(d); HIP_TRY(ctx, e); }
    lights_release(ctx);      /* (only now: a failed call leaves the stored lights as they were) */
    ctx->d_lights = d;
    ctx->host_lights.swap(recs);
    ctx->dev.lights = (const LightRec *) d;
    ctx->dev.n_lights = n;
    return NORI_OK;
}

int nori_hip_get_lights(const nori_hip_ctx *ctx, uint32_t cap, nori_light_desc *out, uint32_t *n) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return NORI_ERR_NOT_READY;      /* (the context is const: no message) */
    if (n) *n = (uint32_t) ctx->host_lights.size();
    if (out)
        for (uint32_t k = 0; k < cap && k < ctx->host_lights.size(); ++k) {
            static_assert(sizeof(nori_light_desc) == sizeof(LightRec), "the record is the description with its direction normalised");
            std::memcpy(&out[k], &ctx->host_lights[k], sizeof(LightRec));
        }
    return NORI_OK;
}

int nori_hip_light_incident(nori_hip_ctx *ctx, const uint32_t *light, const float *p, size_t n, float *dir, float *maxt, float *radiance) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene || ctx->dev.n_lights == 0u) { ctx->error = "light_incident: no lights set"; return NORI_ERR_NOT_READY; }
    if (n == 0) return NORI_OK;
    if (!light || !p || !dir || !maxt || !radiance) { ctx->error = "light_incident: null array"; return NORI_ERR_INVALID_ARGUMENT; }
    for (size_t k = 0; k < n; ++k)
        if (light[k] >= ctx->dev.n_lights) {
            ctx->error = "light_incident: light index " + std::to_string(light[k]) + " of " + std::to_string(ctx->dev.n_lights) + " lights";
            return NORI_ERR_INVALID_ARGUMENT;
        }
    DeviceGuard g(ctx->device);
    SCRATCH_IN(ctx, dl, light, n * sizeof(uint32_t));
    SCRATCH_IN(ctx, dp, p, n * 3 * sizeof(float));
    SCRATCH_OUT(ctx, dd, n * 3 * sizeof(float));
    SCRATCH_OUT(ctx, dm, n * sizeof(float));
    SCRATCH_OUT(ctx, dr, n * 3 * sizeof(float));
    hipLaunchKernelGGL(light_incident_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, ctx->dev.lights, (const uint32_t *) dl.p, (const float *) dp.p, n,
                       (float *) dd.p, (float *) dm.p, (float *) dr.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpy(dir, dd.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(maxt, dm.p, n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(radiance, dr.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return NORI_OK;
}

} // extern "C"
