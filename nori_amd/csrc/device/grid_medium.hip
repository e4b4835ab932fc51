/*
 * grid_medium.hip -- the entry points that set the context's grid medium, and the operator twins of its walk (include/nori_hip.h,
 * "Grid medium"; grid_medium.h holds the per-lane code the path kernels share).
 *
 * The voxels are a plain linear float32 array in device memory, x fastest; the record (GridMediumRec, rt_types.h) lies in DevScene by
 * value.  Albedo and phase function go through the homogeneous medium's record (DevScene::medium, on = 1, sigma_t = sigma_scale), so
 * everything past the free flight and the transmittance is kMedium's code.  The twins run grid_walk, one lane per query, no LDS:
 *   grid_medium_kernel    what 0: the free flight (no event: +inf);  1: the transmittance;  2: the optical depth and the voxels visited
 */
#include "ctx.h"
#include "grid_medium.h"
#include <cmath>
#include <cstring>

namespace {

using namespace nrt;

__global__ __launch_bounds__(256) void grid_medium_kernel(GridMediumRec g, int what, const float *o, const float *d, const float *tmax, const float *xi, size_t n,
                                                          float *out, int32_t *steps) {
    const size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const f3 ro = mk3(o[3 * k], o[3 * k + 1], o[3 * k + 2]), rd = mk3(d[3 * k], d[3 * k + 1], d[3 * k + 2]);
    if (what == 0) {
        float s;
        const bool ev = grid_distance(g, ro, rd, tmax[k], xi[k], s);
        out[k] = ev ? s : kInf;
    } else if (what == 1) {
        out[k] = grid_tr(g, ro, rd, tmax[k]);
    } else {
        const GridWalk w = grid_walk(g, ro, rd, tmax[k], kInf);
        out[k] = w.tau;
        steps[k] = w.steps;
    }
}

int grid_ready(nori_hip_ctx *ctx, const char *who) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene || !ctx->dev.gmed.rho) { ctx->error = std::string(who) + ": no grid medium set"; return NORI_ERR_NOT_READY; }
    return NORI_OK;
}

/* one launch of the twin kernel over n queries; xi and steps may be null (what says which are read) */
int grid_query(nori_hip_ctx *ctx, const char *who, int what, const float *o, const float *d, const float *tmax, const float *xi, size_t n, float *out, int32_t *steps) {
    const int ready = grid_ready(ctx, who);
    if (ready != NORI_OK) return ready;
    if (n == 0) return NORI_OK;
    if (!o || !d || !tmax || !out || (what == 0 && !xi) || (what == 2 && !steps)) { ctx->error = std::string(who) + ": null array"; return NORI_ERR_INVALID_ARGUMENT; }
    DeviceGuard g(ctx->device);
    SCRATCH_IN(ctx, d_o, o, n * 3 * sizeof(float));
    SCRATCH_IN(ctx, d_d, d, n * 3 * sizeof(float));
    SCRATCH_IN(ctx, d_t, tmax, n * sizeof(float));
    SCRATCH_IN(ctx, d_x, what == 0 ? xi : tmax, n * sizeof(float));
    SCRATCH_OUT(ctx, d_out, n * sizeof(float));
    SCRATCH_OUT(ctx, d_steps, n * sizeof(int32_t));
    hipLaunchKernelGGL(grid_medium_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, ctx->dev.gmed, what, (const float *) d_o.p, (const float *) d_d.p,
                       (const float *) d_t.p, (const float *) d_x.p, n, (float *) d_out.p, (int32_t *) d_steps.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpy(out, d_out.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (what == 2) HIP_TRY(ctx, hipMemcpy(steps, d_steps.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return NORI_OK;
}

} // namespace

void grid_medium_release(nori_hip_ctx *ctx) {
    if (!ctx->d_grid_rho) return;      /* (no grid: DevScene::medium is the homogeneous medium's, or off) */
    (void) hipFree(ctx->d_grid_rho);
    ctx->d_grid_rho = nullptr;
    ctx->grid_desc = nori_grid_medium_desc();
    ctx->dev.gmed = GridMediumRec();
    ctx->dev.medium = MediumRec();
}

extern "C" {

int nori_hip_set_grid_medium(nori_hip_ctx *ctx, const nori_grid_medium_desc *m) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) { ctx->error = "set_grid_medium: no scene uploaded"; return NORI_ERR_NOT_READY; }
    DeviceGuard g(ctx->device);
    if (!m) {      /* unsets a grid medium; a homogeneous medium is nori_hip_set_medium's */
        grid_medium_release(ctx);
        return NORI_OK;
    }
    if (!m->rho) { ctx->error = "set_grid_medium: rho is null"; return NORI_ERR_INVALID_ARGUMENT; }
    const int32_t dims[3] = {m->nx, m->ny, m->nz};
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 1 || dims[a] > 256) {
            ctx->error = "set_grid_medium: nx, ny and nz must each lie in 1 .. 256 (got " + std::to_string(m->nx) + " x " + std::to_string(m->ny) + " x " + std::to_string(m->nz) + ")";
            return NORI_ERR_INVALID_ARGUMENT;
        }
        if (!(std::isfinite(m->bmin[a]) && std::isfinite(m->bmax[a]) && m->bmin[a] < m->bmax[a] && std::isfinite(m->bmax[a] - m->bmin[a]))) {
            ctx->error = "set_grid_medium: the box needs finite bmin < bmax on every axis (axis " + std::to_string(a) + ": " + std::to_string(m->bmin[a]) + ", " + std::to_string(m->bmax[a]) + ")";
            return NORI_ERR_INVALID_ARGUMENT;
        }
    }
    if (!std::isfinite(m->sigma_scale) || !(m->sigma_scale >= 0.0f)) {
        ctx->error = "set_grid_medium: sigma_scale must be finite and not negative (got " + std::to_string(m->sigma_scale) + ")";
        return NORI_ERR_INVALID_ARGUMENT;
    }
    for (int c = 0; c < 3; ++c)
        if (!(std::isfinite(m->albedo[c]) && m->albedo[c] >= 0.0f && m->albedo[c] <= 1.0f)) {
            ctx->error = "set_grid_medium: every albedo component must be finite and lie in [0, 1] (got " + std::to_string(m->albedo[c]) + ")";
            return NORI_ERR_INVALID_ARGUMENT;
        }
    if (!(std::fabs(m->g) <= 0.99f)) {
        ctx->error = "set_grid_medium: the Henyey-Greenstein asymmetry g must lie in [-0.99, 0.99] (got " + std::to_string(m->g) + ")";
        return NORI_ERR_INVALID_ARGUMENT;
    }
    const size_t n = (size_t) m->nx * (size_t) m->ny * (size_t) m->nz;
    for (size_t k = 0; k < n; ++k) {      /* every voxel: the homogeneous medium's bounds, or vacuum */
        const float rho = m->rho[k];
        const float sigma = m->sigma_scale * rho;
        if (!(std::isfinite(rho) && rho >= 0.0f && (sigma == 0.0f || (sigma >= 1e-4f && sigma <= 1e4f)))) {
            const size_t x = k % (size_t) m->nx, y = (k / (size_t) m->nx) % (size_t) m->ny, z = k / ((size_t) m->nx * (size_t) m->ny);
            ctx->error = "set_grid_medium: voxel " + std::to_string(k) + " (x " + std::to_string(x) + ", y " + std::to_string(y) + ", z " + std::to_string(z) +
                         "): rho must be finite and not negative, and sigma_scale * rho 0 or in [1e-4, 1e4] (rho " + std::to_string(rho) + ", sigma " + std::to_string(sigma) + ")";
            return NORI_ERR_INVALID_ARGUMENT;
        }
    }
    const int integ = ctx->host.integrator.type;
    if (integ != NORI_INTEGRATOR_PATH_MATS && integ != NORI_INTEGRATOR_PATH_EMS && integ != NORI_INTEGRATOR_PATH_MIS) {
        ctx->error = "set_grid_medium: only path_mats, path_ems and path_mis render a medium (the other integrators have no variant for it)";
        return NORI_ERR_UNSUPPORTED;
    }
    if (ctx->dev.env) {
        ctx->error = "set_grid_medium: the context has an environment map, and no kernel set combines a grid medium with an environment map yet; "
                     "unset the environment first (nori_hip_set_environment with NULL)";
        return NORI_ERR_UNSUPPORTED;
    }
    void *d = nullptr;
    HIP_TRY(ctx, hipMalloc(&d, n * sizeof(float)));
    const hipError_t e = hipMemcpy(d, m->rho, n * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void) hipFree(d); HIP_TRY(ctx, e); }
    grid_medium_release(ctx);      /* (only now: a failed call leaves the context's medium as it was) */
    GridMediumRec r;
    r.rho = (const float *) d;
    r.sigma_scale = m->sigma_scale;
    for (int a = 0; a < 3; ++a) {
        const float ext = m->bmax[a] - m->bmin[a];
        r.n[a] = dims[a]; r.bmin[a] = m->bmin[a]; r.bmax[a] = m->bmax[a];
        r.cell[a] = ext / (float) dims[a];
        r.inv_cell[a] = (float) dims[a] / ext;
    }
    ctx->d_grid_rho = d;
    ctx->grid_desc = *m;
    ctx->grid_desc.rho = nullptr;
    ctx->dev.gmed = r;
    ctx->dev.medium = medium_record(m->sigma_scale, m->albedo, m->g);      /* the albedo and the phase function; it replaces a homogeneous medium */
    ctx->grid_desc.g = ctx->dev.medium.g;
    return NORI_OK;
}

int nori_hip_get_grid_medium(const nori_hip_ctx *ctx, nori_grid_medium_desc *m) {
    if (!ctx) return NORI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return NORI_ERR_NOT_READY;      /* (the context is const: no message) */
    if (m) *m = ctx->grid_desc;      /* rho null: the voxels are not read back */
    return ctx->dev.gmed.rho ? 1 : 0;
}

int nori_hip_grid_medium_distance(nori_hip_ctx *ctx, const float *o, const float *d, const float *tmax, const float *xi, size_t n, float *s) {
    return grid_query(ctx, "grid_medium_distance", 0, o, d, tmax, xi, n, s, nullptr);
}

int nori_hip_grid_medium_transmittance(nori_hip_ctx *ctx, const float *o, const float *d, const float *dist, size_t n, float *tr) {
    return grid_query(ctx, "grid_medium_transmittance", 1, o, d, dist, nullptr, n, tr, nullptr);
}

int nori_hip_grid_medium_optical_depth(nori_hip_ctx *ctx, const float *o, const float *d, const float *tmax, size_t n, float *tau, int32_t *steps) {
    return grid_query(ctx, "grid_medium_optical_depth", 2, o, d, tmax, nullptr, n, tau, steps);
}

} // extern "C"
