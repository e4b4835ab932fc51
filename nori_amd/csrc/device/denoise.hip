/* denoise.hip -- the guide records and the NL-means filter of nori_hip_denoise (see denoise.h). */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "denoise.h"
#include "denoise_filter.h"

using namespace nrt;

namespace {

/* step A (include/nori_hip.h): one thread per pixel of the frame without its border */
__global__ __launch_bounds__(kDnBlock) void denoise_guides_kernel(int width, int height, int border, const float *__restrict__ rgbw, const float *__restrict__ m2,
                                                                  const float *__restrict__ albedo, const float *__restrict__ normal,
                                                                  const float *__restrict__ depth, float4 *__restrict__ guides) {
    const size_t i = (size_t) blockIdx.x * kDnBlock + (size_t) threadIdx.x, n = (size_t) width * (size_t) height;
    if (i >= n) return;
    const int y = (int) (i / (size_t) width), x = (int) (i - (size_t) y * (size_t) width);
    const size_t at = ((size_t) (y + border) * (size_t) (width + 2 * border) + (size_t) (x + border)) * 4;
    const float4 S = *reinterpret_cast<const float4 *>(rgbw + at), M = *reinterpret_cast<const float4 *>(m2 + at);
    float mu[3], var[3];
    const bool valid = denoise_pixel_moments(f4{S.x, S.y, S.z, S.w}, f4{M.x, M.y, M.z, M.w}, mu, var);
    float a[3] = {0.0f, 0.0f, 0.0f}, nn[3] = {0.0f, 0.0f, 0.0f}, z = 0.0f, cov = 0.0f;
    if (albedo) {
        const float4 A = *reinterpret_cast<const float4 *>(albedo + at);
        a[0] = denoise_quot(A.x, A.w); a[1] = denoise_quot(A.y, A.w); a[2] = denoise_quot(A.z, A.w);
    }
    if (normal) {
        const float4 N = *reinterpret_cast<const float4 *>(normal + at);
        if (N.w > 0.0f) { nn[0] = 2.0f * (N.x / N.w) - 1.0f; nn[1] = 2.0f * (N.y / N.w) - 1.0f; nn[2] = 2.0f * (N.z / N.w) - 1.0f; }
    }
    if (depth) {
        const float4 D = *reinterpret_cast<const float4 *>(depth + at);
        cov = denoise_quot(D.z, D.w); z = denoise_quot(D.x, D.z);
    }
    float4 *g = guides + i * 4;
    g[0] = make_float4(mu[0], mu[1], mu[2], var[0]);
    g[1] = make_float4(var[1], var[2], a[0], a[1]);
    g[2] = make_float4(a[2], nn[0], nn[1], nn[2]);
    g[3] = make_float4(z, cov, valid ? 1.0f : 0.0f, 0.0f);
}

/* step B (include/nori_hip.h): the body is denoise_filter.h's, without the variance accumulators */
template <int F, int RMAX>
__global__ __launch_bounds__(kDnBlock, dn_min_waves(RMAX)) void denoise_filter_kernel(DenoiseLaunch dl, const float4 *__restrict__ guides, float *__restrict__ rgb_out,
                                                                               float *__restrict__ wsum_out) {
    denoise_filter_body<F, RMAX, false>(dl, guides, (int) blockIdx.x, rgb_out, nullptr, wsum_out);
}

template <int F, int RMAX>
hipError_t launch_filter(const DenoiseLaunch &dl, const float *d_guides, float *d_rgb_out, float *d_wsum, hipStream_t s) {
    const unsigned n_tiles = (unsigned) ((dl.width + kTile - 1) / kTile) * (unsigned) ((dl.height + kTile - 1) / kTile);
    hipLaunchKernelGGL((denoise_filter_kernel<F, RMAX>), dim3(n_tiles), dim3(kDnBlock), 0, s, dl, reinterpret_cast<const float4 *>(d_guides), d_rgb_out, d_wsum);
    return hipGetLastError();
}

template <int F>
hipError_t launch_filter_patch(const DenoiseLaunch &dl, const float *d_guides, float *d_rgb_out, float *d_wsum, hipStream_t s) {
    return dl.radius <= 5 ? launch_filter<F, 5>(dl, d_guides, d_rgb_out, d_wsum, s) : launch_filter<F, 8>(dl, d_guides, d_rgb_out, d_wsum, s);
}

} // namespace

namespace nrt {

std::string denoise_store_guides(DenoiseStore &ds, void *stream, size_t n_pixels, float **out) {
    const size_t need = std::max<size_t>(n_pixels, 1) * kGuideFloats;
    DenoiseStore::Slot *slot = nullptr;
    for (DenoiseStore::Slot &s : ds.slots)
        if (s.stream == stream) slot = &s;
    if (!slot) { ds.slots.push_back(DenoiseStore::Slot{stream, nullptr, 0}); slot = &ds.slots.back(); }
    if (slot->floats < need || !slot->guides) {
        /* (hipFree waits for the device: no kernel still reads the buffer that goes) */
        if (slot->guides) (void) hipFree(slot->guides);
        slot->guides = nullptr; slot->floats = 0;
        const hipError_t e = hipMalloc((void **) &slot->guides, need * sizeof(float));
        if (e != hipSuccess) return std::string("denoise: guide records: ") + hipGetErrorString(e);
        slot->floats = need;
    }
    *out = slot->guides;
    return std::string();
}

void denoise_store_release(DenoiseStore &ds) {
    for (DenoiseStore::Slot &s : ds.slots)
        if (s.guides) (void) hipFree(s.guides);
    ds.slots.clear();
}

uint32_t denoise_filter_lds_bytes(int radius, int patch) {
    const int side = kTile + 2 * ((radius <= 5 ? 5 : 8) + patch);
    return (uint32_t) (7 * side * side * sizeof(float) + 2 * kDeltaStride * (kTile + 2 * patch) * sizeof(float2));
}

hipError_t denoise_guides_launch(int width, int height, int border, const float *d_rgbw, const float *d_m2, const float *d_albedo,
                                 const float *d_normal, const float *d_depth, float *d_guides, void *stream) {
    const size_t n = (size_t) width * (size_t) height;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_guides_kernel, dim3((unsigned) ((n + kDnBlock - 1) / kDnBlock)), dim3(kDnBlock), 0, (hipStream_t) stream, width, height, border,
                       d_rgbw, d_m2, d_albedo, d_normal, d_depth, reinterpret_cast<float4 *>(d_guides));
    return hipGetLastError();
}

hipError_t denoise_filter_launch(const DenoiseLaunch &dl, const float *d_guides, float *d_rgb_out, float *d_wsum, void *stream) {
    if (dl.width <= 0 || dl.height <= 0) return hipSuccess;
    if (dl.radius < 1 || dl.radius > kDenoiseMaxRadius || dl.patch < 0 || dl.patch > kDenoiseMaxPatch) return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t) stream;
    switch (dl.patch) {
    case 0: return launch_filter_patch<0>(dl, d_guides, d_rgb_out, d_wsum, s);
    case 1: return launch_filter_patch<1>(dl, d_guides, d_rgb_out, d_wsum, s);
    default: return launch_filter_patch<2>(dl, d_guides, d_rgb_out, d_wsum, s);
    }
}

} // namespace nrt
