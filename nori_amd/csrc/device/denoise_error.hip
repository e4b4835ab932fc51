/* denoise_error.hip -- the filter with its output variance, the error of a denoised frame as map, summary and tile means (see denoise_error.h). */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "denoise_error.h"
#include "denoise_filter.h"

using namespace nrt;

namespace {

constexpr int kB = 256;

/* step B with the output variance (include/nori_hip.h: nori_hip_denoise_var): the body is denoise_filter.h's with the accumulators on */
template <int F, int RMAX>
__global__ __launch_bounds__(kDnBlock, dn_min_waves(RMAX)) void denoise_filter_var_kernel(DenoiseLaunch dl, const float4 *__restrict__ guides, const uint32_t *__restrict__ list,
                                                                                   float *__restrict__ rgb_out, float *__restrict__ var_out, float *__restrict__ wsum_out) {
    const int tile = list ? (int) list[blockIdx.x] : (int) blockIdx.x;
    denoise_filter_body<F, RMAX, true>(dl, guides, tile, rgb_out, var_out, wsum_out);
}

template <int F, int RMAX>
hipError_t launch_var(const DenoiseLaunch &dl, const float *d_guides, const uint32_t *d_list, uint32_t n_wg, float *d_rgb_out, float *d_var_out, float *d_wsum, hipStream_t s) {
    hipLaunchKernelGGL((denoise_filter_var_kernel<F, RMAX>), dim3(n_wg), dim3(kDnBlock), 0, s, dl, reinterpret_cast<const float4 *>(d_guides), d_list, d_rgb_out, d_var_out, d_wsum);
    return hipGetLastError();
}

template <int F>
hipError_t launch_var_patch(const DenoiseLaunch &dl, const float *d_guides, const uint32_t *d_list, uint32_t n_wg, float *d_rgb_out, float *d_var_out, float *d_wsum, hipStream_t s) {
    return dl.radius <= 5 ? launch_var<F, 5>(dl, d_guides, d_list, n_wg, d_rgb_out, d_var_out, d_wsum, s) : launch_var<F, 8>(dl, d_guides, d_list, n_wg, d_rgb_out, d_var_out, d_wsum, s);
}

/* per-workgroup (and, slot 0, whole-frame) sums of the error map: the layout of film.hip's */
struct ErrorPartial { double sum; float max; uint32_t pad; unsigned long long n_empty, n_above; };

/* adds the 256 partials of a workgroup in the fixed tree of film.hip's film_error_tree: lane t takes lane t + off for off = 128, 64, ..., 1 */
__device__ __forceinline__ void error_tree(double *s_sum, float *s_max, unsigned long long *s_empty64, unsigned long long *s_above64, int tid,
                                           double sum, float mx, unsigned long long n_empty, unsigned long long n_above, ErrorPartial *out) {
    s_sum[tid] = sum; s_max[tid] = mx; s_empty64[tid] = n_empty; s_above64[tid] = n_above;
    __syncthreads();
    for (int off = kB / 2; off > 0; off >>= 1) {
        if (tid < off) {
            s_sum[tid] += s_sum[tid + off]; s_max[tid] = fmaxf(s_max[tid], s_max[tid + off]);
            s_empty64[tid] += s_empty64[tid + off]; s_above64[tid] += s_above64[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) { ErrorPartial p; p.sum = s_sum[0]; p.max = s_max[0]; p.pad = 0u; p.n_empty = s_empty64[0]; p.n_above = s_above64[0]; *out = p; }
}

/* the error of frame pixel i of a denoised frame (no border: the filter's outputs have none) */
__device__ __forceinline__ float pixel_error_at(const float *__restrict__ rgb, const float *__restrict__ var, const float *__restrict__ wsum, size_t i, bool &empty) {
    const float c[3] = {rgb[i * 3 + 0], rgb[i * 3 + 1], rgb[i * 3 + 2]}, v[3] = {var[i * 3 + 0], var[i * 3 + 1], var[i * 3 + 2]};
    return denoised_pixel_error(c, v, wsum[i], empty);
}

/* one thread per pixel of the frame, and the workgroup's partial sums (film_error_map_kernel for a denoised frame) */
__global__ __launch_bounds__(kB) void denoise_error_map_kernel(int width, int height, const float *__restrict__ rgb, const float *__restrict__ var,
                                                               const float *__restrict__ wsum, float *__restrict__ err_out, float threshold, ErrorPartial *partials) {
    __shared__ double s_sum[kB];
    __shared__ float s_max[kB];
    __shared__ unsigned long long s_empty[kB], s_above[kB];
    const int tid = threadIdx.x;
    const size_t i = (size_t) blockIdx.x * kB + (size_t) tid, n = (size_t) width * (size_t) height;
    float err = 0.0f;
    bool empty = false;
    if (i < n) {
        err = pixel_error_at(rgb, var, wsum, i, empty);
        if (err_out) err_out[i] = err;
    }
    if (!partials) return;      /* the map alone: nothing shared is written (the same for every thread of the launch) */
    error_tree(s_sum, s_max, s_empty, s_above, tid, (double) err, err, empty ? 1ull : 0ull, i < n && err > threshold ? 1ull : 0ull, partials + blockIdx.x);
}

/* one workgroup: lane t adds the partials t, t + 256, ... in ascending order, then the tree */
__global__ __launch_bounds__(kB) void denoise_error_reduce_kernel(const ErrorPartial *partials, uint32_t n, ErrorPartial *total) {
    __shared__ double s_sum[kB];
    __shared__ float s_max[kB];
    __shared__ unsigned long long s_empty[kB], s_above[kB];
    const int tid = threadIdx.x;
    double sum = 0.0; float mx = 0.0f; unsigned long long n_empty = 0, n_above = 0;
    for (uint32_t i = (uint32_t) tid; i < n; i += kB) {
        const ErrorPartial p = partials[i];
        sum += p.sum; mx = fmaxf(mx, p.max); n_empty += p.n_empty; n_above += p.n_above;
    }
    error_tree(s_sum, s_max, s_empty, s_above, tid, sum, mx, n_empty, n_above, total);
}

/* one workgroup per tile of the frame (include/nori_hip.h: nori_hip_denoised_tile_errors; film_tile_errors_kernel's tree) */
__global__ __launch_bounds__(kB) void denoise_tile_errors_kernel(int width, int height, uint32_t tiles_x, const float *__restrict__ rgb, const float *__restrict__ var,
                                                                 const float *__restrict__ wsum, float *__restrict__ tile_err) {
    __shared__ double s_sum[kB];
    const int tid = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const int x0 = (int) (tile % tiles_x) * kTile, y0 = (int) (tile / tiles_x) * kTile;
    const int x = x0 + (tid & (kTile - 1)), y = y0 + (tid >> 4);
    float err = 0.0f;
    if (x < width && y < height) {
        bool empty;
        err = pixel_error_at(rgb, var, wsum, (size_t) y * (size_t) width + (size_t) x, empty);
    }
    s_sum[tid] = (double) err;
    __syncthreads();
    for (int off = kB / 2; off > 0; off >>= 1) {
        if (tid < off) s_sum[tid] += s_sum[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        const int nx = min(kTile, width - x0), ny = min(kTile, height - y0);
        tile_err[tile] = (float) (s_sum[0] / (double) (nx * ny));
    }
}

} // namespace

namespace nrt {

#define DNE_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(e__); } while (0)

void denoise_error_release(DenoiseErrorStore &s) {
    if (s.partials) (void) hipFree(s.partials);
    s = DenoiseErrorStore();
}

hipError_t denoise_filter_var_launch(const DenoiseLaunch &dl, const float *d_guides, const uint32_t *d_list, uint32_t n_list,
                                     float *d_rgb_out, float *d_var_out, float *d_wsum, void *stream) {
    if (dl.width <= 0 || dl.height <= 0) return hipSuccess;
    if (dl.radius < 1 || dl.radius > kDenoiseMaxRadius || dl.patch < 0 || dl.patch > kDenoiseMaxPatch) return hipErrorInvalidValue;
    const uint32_t n_frame = (uint32_t) ((dl.width + kTile - 1) / kTile) * (uint32_t) ((dl.height + kTile - 1) / kTile);
    if (d_list && n_list > n_frame) return hipErrorInvalidValue;      /* (a list names a tile once) */
    const uint32_t n_wg = d_list ? n_list : n_frame;
    if (n_wg == 0) return hipSuccess;
    hipStream_t s = (hipStream_t) stream;
    switch (dl.patch) {
    case 0: return launch_var_patch<0>(dl, d_guides, d_list, n_wg, d_rgb_out, d_var_out, d_wsum, s);
    case 1: return launch_var_patch<1>(dl, d_guides, d_list, n_wg, d_rgb_out, d_var_out, d_wsum, s);
    default: return launch_var_patch<2>(dl, d_guides, d_list, n_wg, d_rgb_out, d_var_out, d_wsum, s);
    }
}

std::string denoised_error_map(DenoiseErrorStore &store, int w, int h, const float *d_rgb, const float *d_var, const float *d_wsum,
                               float *d_err, float threshold, FilmErrorSummary *out, void *stream) {
    const size_t n_pixels = (size_t) std::max(w, 0) * (size_t) std::max(h, 0);
    if (n_pixels == 0 || n_pixels > ((size_t) 1 << 31)) return "denoised_error_map: frame of no pixels or more than 2^31";
    const uint32_t n_blocks = (uint32_t) ((n_pixels + kB - 1) / kB);
    hipStream_t s = (hipStream_t) stream;
    if (!out) {      /* the map alone touches nothing of the context's: such calls may run on several streams at once */
        hipLaunchKernelGGL(denoise_error_map_kernel, dim3(n_blocks), dim3(kB), 0, s, w, h, d_rgb, d_var, d_wsum, d_err, threshold, (ErrorPartial *) nullptr);
        DNE_TRY(hipGetLastError());
        return std::string();
    }
    /* the summary goes through the context's one array of partial sums; the call ends with the stream synchronised (film_error_map) */
    if (store.blocks < (size_t) n_blocks + 1) {
        if (store.partials) (void) hipFree(store.partials);
        store.partials = nullptr; store.blocks = 0;
        DNE_TRY(hipMalloc((void **) &store.partials, ((size_t) n_blocks + 1) * sizeof(ErrorPartial)));
        store.blocks = (size_t) n_blocks + 1;
    }
    ErrorPartial *part = (ErrorPartial *) store.partials;
    hipLaunchKernelGGL(denoise_error_map_kernel, dim3(n_blocks), dim3(kB), 0, s, w, h, d_rgb, d_var, d_wsum, d_err, threshold, part + 1);
    DNE_TRY(hipGetLastError());
    hipLaunchKernelGGL(denoise_error_reduce_kernel, dim3(1), dim3(kB), 0, s, (const ErrorPartial *) (part + 1), n_blocks, part);
    DNE_TRY(hipGetLastError());
    ErrorPartial total;
    DNE_TRY(hipMemcpyAsync(&total, part, sizeof(total), hipMemcpyDeviceToHost, s));
    DNE_TRY(hipStreamSynchronize(s));
    out->sum_err = total.sum; out->max_err = total.max; out->n_pixels = n_pixels; out->n_empty = total.n_empty; out->n_above = total.n_above;
    return std::string();
}

std::string denoised_tile_errors(int w, int h, const float *d_rgb, const float *d_var, const float *d_wsum, float *d_tile_err, void *stream) {
    if (w <= 0 || h <= 0) return "denoised_tile_errors: frame of no pixels";
    const uint32_t tiles_x = (uint32_t) ((w + kTile - 1) / kTile), tiles_y = (uint32_t) ((h + kTile - 1) / kTile);
    hipLaunchKernelGGL(denoise_tile_errors_kernel, dim3(tiles_x * tiles_y), dim3(kB), 0, (hipStream_t) stream, w, h, tiles_x, d_rgb, d_var, d_wsum, d_tile_err);
    DNE_TRY(hipGetLastError());
    return std::string();
}

} // namespace nrt
