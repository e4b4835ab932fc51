/* film_tiles.hip -- the film for renders of a tile list, per-tile errors, selection (see film_tiles.h). */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "film_tiles.h"

using namespace nrt;

namespace {

constexpr int kB = 256;

/* film_resolve_kernel (film.hip) with the ordinal of a covering tile read from the inverse table: the same loops in the same
   order, so every frame pixel adds the same accumulators in the same sequence when the list equals a progression */
__global__ void film_resolve_tiles_kernel(int width, int height, int border, int tile_w, uint32_t tiles_x, uint32_t tiles_y,
                                          const uint32_t *__restrict__ inverse, uint32_t n_parts, const float *tile_acc, float *rgbw) {
    const int cols = width + 2 * border, rows = height + 2 * border;
    const int gx = blockIdx.x * blockDim.x + threadIdx.x, gy = blockIdx.y;
    if (gx >= cols || gy >= rows) return;
    float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int tx1 = min(gx / kTile, (int) tiles_x - 1), ty1 = min(gy / kTile, (int) tiles_y - 1);
    const int tx0 = max(0, (gx - tile_w + kTile) / kTile), ty0 = max(0, (gy - tile_w + kTile) / kTile);
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const int lx = gx - tx * kTile, ly = gy - ty * kTile;
            if (lx < 0 || ly < 0 || lx >= tile_w || ly >= tile_w) continue;
            const uint32_t ord = inverse[(uint32_t) ty * tiles_x + (uint32_t) tx];
            if (ord == kTileNotListed) continue;
            for (uint32_t part = 0; part < n_parts; ++part) {      /* fixed order: deterministic */
                const float4 v = *reinterpret_cast<const float4 *>(tile_acc + ((((size_t) ord * n_parts + part) * tile_w + (size_t) ly) * tile_w + lx) * 4);
                sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
            }
        }
    float4 *dst = reinterpret_cast<float4 *>(rgbw) + (size_t) gy * cols + gx;
    float4 cur = *dst;
    cur.x += sum.x; cur.y += sum.y; cur.z += sum.z; cur.w += sum.w;
    *dst = cur;
}

/* one workgroup per tile of the frame (include/nori_hip.h: nori_hip_tile_errors states the operation) */
__global__ __launch_bounds__(kB) void film_tile_errors_kernel(int width, int height, int border, uint32_t tiles_x, const float *__restrict__ rgbw,
                                                              const float *__restrict__ m2, float *__restrict__ tile_err) {
    __shared__ double s_sum[kB];
    const int tid = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const int x0 = (int) (tile % tiles_x) * kTile, y0 = (int) (tile / tiles_x) * kTile;
    const int x = x0 + (tid & (kTile - 1)), y = y0 + (tid >> 4);
    float err = 0.0f;
    if (x < width && y < height) {
        const size_t at = ((size_t) (y + border) * (size_t) (width + 2 * border) + (size_t) (x + border)) * 4;
        const float4 S = *reinterpret_cast<const float4 *>(rgbw + at), M = *reinterpret_cast<const float4 *>(m2 + at);
        bool empty;
        err = film_pixel_error(f4{S.x, S.y, S.z, S.w}, f4{M.x, M.y, M.z, M.w}, empty);
    }
    s_sum[tid] = (double) err;
    __syncthreads();
    for (int off = kB / 2; off > 0; off >>= 1) {      /* the tree of film_error_tree */
        if (tid < off) s_sum[tid] += s_sum[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        const int nx = min(kTile, width - x0), ny = min(kTile, height - y0);
        tile_err[tile] = (float) (s_sum[0] / (double) (nx * ny));
    }
}

/* a tile stays while its error is not known to be at or below the target: a NaN stays */
__device__ __forceinline__ bool tile_stays(const uint32_t *__restrict__ list, uint32_t n, const float *__restrict__ err, float target, uint32_t i, uint32_t &tile) {
    tile = 0u;
    if (i >= n) return false;
    tile = list[i];
    return !(err[tile] <= target);
}

/* survivors among entries [256 b, 256 b + 256) of the list */
__global__ __launch_bounds__(kB) void film_tile_select_count_kernel(const uint32_t *__restrict__ list, uint32_t n, const float *__restrict__ err, float target,
                                                                    uint32_t *__restrict__ block_counts) {
    __shared__ uint32_t s_n[kB];
    const int tid = threadIdx.x;
    uint32_t tile;
    s_n[tid] = tile_stays(list, n, err, target, blockIdx.x * kB + (uint32_t) tid, tile) ? 1u : 0u;
    __syncthreads();
    for (int off = kB / 2; off > 0; off >>= 1) {
        if (tid < off) s_n[tid] += s_n[tid + off];
        __syncthreads();
    }
    if (tid == 0) block_counts[blockIdx.x] = s_n[0];
}

/* one workgroup: the counts become their exclusive prefix sums, *d_count their total.  Thread t owns a run of consecutive
   counts; the runs' sums are scanned in LDS. */
__global__ __launch_bounds__(kB) void film_tile_select_scan_kernel(uint32_t *block_counts, uint32_t n_blocks, uint32_t *d_count) {
    __shared__ uint32_t s_n[kB];
    const int tid = threadIdx.x;
    const uint32_t per = (n_blocks + kB - 1) / kB;
    const uint32_t lo = min((uint32_t) tid * per, n_blocks), hi = min(lo + per, n_blocks);
    uint32_t own = 0;
    for (uint32_t i = lo; i < hi; ++i) own += block_counts[i];
    s_n[tid] = own;
    __syncthreads();
    for (int off = 1; off < kB; off <<= 1) {      /* inclusive scan */
        const uint32_t add = tid >= off ? s_n[tid - off] : 0u;
        __syncthreads();
        s_n[tid] += add;
        __syncthreads();
    }
    uint32_t run = s_n[tid] - own;
    for (uint32_t i = lo; i < hi; ++i) { const uint32_t c = block_counts[i]; block_counts[i] = run; run += c; }
    if (tid == kB - 1) *d_count = s_n[kB - 1];
}

/* the survivors of entries [256 b, 256 b + 256) to out[block_offsets[b] + rank among them], and their ordinals to the inverse
   table (set to kTileNotListed beforehand) */
__global__ __launch_bounds__(kB) void film_tile_select_scatter_kernel(const uint32_t *__restrict__ list, uint32_t n, const float *__restrict__ err, float target,
                                                                      const uint32_t *__restrict__ block_offsets, uint32_t *__restrict__ out,
                                                                      uint32_t *__restrict__ inverse) {
    __shared__ uint32_t s_n[kB];
    const int tid = threadIdx.x;
    uint32_t tile;
    const bool stays = tile_stays(list, n, err, target, blockIdx.x * kB + (uint32_t) tid, tile);
    s_n[tid] = stays ? 1u : 0u;
    __syncthreads();
    for (int off = 1; off < kB; off <<= 1) {
        const uint32_t add = tid >= off ? s_n[tid - off] : 0u;
        __syncthreads();
        s_n[tid] += add;
        __syncthreads();
    }
    if (stays) {
        const uint32_t ord = block_offsets[blockIdx.x] + s_n[tid] - 1u;
        out[ord] = tile;
        inverse[tile] = ord;
    }
}

__global__ void film_tiles_add_spp_kernel(const uint32_t *__restrict__ list, uint32_t n, uint32_t spp, uint32_t *__restrict__ tile_spp) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tile_spp[list[i]] += spp;      /* (a list names a tile once) */
}

} // namespace

namespace nrt {

#define TILES_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(e__); } while (0)

void film_tiles_release(FilmTiles &t) {
    for (uint32_t *&p : t.list) if (p) (void) hipFree(p);
    if (t.inverse) (void) hipFree(t.inverse);
    if (t.d_count) (void) hipFree(t.d_count);
    if (t.block_counts) (void) hipFree(t.block_counts);
    if (t.tile_err) (void) hipFree(t.tile_err);
    if (t.tile_spp) (void) hipFree(t.tile_spp);
    t = FilmTiles();
}

std::string film_tiles_reserve(FilmTiles &t, size_t n_frame_tiles) {
    if (n_frame_tiles == 0 || n_frame_tiles >= (size_t) kTileNotListed) return "tiles: frame of no tiles or too many";
    if (t.capacity >= n_frame_tiles) return std::string();
    film_tiles_release(t);
    const size_t words = n_frame_tiles * sizeof(uint32_t);
    for (uint32_t *&p : t.list) TILES_TRY(hipMalloc((void **) &p, words));
    TILES_TRY(hipMalloc((void **) &t.inverse, words));
    TILES_TRY(hipMalloc((void **) &t.d_count, sizeof(uint32_t)));
    TILES_TRY(hipMalloc((void **) &t.block_counts, ((n_frame_tiles + kB - 1) / kB) * sizeof(uint32_t)));
    TILES_TRY(hipMalloc((void **) &t.tile_err, n_frame_tiles * sizeof(float)));
    TILES_TRY(hipMalloc((void **) &t.tile_spp, words));
    t.capacity = n_frame_tiles;
    return std::string();
}

std::string film_tiles_upload(FilmTiles &t, const uint32_t *tiles, uint32_t n, size_t n_frame_tiles, void *stream) {
    std::string err = film_tiles_reserve(t, n_frame_tiles);
    if (!err.empty()) return err;
    std::vector<uint32_t> inverse(n_frame_tiles, kTileNotListed);
    for (uint32_t i = 0; i < n; ++i) inverse[tiles[i]] = i;
    hipStream_t s = (hipStream_t) stream;
    if (n) TILES_TRY(hipMemcpyAsync(t.list[t.cur], tiles, (size_t) n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    TILES_TRY(hipMemcpyAsync(t.inverse, inverse.data(), n_frame_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    TILES_TRY(hipStreamSynchronize(s));
    t.n = n;
    return std::string();
}

void film_resolve_tiles(const DevScene &sc, const FilmStore &st, const FilmLaunch &fl, float *d_rgbw, void *stream) {
    const int border = sc.filter.border, cols = sc.camera.width + 2 * border, rows = sc.camera.height + 2 * border;
    hipLaunchKernelGGL(film_resolve_tiles_kernel, dim3((cols + 255) / 256, rows), dim3(256), 0, (hipStream_t) stream, sc.camera.width,
                       sc.camera.height, border, fl.tile_w, fl.tiles_x, fl.tiles_y, fl.tile_inverse, st.n_parts, (const float *) st.tile_acc, d_rgbw);
}

std::string film_tile_errors(const DevScene &sc, const float *d_rgbw, const float *d_m2, float *d_tile_err, void *stream) {
    const int w = sc.camera.width, h = sc.camera.height;
    if (w <= 0 || h <= 0) return "tile_errors: frame of no pixels";
    const uint32_t tiles_x = (uint32_t) ((w + kTile - 1) / kTile), tiles_y = (uint32_t) ((h + kTile - 1) / kTile);
    hipLaunchKernelGGL(film_tile_errors_kernel, dim3(tiles_x * tiles_y), dim3(kB), 0, (hipStream_t) stream, w, h, sc.filter.border, tiles_x, d_rgbw, d_m2, d_tile_err);
    TILES_TRY(hipGetLastError());
    return std::string();
}

std::string film_tiles_select(FilmTiles &t, const float *d_tile_err, float target, size_t n_frame_tiles, void *stream) {
    hipStream_t s = (hipStream_t) stream;
    if (t.capacity < n_frame_tiles || t.n > n_frame_tiles) return "select_tiles: no list for this frame";
    TILES_TRY(hipMemsetAsync(t.inverse, 0xff, n_frame_tiles * sizeof(uint32_t), s));      /* kTileNotListed */
    if (t.n == 0) { TILES_TRY(hipMemsetAsync(t.d_count, 0, sizeof(uint32_t), s)); return std::string(); }      /* (nothing to scan: the length on the device is 0 too) */
    const uint32_t n_blocks = (t.n + kB - 1) / kB;
    const uint32_t *in = t.list[t.cur];
    uint32_t *out = t.list[t.cur ^ 1];
    hipLaunchKernelGGL(film_tile_select_count_kernel, dim3(n_blocks), dim3(kB), 0, s, in, t.n, d_tile_err, target, t.block_counts);
    TILES_TRY(hipGetLastError());
    hipLaunchKernelGGL(film_tile_select_scan_kernel, dim3(1), dim3(kB), 0, s, t.block_counts, n_blocks, t.d_count);
    TILES_TRY(hipGetLastError());
    hipLaunchKernelGGL(film_tile_select_scatter_kernel, dim3(n_blocks), dim3(kB), 0, s, in, t.n, d_tile_err, target, (const uint32_t *) t.block_counts, out, t.inverse);
    TILES_TRY(hipGetLastError());
    uint32_t n_out = 0;
    TILES_TRY(hipMemcpyAsync(&n_out, t.d_count, sizeof(n_out), hipMemcpyDeviceToHost, s));
    TILES_TRY(hipStreamSynchronize(s));
    if (n_out > t.n) return "select_tiles: the selection grew the list";
    t.cur ^= 1; t.n = n_out;
    return std::string();
}

void film_tiles_add_spp(const FilmTiles &t, uint32_t *d_tile_spp, uint32_t spp, void *stream) {
    if (t.n == 0) return;
    hipLaunchKernelGGL(film_tiles_add_spp_kernel, dim3((t.n + kB - 1) / kB), dim3(kB), 0, (hipStream_t) stream, (const uint32_t *) t.list[t.cur], t.n, spp, d_tile_spp);
}

} // namespace nrt
