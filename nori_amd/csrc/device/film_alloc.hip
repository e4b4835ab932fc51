/* film_alloc.hip -- sample levels per tile from the tile errors: classification, stable grouping by pair, inverse table (see film_alloc.h). */
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "film_alloc.h"

using namespace nrt;

namespace {

constexpr int kB = 256;

/* one thread per tile of the frame: the rule of include/nori_hip.h (nori_hip_render_allocated) */
__global__ __launch_bounds__(kB) void film_alloc_classify_kernel(const float *__restrict__ err, float target, float headroom, AllocLevels lv, uint32_t n_tiles,
                                                                 uint32_t *__restrict__ level, uint32_t *__restrict__ done, uint32_t *__restrict__ bucket) {
    const uint32_t t = blockIdx.x * kB + threadIdx.x;
    if (t >= n_tiles) return;
    uint32_t b = kAllocStays;
    if (done[t] == 0u) {
        const uint32_t l = min(level[t], lv.J);
        bool stop;
        const uint32_t j = alloc_rule(err[t], target, headroom, lv, l, stop);
        if (stop) done[t] = 1u;
        else { level[t] = j; b = alloc_bucket(lv.J, l, j); }
    }
    bucket[t] = b;
}

/* The 28 counters of a block in ONE LDS scan.  A tile adds 1 to the 9-bit field of its bucket (a count reaches 256), seven fields to a
   64-bit word, four words for the 28 buckets; fields never carry into each other, so the inclusive scan of the four words over the
   256 lanes (Hillis-Steele, as film_tile_select_scatter_kernel's) is the inclusive scan of every bucket's flags at once.  After it
   field b of lane t is the number of tiles of bucket b among lanes 0 .. t: a tile's rank + 1, and in lane 255 the block's count. */
constexpr uint32_t kFieldBits = 9, kFieldsPerWord = 7, kWords = 4;
static_assert(kFieldsPerWord * kWords >= (uint32_t) kAllocMaxBuckets && kFieldBits * kFieldsPerWord <= 64 && (1u << kFieldBits) > (uint32_t) kB, "28 counters of up to 256");

__device__ __forceinline__ uint32_t scan_field(const uint64_t (*s_c)[kB], uint32_t lane, uint32_t b) {
    return (uint32_t) (s_c[b / kFieldsPerWord][lane] >> (kFieldBits * (b % kFieldsPerWord))) & ((1u << kFieldBits) - 1u);
}

__device__ __forceinline__ void block_bucket_scan(uint64_t (*s_c)[kB], uint32_t tid, uint32_t b) {
#pragma unroll
    for (uint32_t w = 0; w < kWords; ++w)
        s_c[w][tid] = (b != kAllocStays && b / kFieldsPerWord == w) ? (uint64_t) 1 << (kFieldBits * (b % kFieldsPerWord)) : (uint64_t) 0;
    __syncthreads();
    for (uint32_t off = 1; off < (uint32_t) kB; off <<= 1) {      /* inclusive scan of the four words */
        uint64_t add[kWords];
#pragma unroll
        for (uint32_t w = 0; w < kWords; ++w) add[w] = tid >= off ? s_c[w][tid - off] : (uint64_t) 0;
        __syncthreads();
#pragma unroll
        for (uint32_t w = 0; w < kWords; ++w) s_c[w][tid] += add[w];
        __syncthreads();
    }
}

/* tiles [256 blk, 256 blk + 256): the block's count of every bucket, bucket-major */
__global__ __launch_bounds__(kB) void film_alloc_count_kernel(const uint32_t *__restrict__ bucket, uint32_t n_tiles, uint32_t n_buckets, uint32_t n_blocks,
                                                              uint32_t *__restrict__ counts) {
    __shared__ uint64_t s_c[kWords][kB];
    const uint32_t tid = threadIdx.x, t = blockIdx.x * kB + tid;
    block_bucket_scan(s_c, tid, t < n_tiles ? bucket[t] : kAllocStays);
    if (tid < n_buckets) counts[(size_t) tid * n_blocks + blockIdx.x] = scan_field(s_c, kB - 1, tid);
}

/* one workgroup: the n counts become their exclusive prefix sums (film_tile_select_scan_kernel's form: lane t owns a run of
   consecutive counts, the runs' sums are scanned in LDS); the offset at the head of bucket b goes to bucket_begin[b], the total to
   bucket_begin[n_buckets .. kAllocMaxBuckets] */
__global__ __launch_bounds__(kB) void film_alloc_scan_kernel(uint32_t *counts, uint32_t n, uint32_t n_blocks, uint32_t n_buckets, uint32_t *__restrict__ bucket_begin) {
    __shared__ uint32_t s_n[kB];
    const int tid = threadIdx.x;
    const uint32_t per = (n + kB - 1) / kB;
    const uint32_t lo = min((uint32_t) tid * per, n), hi = min(lo + per, n);
    uint32_t own = 0;
    for (uint32_t i = lo; i < hi; ++i) own += counts[i];
    s_n[tid] = own;
    __syncthreads();
    for (int off = 1; off < kB; off <<= 1) {      /* inclusive scan */
        const uint32_t add = tid >= off ? s_n[tid - off] : 0u;
        __syncthreads();
        s_n[tid] += add;
        __syncthreads();
    }
    uint32_t run = s_n[tid] - own;
    uint32_t head = lo % n_blocks, b = lo / n_blocks;      /* (i = b n_blocks + head, kept without a division per count) */
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = counts[i];
        counts[i] = run;
        if (head == 0u) bucket_begin[b] = run;
        run += c;
        if (++head == n_blocks) { head = 0u; ++b; }
    }
    const uint32_t total = s_n[kB - 1];
    if ((uint32_t) tid >= n_buckets && tid <= kAllocMaxBuckets) bucket_begin[tid] = total;
}

/* a moving tile of [256 blk, 256 blk + 256) to list[offsets[b n_blocks + blk] + rank], rank = the block's tiles of bucket b before it: the same scan */
__global__ __launch_bounds__(kB) void film_alloc_scatter_kernel(const uint32_t *__restrict__ bucket, uint32_t n_tiles, uint32_t n_blocks,
                                                                const uint32_t *__restrict__ offsets, uint32_t *__restrict__ list) {
    __shared__ uint64_t s_c[kWords][kB];
    const uint32_t tid = threadIdx.x, t = blockIdx.x * kB + tid;
    const uint32_t b = t < n_tiles ? bucket[t] : kAllocStays;
    block_bucket_scan(s_c, tid, b);
    if (b >= (uint32_t) kAllocMaxBuckets) return;      /* kAllocStays */
    list[offsets[(size_t) b * n_blocks + blockIdx.x] + scan_field(s_c, tid, b) - 1u] = t;
}

__global__ __launch_bounds__(kB) void film_alloc_inverse_kernel(const uint32_t *__restrict__ list, uint32_t n, uint32_t n_tiles, uint32_t *__restrict__ inverse) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = list[i];
    if (t < n_tiles) inverse[t] = i;      /* (a list names a tile once) */
}

__global__ __launch_bounds__(kB) void film_alloc_tile_spp_kernel(const uint32_t *__restrict__ level, AllocLevels lv, uint32_t n_tiles, uint32_t *__restrict__ tile_spp) {
    const uint32_t t = blockIdx.x * kB + threadIdx.x;
    if (t < n_tiles) tile_spp[t] = alloc_spp(lv, min(level[t], lv.J));
}

} // namespace

namespace nrt {

#define ALLOC_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(e__); } while (0)

void film_alloc_release(FilmAlloc &a) {
    for (uint32_t *p : {a.level, a.done, a.bucket, a.list, a.counts, a.bucket_begin}) if (p) (void) hipFree(p);
    a = FilmAlloc();
}

std::string film_alloc_reserve(FilmAlloc &a, size_t n_frame_tiles) {
    if (n_frame_tiles == 0 || n_frame_tiles >= (size_t) kTileNotListed) return "allocate: frame of no tiles or too many";
    if (a.capacity >= n_frame_tiles) return std::string();
    film_alloc_release(a);
    const size_t words = n_frame_tiles * sizeof(uint32_t), n_blocks = (n_frame_tiles + kB - 1) / kB;
    for (uint32_t **p : {&a.level, &a.done, &a.bucket, &a.list}) ALLOC_TRY(hipMalloc((void **) p, words));
    ALLOC_TRY(hipMalloc((void **) &a.counts, n_blocks * (size_t) kAllocMaxBuckets * sizeof(uint32_t)));
    ALLOC_TRY(hipMalloc((void **) &a.bucket_begin, (size_t) (kAllocMaxBuckets + 1) * sizeof(uint32_t)));
    a.capacity = n_frame_tiles;
    return std::string();
}

std::string film_alloc_round(FilmAlloc &a, const float *d_tile_err, float target, float headroom, const AllocLevels &lv, size_t n_frame_tiles,
                             uint32_t *bucket_begin, void *stream) {
    hipStream_t s = (hipStream_t) stream;
    if (a.capacity < n_frame_tiles || n_frame_tiles == 0) return "allocate: no levels for this frame";
    if (lv.J > (uint32_t) kAllocMaxLevel) return "allocate: more than eight levels";
    const uint32_t n = (uint32_t) n_frame_tiles, n_blocks = (n + kB - 1) / kB, n_buckets = alloc_n_buckets(lv.J);
    hipLaunchKernelGGL(film_alloc_classify_kernel, dim3(n_blocks), dim3(kB), 0, s, d_tile_err, target, headroom, lv, n, a.level, a.done, a.bucket);
    ALLOC_TRY(hipGetLastError());
    if (n_buckets == 0) {      /* one level: nothing can move */
        for (int b = 0; b <= kAllocMaxBuckets; ++b) bucket_begin[b] = 0;
        ALLOC_TRY(hipStreamSynchronize(s));
        return std::string();
    }
    hipLaunchKernelGGL(film_alloc_count_kernel, dim3(n_blocks), dim3(kB), 0, s, (const uint32_t *) a.bucket, n, n_buckets, n_blocks, a.counts);
    ALLOC_TRY(hipGetLastError());
    hipLaunchKernelGGL(film_alloc_scan_kernel, dim3(1), dim3(kB), 0, s, a.counts, n_buckets * n_blocks, n_blocks, n_buckets, a.bucket_begin);
    ALLOC_TRY(hipGetLastError());
    hipLaunchKernelGGL(film_alloc_scatter_kernel, dim3(n_blocks), dim3(kB), 0, s, (const uint32_t *) a.bucket, n, n_blocks, (const uint32_t *) a.counts, a.list);
    ALLOC_TRY(hipGetLastError());
    ALLOC_TRY(hipMemcpyAsync(bucket_begin, a.bucket_begin, (size_t) (kAllocMaxBuckets + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ALLOC_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < kAllocMaxBuckets; ++b)
        if (bucket_begin[b] > bucket_begin[b + 1] || bucket_begin[b + 1] > n) return "allocate: the grouping's offsets are not a partition";
    return std::string();
}

std::string film_alloc_inverse(const FilmAlloc &a, uint32_t begin, uint32_t n, uint32_t *d_inverse, size_t n_frame_tiles, void *stream) {
    hipStream_t s = (hipStream_t) stream;
    if (a.capacity < n_frame_tiles || (size_t) begin + n > n_frame_tiles) return "allocate: a bucket outside the list";
    ALLOC_TRY(hipMemsetAsync(d_inverse, 0xff, n_frame_tiles * sizeof(uint32_t), s));      /* kTileNotListed */
    if (n == 0) return std::string();
    hipLaunchKernelGGL(film_alloc_inverse_kernel, dim3((n + kB - 1) / kB), dim3(kB), 0, s, (const uint32_t *) a.list + begin, n, (uint32_t) n_frame_tiles, d_inverse);
    ALLOC_TRY(hipGetLastError());
    return std::string();
}

std::string film_alloc_tile_spp(const FilmAlloc &a, const AllocLevels &lv, uint32_t *d_tile_spp, size_t n_frame_tiles, void *stream) {
    if (a.capacity < n_frame_tiles || n_frame_tiles == 0) return "allocate: no levels for this frame";
    const uint32_t n = (uint32_t) n_frame_tiles;
    hipLaunchKernelGGL(film_alloc_tile_spp_kernel, dim3((n + kB - 1) / kB), dim3(kB), 0, (hipStream_t) stream, (const uint32_t *) a.level, lv, n, d_tile_spp);
    ALLOC_TRY(hipGetLastError());
    return std::string();
}

} // namespace nrt
