/* features.hip -- the first-hit feature pass and its store (see features.h). */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "features.h"

using namespace nrt;

namespace {

constexpr int kFeatBlock = 256;
/* Registers: 4 waves per SIMD = 128 VGPRs, the budget of the megakernel; the walk and the texture lookup fit it without
   scratch.  LDS is the stack alone, STACK * 1 KiB per workgroup: 16 / 24 / 32 entries leave 10 / 6 / 5 workgroups per CU
   (160 KiB), at or above the 4 the launch bounds ask for; only the 64-entry stack of deep trees (64 KiB, 2 workgroups) is bound by LDS. */
constexpr int kFeatMinWaves = 4;

/* a column of the workgroup's LDS stack array, [depth][thread]: bank = lane, conflict free (as nori_hip.hip's) */
template <int DEPTH, int STRIDE>
struct LdsStack {
    int *base;      /* &lds[threadIdx.x] */
    int sp;
    __device__ __forceinline__ void reset() { sp = 0; }
    __device__ __forceinline__ void push(int v) {
        if (sp < DEPTH) base[sp * STRIDE] = v;
        sp++;
    }
    __device__ __forceinline__ int pop() {
        sp--;
        return sp < DEPTH ? base[sp * STRIDE] : 0;
    }
    __device__ __forceinline__ int pop_or(int empty_value) { return sp == 0 ? empty_value : pop(); }
};

template <int STACK>
__global__ __launch_bounds__(kFeatBlock, kFeatMinWaves) void feature_pass_kernel(DevScene sc, FeatureLaunch fl, f2 *__restrict__ pos, P3 *__restrict__ albedo,
                                                                                 P3 *__restrict__ normal, P3 *__restrict__ depth, unsigned long long *stats) {
    __shared__ int s_stack[STACK * kFeatBlock];
    const int tid = threadIdx.x;
    const uint32_t sel = blockIdx.x / fl.n_chunks, chunk = blockIdx.x % fl.n_chunks;
    const uint32_t tile_id = fl.tile_rem + sel * fl.tile_mod;
    const int x0 = (int) (tile_id % fl.tiles_x) * kTile, y0 = (int) (tile_id / fl.tiles_x) * kTile;
    /* the chunk's samples RELATIVE to spp_begin, [r0, r1), as render_kernel counts them: spp_begin + spp_count itself may be 2^32
       (the frame of sample 2^32 - 1) */
    const uint32_t r0 = min(chunk * fl.chunk_spp, fl.spp_count);
    const uint32_t r1 = r0 + min(fl.chunk_spp, fl.spp_count - r0);
    int px, py; film_tile_pixel(tid, x0, y0, px, py);
    const bool live = px < sc.camera.width && py < sc.camera.height;

    LdsStack<STACK, kFeatBlock> stack;
    stack.base = s_stack + tid; stack.sp = 0;
    TraversalCounters tc; tc.nodes = tc.tris = 0;
    const uint32_t mask = fl.mask;
    if (live) {
        for (uint32_t r = r0; r < r1; ++r) {
            const uint32_t s = fl.spp_begin + r;
            /* renderBlock, src/main.cpp:41-46: jitter, aperture draw, sampleRay -- the camera sample of render_kernel / first_vertex */
            Rng rng;
            rng_seed(rng, (uint64_t) py * (uint64_t) sc.camera.width + (uint64_t) px, (uint64_t) s);
            const f2 j = rng_next_2d(rng);
            const f2 pixelSample = mk2((float) px + j.x, (float) py + j.y);
            const f2 apertureSample = rng_next_2d(rng);        /* perspective.cpp:78; used by a lens only */
            RayIn ray;
            camera_sample_ray_lens(sc.camera, pixelSample, apertureSample, ray);
            /* the closest-hit query: the device body of the generic traverse<false> (rt_trace.h), statement for statement -- every
               tree form, no LDS image, the same steps in the same order, hence the same hit.  Spelt out because a call of
               traverse() itself leaves its Trav in memory (the compiler widens the loads of tv.o / tv.d before it splits the
               struct): 16 B per lane of scratch or LDS, outside this kernel's budget. */
            Trav tv;
            trav_begin<kLayoutAny>(sc, ray, false, stack, tv);
            while (trav_active(tv)) {
                if (trav_at_inner(tv)) {
                    if (sc.wide) trav_wide_step<false>(sc, stack, tv, tc);
                    else trav_inner_step<false>(sc, stack, tv, tc);
                } else {
                    trav_leaf_step<false>(sc, stack, tv, tc);
                }
            }
            const Hit hit = tv.hit;
            const bool found = hit.tri != kNoHit;
            P3 a, n, d;
            first_hit_features(sc, hit, found, mask, a, n, d);
            const size_t idx = ((size_t) sel * fl.spp_count + (size_t) r) * 256u + (size_t) tid;
            pos[idx] = pixelSample;
            if (mask & kFeatureAlbedo) albedo[idx] = a;
            if (mask & kFeatureNormal) normal[idx] = n;
            if (mask & kFeatureDepth) depth[idx] = d;
        }
    }
    /* one camera sample = one closest-hit ray; counted per wave, no LDS beside the stack */
    const unsigned long long n_lanes = (unsigned long long) __popcll(__ballot(live));
    if ((tid & 63) == 0 && n_lanes != 0ull && r1 > r0) {
        const unsigned long long n = n_lanes * (unsigned long long) (r1 - r0);
        atomicAdd(&stats[0], n); atomicAdd(&stats[1], n);
    }
}

template <int STACK>
hipError_t launch(const DevScene &sc, const FeatureLaunch &fl, const FilmStore &film, const FeatureStore &fs, unsigned long long *d_stats, hipStream_t s) {
    hipLaunchKernelGGL((feature_pass_kernel<STACK>), dim3(fl.n_sel_tiles * fl.n_chunks), dim3(kFeatBlock), 0, s, sc, fl, film.pos,
                       fs.plane[0], fs.plane[1], fs.plane[2], d_stats);
    return hipGetLastError();
}

int stack_entries(uint32_t need) { return need <= 16 ? 16 : need <= 24 ? 24 : need <= 32 ? 32 : 64; }

} // namespace

namespace nrt {

#define FEAT_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(e__); } while (0)

void feature_store_release(FeatureStore &fs) {
    for (int f = 0; f < kFeatureCount; ++f) {
        if (fs.plane[f]) (void) hipFree(fs.plane[f]);
        if (fs.tile_acc[f]) (void) hipFree(fs.tile_acc[f]);
    }
    fs = FeatureStore();
}

std::string feature_store_prepare(FeatureStore &fs, uint32_t mask, const FilmStore &view, size_t n_samples, size_t n_sel_tiles, int tile_w, void *stream) {
    const size_t acc = n_sel_tiles * view.n_parts * (size_t) tile_w * tile_w * 4;      /* film_prepare's */
    for (int f = 0; f < kFeatureCount; ++f) {
        if (!(mask & (1u << f))) continue;
        if (fs.capacity[f] < n_samples || !fs.plane[f]) {
            if (fs.plane[f]) (void) hipFree(fs.plane[f]);
            fs.plane[f] = nullptr; fs.capacity[f] = 0;
            FEAT_TRY(hipMalloc((void **) &fs.plane[f], std::max<size_t>(n_samples, 1) * sizeof(P3)));
            fs.capacity[f] = n_samples;
        }
        if (fs.acc_floats[f] < acc || !fs.tile_acc[f]) {
            if (fs.tile_acc[f]) (void) hipFree(fs.tile_acc[f]);
            fs.tile_acc[f] = nullptr; fs.acc_floats[f] = 0;
            FEAT_TRY(hipMalloc((void **) &fs.tile_acc[f], std::max<size_t>(acc, 4) * sizeof(float)));
            fs.acc_floats[f] = acc;
        }
        FEAT_TRY(hipMemsetAsync(fs.tile_acc[f], 0, std::max<size_t>(acc, 4) * sizeof(float), (hipStream_t) stream));
    }
    return std::string();
}

uint32_t feature_pass_lds_bytes(uint32_t stack_need) { return (uint32_t) (stack_entries(stack_need) * kFeatBlock * sizeof(int)); }

hipError_t feature_pass_launch(const DevScene &sc, const FeatureLaunch &fl, uint32_t stack_need, const FilmStore &film, const FeatureStore &fs,
                               unsigned long long *d_stats, void *stream) {
    if (fl.n_sel_tiles == 0 || fl.spp_count == 0 || fl.n_chunks == 0) return hipSuccess;
    hipStream_t s = (hipStream_t) stream;
    /* the LDS stack is sized to the tree: fewer entries -> more workgroups per CU */
    switch (stack_entries(stack_need)) {
    case 16: return launch<16>(sc, fl, film, fs, d_stats, s);
    case 24: return launch<24>(sc, fl, film, fs, d_stats, s);
    case 32: return launch<32>(sc, fl, film, fs, d_stats, s);
    default: return launch<64>(sc, fl, film, fs, d_stats, s);
    }
}

} // namespace nrt
