/*
 * wavefront_first.hip -- the first pass of a batch for a pinhole camera on a BVH2 tree: camera rays against per-tile lists of
 * candidate pair records (first_lists.h) instead of a walk of the tree per ray.
 *
 *   wf_first_build      one lane per tile of the frame: the tile's pyramid, then the walk that collects its list (<= K pairs) or
 *                       marks the tile overflow.  Once per (tree, camera, frame geometry); the context keeps the lists.
 *   wf_first_extend<false>  the launch that replaces wf_extend<..., kFreshOnly, ...>: same samples (pass_shape<kFreshOnly>), same
 *                       first_vertex, same sample positions, hit records, counters and counter hand-over.  A workgroup takes the
 *                       256 consecutive sample indices of one sample round of one tile, so list base and count are uniform: the
 *                       pair records arrive by scalar loads, every lane runs the shared pair test with the walk's tie rule.  No
 *                       stack, no LDS, no refill.  Tiles without a list are left to ...
 *   wf_first_extend<true>  ... this instantiation, launched behind it: the same rounds, only the overflow tiles, every ray through the generic
 *                       traverse<> (rt_trace.h) as wf_finish walks -- its registers and LDS stack stay out of the list kernel.
 * The kernels live in this unit so that wavefront.hip's kernel set stays what it was (its names and resources are pinned by tests).
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "wf_device.h"
#include "first_lists.h"

namespace {

struct FirstTable {      /* as the kernels see the context's lists */
    const uint32_t *pairs;      /* [tile][K] */
    const uint32_t *count;      /* [tile]: pairs in the list, or kFirstListOverflow */
    uint32_t K;
};

__global__ __launch_bounds__(64) void wf_first_build(DevScene sc, uint32_t tiles_x, uint32_t n_tiles, uint32_t K, uint32_t *pairs, uint32_t *count) {
    const uint32_t tile = blockIdx.x * 64u + threadIdx.x;
    if (tile >= n_tiles) return;
    FirstCamera C; first_camera(sc, C);
    FirstFrustum F; first_tile_frustum(sc.camera, C, (int) (tile % tiles_x) * kTile, (int) (tile / tiles_x) * kTile, 1.0, F);
    uint32_t local[kFirstListMaxK];
    const uint32_t n = first_tile_walk(sc, C, F, 1.0, K, local);
    count[tile] = n;
    if (n != kFirstListOverflow) for (uint32_t k = 0; k < n; ++k) pairs[(size_t) tile * K + k] = local[k];
}

/* The lists and the pair records are read through the constant address space: nothing writes them while a render runs, and a load the
   compiler knows to be invariant at a uniform address is a scalar load -- the record arrives in SGPRs, no vector register holds it. */
typedef float cv4_t __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) cv4_t *ConstQuads;
typedef const __attribute__((address_space(4))) uint32_t *ConstWords;
__device__ __forceinline__ f4 const_quad(ConstQuads p) { const cv4_t v = *p; f4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; return r; }

/* the tile of sample round g (256 consecutive sample indices) of the batch: first_vertex's arithmetic, uniform over the workgroup */
__device__ __forceinline__ uint32_t round_tile(const WfBatch &bt, uint32_t g) {
    const uint32_t tsel = g / bt.n_spp;
    return bt.tile_list ? bt.tile_list[bt.tile_first + tsel] : bt.tile_rem + (bt.tile_first + tsel) * bt.tile_mod;
}

/* OVERFLOW = false: the rounds of tiles with a list; true: the others.  Sample s0 + k is path n_f0 + k (pass_shape); rounds are
   aligned to multiples of 256 sample indices, so a round lies in one tile whatever s0 is. */
template <bool OVERFLOW>
__global__ __launch_bounds__(kB, OVERFLOW ? 4 : 8) void wf_first_extend(DevScene sc_, WfBuf b, int cur, WfBatch bt, FirstTable tab, int hand_over) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    /* this launch is made for pinholes only: with the radius a constant the lens arithmetic of first_vertex is dead code */
    DevScene sc = sc_; sc.camera.lens_radius = 0.0f;
    const PassShape shape = pass_shape<kFreshOnly>(b.ctr, cur, bt);
    if (hand_over && blockIdx.x == 0 && threadIdx.x == 0) {      /* wf_extend's hand-over of the counters (wavefront.hip) */
        b.ctr[C_N + (cur ^ 1)] = 0u; b.ctr[C_HEAD + (cur ^ 1)] = 0u; b.ctr[C_HEAD_FRESH + (cur ^ 1)] = 0u;
        b.ctr[C_SAMPLE + (cur ^ 1)] = shape.s0 + shape.n_fresh;
    }
    uint32_t nCam = 0;      /* uniform: counted from ballots; every camera ray is a closest-hit query */
    LdsStackW<16, true> stack;
    if (OVERFLOW) stack.init(smem, b.stack_spill, gridDim.x * kB);
    if (shape.n_fresh != 0u) {
        const uint32_t s_end = shape.s0 + shape.n_fresh;
        const uint32_t g0 = shape.s0 >> 8, g1 = (s_end >> 8) + ((s_end & 255u) != 0u ? 1u : 0u);      /* (no wrap for an end within 255 of 2^32) */
        /* A workgroup takes the rounds g0 + blockIdx.x + k gridDim.x.  Which of them are this kernel's is found 64 at a time -- lane l
           of every wave looks at round k = 64 j + l -- so that a run of rounds of the other kernel costs one trip to memory, not one each. */
        const uint32_t lane = (uint32_t) lane_id();
        for (uint32_t gb = g0 + blockIdx.x; gb < g1; gb += 64u * gridDim.x) {
            const uint32_t gl = gb + lane * gridDim.x;
            const bool mine = gl < g1 && gl >= gb && ((tab.count[round_tile(bt, gl)] == kFirstListOverflow) == OVERFLOW);
            unsigned long long todo = __ballot(mine);
            while (todo != 0ull) {
                const uint32_t j = (uint32_t) __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const uint32_t g = gb + j * gridDim.x;
                const uint32_t tile = (uint32_t) __builtin_amdgcn_readfirstlane((int) round_tile(bt, g));
                const uint32_t sid = (g << 8) + threadIdx.x;
                f2 ps; RayIn ray; Rng rng;
                const bool valid = sid >= shape.s0 && sid < s_end && first_vertex(sc, bt, sid, ps, ray, rng);
                nCam += (uint32_t) __popcll(__ballot(valid));
                if (valid) {
                    st_f2<1>(&b.samp_pos[sid], ps);
                    Hit hit;
                    if (OVERFLOW) {
                        TraversalCounters tc; tc.nodes = 0; tc.tris = 0;
                        traverse<false>(sc, ray, false, stack, hit, tc);
                    } else {
                        hit.tri = kNoHit; hit.mesh = kNoHit; hit.t = ray.maxt; hit.u = 0.0f; hit.v = 0.0f;
                        const uint32_t cnt = (uint32_t) __builtin_amdgcn_readfirstlane((int) tab.count[tile]);
                        const ConstWords list = (ConstWords) (tab.pairs + (size_t) tile * tab.K);
                        for (uint32_t k = 0; k < cnt; ++k) {
                            const ConstQuads tq = (ConstQuads) (sc.tris + (size_t) list[k] * kPairQuads);
                            first_pair_step(const_quad(tq), const_quad(tq + 1), const_quad(tq + 2), const_quad(tq + 3), const_quad(tq + 4), ray.o, ray.d, ray.mint, hit);
                        }
                    }
                    st_f4<1>(&b.hit[shape.n_f0 + (sid - shape.s0)], hit_pack(&hit, false));
                }
            }
        }
    }
    /* the ray counters: one atomic per workgroup and counter, as wf_extend adds them */
    __shared__ uint32_t s_sum;
    __syncthreads();
    if (threadIdx.x == 0) s_sum = 0u;
    __syncthreads();
    if (lane_id() == 0 && nCam) atomicAdd(&s_sum, nCam);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) {
        atomicAdd(&b.stats[S_CLOSEST], (unsigned long long) s_sum);
        atomicAdd(&b.stats[S_CAM], (unsigned long long) s_sum);
    }
}

} // namespace

namespace nrt {

struct WfFirstLists {
    uint32_t *d_pairs = nullptr, *d_count = nullptr;
    size_t pairs_cap = 0, count_cap = 0;
    bool valid = false;
    /* what the lists were built for */
    CameraRec camera; const void *nodes = nullptr, *tris = nullptr; int32_t root = 0; uint32_t n_triangles = 0;
    uint32_t tiles_x = 0, tiles_y = 0, K = 0; int32_t tile_w = 0, border = 0;
    uint32_t list_tiles = 0, overflow_tiles = 0;
    std::vector<uint32_t> h_count;      /* tile_count on the host: which tiles of a call's selection overflow */
    float build_ms = 0.0f;
};

/* the switches, read once per process */
static int first_env_on() { static const int v = [] { const char *e = getenv("NORI_HIP_WF_FIRST"); return e ? atoi(e) : 1; }(); return v; }
static uint32_t first_env_k() {
    static const uint32_t v = [] { const char *e = getenv("NORI_HIP_WF_FIRST_K"); return e ? (uint32_t) std::min<long>((long) kFirstListMaxK, std::max<long>(0, atol(e))) : kFirstListDefaultK; }();
    return v;
}
static int first_env_rebuild() { static const int v = [] { const char *e = getenv("NORI_HIP_WF_FIRST_REBUILD"); return e ? atoi(e) : 0; }(); return v; }

WfFirstLists *wf_first_create() { return new WfFirstLists(); }
void wf_first_destroy(WfFirstLists *f) {
    if (!f) return;
    if (f->d_pairs) (void) hipFree(f->d_pairs);
    if (f->d_count) (void) hipFree(f->d_count);
    delete f;
}
void wf_first_invalidate(WfFirstLists *f) { if (f) f->valid = false; }

bool wf_first_forced() { return first_env_on() >= 2; }
bool wf_first_applies(const DevScene &sc, bool count_traversal) {
    return first_env_on() != 0 && !(sc.camera.lens_radius > 0.0f) && !sc.wide && !count_traversal && sc.n_triangles != 0u && sc.root >= 0;
}

#define WFF_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(e__); } while (0)

std::string wf_first_prepare(WfFirstLists &f, const DevScene &sc, uint32_t tiles_x, uint32_t tiles_y, int32_t tile_w, void *stream, WfFirstInfo &info) {
    hipStream_t s = (hipStream_t) stream;
    const uint32_t K = first_env_k(), n_tiles = tiles_x * tiles_y;
    const bool same = f.valid && memcmp(&f.camera, &sc.camera, sizeof(CameraRec)) == 0 && f.nodes == sc.nodes && f.tris == sc.tris && f.root == sc.root &&
                      f.n_triangles == sc.n_triangles && f.tiles_x == tiles_x && f.tiles_y == tiles_y && f.K == K && f.tile_w == tile_w && f.border == sc.filter.border;
    info.rebuilt = false;
    if (!same || first_env_rebuild() != 0) {
        f.valid = false;
        const size_t need_pairs = (size_t) n_tiles * std::max(1u, K);
        if (f.pairs_cap < need_pairs) {
            if (f.d_pairs) (void) hipFree(f.d_pairs);
            f.d_pairs = nullptr; f.pairs_cap = 0;
            WFF_TRY(hipMalloc((void **) &f.d_pairs, need_pairs * sizeof(uint32_t)));
            f.pairs_cap = need_pairs;
        }
        if (f.count_cap < n_tiles) {
            if (f.d_count) (void) hipFree(f.d_count);
            f.d_count = nullptr; f.count_cap = 0;
            WFF_TRY(hipMalloc((void **) &f.d_count, (size_t) n_tiles * sizeof(uint32_t)));
            f.count_cap = n_tiles;
        }
        /* A build costs two events and a wait for the stream (the overflow counts decide which kernel runs): about 0.25 ms of a call,
           once per camera and tree.  A camera that moves every call pays it every call -- also where the frame then keeps the old
           kernel, since that is known only from the counts. */
        hipEvent_t e0 = nullptr, e1 = nullptr;
        WFF_TRY(hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) { (void) hipEventDestroy(e0); return "wf_first: hipEventCreate"; }
        (void) hipEventRecord(e0, s);
        hipLaunchKernelGGL(wf_first_build, dim3((n_tiles + 63u) / 64u), dim3(64), 0, s, sc, tiles_x, n_tiles, K, f.d_pairs, f.d_count);
        (void) hipEventRecord(e1, s);
        std::vector<uint32_t> &h = f.h_count;
        h.assign(n_tiles, 0u);
        hipError_t rc = hipMemcpyAsync(h.data(), f.d_count, (size_t) n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (rc == hipSuccess) rc = hipStreamSynchronize(s);
        float ms = 0.0f;
        if (rc == hipSuccess) (void) hipEventElapsedTime(&ms, e0, e1);
        (void) hipEventDestroy(e0); (void) hipEventDestroy(e1);
        if (rc != hipSuccess) return std::string("wf_first_build: ") + hipGetErrorString(rc);
        f.list_tiles = f.overflow_tiles = 0;
        for (uint32_t c : h) { if (c == kFirstListOverflow) f.overflow_tiles++; else f.list_tiles++; }
        f.build_ms = ms;
        f.camera = sc.camera; f.nodes = sc.nodes; f.tris = sc.tris; f.root = sc.root; f.n_triangles = sc.n_triangles;
        f.tiles_x = tiles_x; f.tiles_y = tiles_y; f.K = K; f.tile_w = tile_w; f.border = sc.filter.border;
        f.valid = true;
        info.rebuilt = true;
    }
    info.K = K; info.list_tiles = f.list_tiles; info.overflow_tiles = f.overflow_tiles; info.build_ms = f.build_ms;
    return std::string();
}

/* list / overflow tiles among the tiles a call selects: the progression tile_rem + k tile_mod, k < n_sel.  (A render by tile list
   keeps its list in device memory: it is judged by the whole frame's counts.) */
void wf_first_selected(const WfFirstLists &f, uint32_t tile_mod, uint32_t tile_rem, uint32_t n_sel, bool by_list, uint32_t &list_tiles, uint32_t &overflow_tiles) {
    list_tiles = f.list_tiles; overflow_tiles = f.overflow_tiles;
    if (by_list || !f.valid || f.h_count.empty()) return;
    list_tiles = overflow_tiles = 0;
    for (uint32_t k = 0; k < n_sel; ++k) {
        const size_t tile = (size_t) tile_rem + (size_t) k * tile_mod;
        if (tile >= f.h_count.size()) break;
        if (f.h_count[tile] == kFirstListOverflow) overflow_tiles++; else list_tiles++;
    }
}

/* nori_hip_debug_first_lists: wf_first_build over the frame's tiles into buffers of this call's own, copied out.  Neither the
   engine's lists nor the switches above are looked at. */
std::string wf_first_debug_lists(const DevScene &sc, uint32_t K, uint32_t *count, uint32_t *pairs) {
    if (K > kFirstListMaxK) return "K = " + std::to_string(K) + " is more than a list may hold (" + std::to_string(kFirstListMaxK) + ")";
    if (sc.camera.width <= 0 || sc.camera.height <= 0) return "the camera has no pixels";
    const uint32_t tiles_x = (uint32_t) (sc.camera.width + kTile - 1) / kTile, tiles_y = (uint32_t) (sc.camera.height + kTile - 1) / kTile;
    const uint32_t n_tiles = tiles_x * tiles_y;
    const size_t pair_bytes = (size_t) n_tiles * std::max(1u, K) * sizeof(uint32_t), count_bytes = (size_t) n_tiles * sizeof(uint32_t);
    uint32_t *d_pairs = nullptr, *d_count = nullptr;
    hipError_t rc = hipMalloc((void **) &d_pairs, pair_bytes);
    if (rc == hipSuccess) rc = hipMalloc((void **) &d_count, count_bytes);
    if (rc == hipSuccess) rc = hipMemset(d_pairs, 0, pair_bytes);      /* (slots past a tile's count read as 0) */
    if (rc == hipSuccess) rc = hipMemset(d_count, 0, count_bytes);
    if (rc == hipSuccess) {
        hipLaunchKernelGGL(wf_first_build, dim3((n_tiles + 63u) / 64u), dim3(64), 0, (hipStream_t) nullptr, sc, tiles_x, n_tiles, K, d_pairs, d_count);
        rc = hipGetLastError();
    }
    if (rc == hipSuccess) rc = hipMemcpy(count, d_count, count_bytes, hipMemcpyDeviceToHost);
    if (rc == hipSuccess) rc = hipMemcpy(pairs, d_pairs, pair_bytes, hipMemcpyDeviceToHost);
    if (d_pairs) (void) hipFree(d_pairs);
    if (d_count) (void) hipFree(d_count);
    return rc == hipSuccess ? std::string() : std::string("wf_first_build: ") + hipGetErrorString(rc);
}

void wf_first_launch_extend(const WfFirstLists &f, const DevScene &sc, const void *wf_buf, int cur, const void *batch, int grid, void *stream) {
    hipStream_t s = (hipStream_t) stream;
    const WfBuf &b = *static_cast<const WfBuf *>(wf_buf);
    const WfBatch &bt = *static_cast<const WfBatch *>(batch);
    FirstTable tab; tab.pairs = f.d_pairs; tab.count = f.d_count; tab.K = std::max(1u, f.K);
    /* the list tiles first; the overflow tiles behind them on the same stream (the first launch makes the counter hand-over) */
    if (f.list_tiles != 0u) hipLaunchKernelGGL((wf_first_extend<false>), dim3(grid), dim3(kB), 0, s, sc, b, cur, bt, tab, 1);
    if (f.overflow_tiles != 0u || f.list_tiles == 0u) {
        const size_t lds = (size_t) LdsStackW<16, true>::kLdsEntries * kB * sizeof(int);
        hipLaunchKernelGGL((wf_first_extend<true>), dim3(grid), dim3(kB), lds, s, sc, b, cur, bt, tab, f.list_tiles == 0u ? 1 : 0);
    }
}

} // namespace nrt
