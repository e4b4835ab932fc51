/*
 * wf_device.h -- what the kernels of the wavefront engine share: the path-state pool as the device sees it (WfState, WfBuf, WfBatch), the
 * shape of a pass, the per-lane LDS stacks, the streaming loads and stores, the first vertex, and the text of wf_shade / wf_finish
 * (wf_path_kernels.h).  Included by wavefront.hip (wf_extend, the launches, the engine) and by wavefront_env.hip (the instantiations of
 * wf_shade / wf_finish for scenes with an environment map).  Everything here is declared in the unnamed namespace, so each unit has
 * its own copy and a kernel belongs to the unit that instantiates it.  The text is wavefront.hip's of before, moved, not changed.
 */
#pragma once

/* The laboratory -- perturbations of the node step and of wf_shade, the cycle profile of a wave -- lives in wf_experiments.h and is
   compiled only into the variant libraries of tools/build_variant*.sh (-DNORI_LAB); the product build defines every hook empty. */
#ifdef NORI_LAB
#include "wf_experiments.h"
#else
#define NORI_EXP_Q_GLOBAL
#define NORI_EXP_Q_LDS
#define NORI_EXP_Q_ALU
#define NORI_PROF_DECL
#define NORI_PROF_MARK(acc)
#define NORI_PROF_STORE
#define NORI_PROF_REPORT(h)
#define NORI_LAB_SHADE_PAD
#define NORI_LAB_SHADE_VERTEX
#define NORI_LAB_SHADE_STORE
#endif

#include "film.h"
#include "ktimer.h"
#include "shade_tables.h"
#include "rt_path.h"
#include "wavefront.h"
#include "wf_records.h"

using namespace nrt;

namespace {

constexpr int kB = 256;

/* counters: path count and dynamic-chunk head per state copy (index + copy), overflow flag */
enum { C_N = 0, C_HEAD = 2, C_OVERFLOW = 4, C_TAIL_HEAD = 5, C_SAMPLE = 6, C_HEAD_FRESH = 8, C_COUNT = 12 };      /* C_SAMPLE + copy: the batch's next camera sample (regeneration); C_HEAD_FRESH + copy: chunk head of the launch that traces a pass's NEW paths */
enum { S_CAM = 0, S_CLOSEST = 1, S_SHADOW = 2, S_NODES = 3, S_TRIS = 4, S_INVALID = 5, S_COUNT = 8 };
/* census (COUNT builds, NORI_HIP_CENSUS): wave-level trips of wf_extend's loop and the lanes they used */
enum { Z_TRIPS = 0, Z_INNER_TRIPS = 1, Z_INNER_LANES = 2, Z_LEAF_TRIPS = 3, Z_LEAF_LANES = 4, Z_REFILLS = 5, Z_REFILL_LANES = 6, Z_COUNT = 8 };

constexpr uint32_t kShadeChunk = 4096u;     /* output space a wf_shade workgroup reserves per atomic */

/* The state of the paths in flight, one record per path, structure of arrays.  Two copies: wf_shade
   reads copy `cur` at index i and writes the surviving paths COMPACTED into copy `cur ^ 1`, so every
   kernel reads and writes dense, fully coalesced ranges [0, n) however many paths have died. */
struct WfState {      /* wf_records.h: how a record lies in HBM */
    P3 *o;          /* origin of both rays (their mint is kStoredMint) */
    f4 *dA;         /* (d.xyz of the continuation ray -- its maxt is inf --, bits: F_* | prev_measure << 4 | depth << 8; 0 = no path in this slot) */
    f4 *dB;         /* (d.xyz, maxt) shadow ray, same origin */
    f4 *T_eta, *L_pdf;
    P3 *Ld;
    uint32_t *sidx;    /* the path's camera sample: index into the film's sample store */
    unsigned long long *rng;
};

struct WfBuf {
    WfState st[2];
    f4 *hit;           /* (t, u, v, hit word) written by wf_extend for the paths of copy `cur` */
    f2 *samp_pos;
    P3 *samp_L;        /* the film's sample store (film.h) */
    uint32_t *ctr;
    unsigned long long *stats;
    uint32_t capacity; /* records per copy */
    int *stack_spill;  /* [entry beyond the LDS stack][lane of the wf_extend grid] */
    unsigned long long *census;   /* Z_* counters or null */
};

struct WfBatch {
    uint32_t tile_first, n_tiles;       /* range of selected-tile ordinals */
    uint32_t s_first, n_spp;            /* absolute first sample index, samples per pixel in this batch */
    uint32_t tile_mod, tile_rem, tiles_x;
    int32_t tile_w;
    int32_t inner_repeat;               /* wf_extend: node steps repeat while at least this many lanes are at inner nodes (65: never) */
    uint32_t flags;                     /* kBatch* */
    uint32_t pool;                      /* paths a pass works on: the stored survivors + as many NEW camera samples of the batch as fill it up */
    const uint32_t *tile_list = nullptr;    /* a render by list (film_tiles.h): selected-tile ordinal -> tile; null: tile_rem + ordinal * tile_mod */
};

/* Regeneration (constant population).  A pass over state copy `cur` works on the n_s survivors the last wf_shade stored plus
   n_fresh camera samples of the batch that have not been started yet -- path i >= n_f0 IS camera sample s0 + (i - n_f0): nothing of
   it is stored, both kernels compute its first vertex (first_vertex) as the batch's first pass always did.  So a batch of any
   size runs on a pool of bt.pool paths, every pass full until the batch's samples run out; with pool >= the batch's samples the
   first pass starts them all and the schedule is the shrinking one of rounds 2 - 5.  Which pass a sample starts in is not
   observable: its pcg32 stream is seeded by (pixel, sample), its radiance goes to the film store at its own index.
   MODE of a kernel: kStoredOnly it works on the stored paths [0, n_s) and carries no camera code; kFreshOnly on the new paths [n_f0, n) and
   reads no state; kMixed (wf_shade only) on both.  wf_extend exists in the two pure forms only -- one kernel with both refills needs 80 B of scratch
   and runs 17 % slower (profiles/r6_01_pool_sweep.txt, "mixed kernels") --: a pass that holds stored AND new paths is traced by TWO launches, the
   stored paths first, then the new ones, each with its own chunk counter; a batch's first pass has only the second, its passes after the last sample
   only the first. */
enum { kStoredOnly = 0, kFreshOnly = 1, kMixed = 2 };
struct PassShape { uint32_t n_s, s0, n_fresh, n_f0, n; };      /* stored paths [0, n_s), new paths [n_f0, n): n_f0 = n_s rounded up to a wf_shade round */
template <int MODE> __device__ __forceinline__ PassShape pass_shape(const uint32_t *ctr, int cur, const WfBatch &bt) {
    PassShape ps;
    ps.n_s = ctr[C_N + cur];      /* (zero in a batch's first pass: the counters are cleared when it starts) */
    ps.s0 = ctr[C_SAMPLE + cur];
    ps.n_f0 = (ps.n_s + 255u) & ~255u;
    const uint32_t total = bt.n_tiles * 256u * bt.n_spp;
    ps.n_fresh = MODE == kStoredOnly ? 0u : min(total - ps.s0, bt.pool > ps.n_f0 ? bt.pool - ps.n_f0 : 0u);
    ps.n = ps.n_fresh ? ps.n_f0 + ps.n_fresh : ps.n_s;
    return ps;
}
constexpr uint32_t kBatchNoAsmLoop = 1u;       /* wf_extend: the compiler's node loop instead of the hand-written one (A/B, tests) */
constexpr uint32_t kBatchCountQ = 2u;          /* wf_extend, COUNT builds: walk the 32-B node records (trav_inner_step_q, the C++ statement of the
                                                  hand-written loop) -- the node / triangle tests counted are those of the tree form the timed kernel walks */

/* Per-lane traversal stack in LDS ([entry][thread], bank = lane -> conflict free).
   Trees no deeper than DEPTH: one register (the address of the next free slot); entry 0 holds the
   "finished" marker, so popping the empty stack ends the traversal without an emptiness test.
   Deeper trees (SPILL): the first DEPTH entries in LDS, the rest -- rare -- in a per-lane column of
   a global buffer.  A small DEPTH keeps wf_extend at 8 waves/SIMD however deep the tree is (a
   64-entry LDS stack would allow 2), which is what hides the HBM latency of scenes that do not fit
   in L2. */
template <int DEPTH, bool SPILL, int BLOCK = kB>
struct LdsStackW {
    int *base; int sp;
    int *spill; uint32_t spill_stride;      /* wave-uniform base, lanes in flight */
    __device__ __forceinline__ void init(char *smem, int *spill_, uint32_t stride_) {
        base = reinterpret_cast<int *>(smem) + threadIdx.x; sp = 0; spill = spill_; spill_stride = stride_;
    }
    __device__ __forceinline__ void reset() { sp = 0; }
    __device__ __forceinline__ void push(int v) {
        if (sp < DEPTH) base[sp * BLOCK] = v;
        else spill[(size_t) (sp - DEPTH) * spill_stride + blockIdx.x * BLOCK + threadIdx.x] = v;
        sp++;
    }
    __device__ __forceinline__ int pop_or(int empty_value) {
        if (sp == 0) return empty_value;
        sp--;
        if (sp < DEPTH) return base[sp * BLOCK];
        return spill[(size_t) (sp - DEPTH) * spill_stride + blockIdx.x * BLOCK + threadIdx.x];
    }
    static constexpr int kLdsEntries = DEPTH;
};

/* LDS as the hardware addresses it: 32-bit byte addresses, so that the walk's stack pointer is ONE register the hand-written
   node loop below can use as it is */
typedef __attribute__((address_space(3))) int lds_int_t;
__device__ __forceinline__ uint32_t lds_address(const void *generic) {
    return (uint32_t) reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) char *) generic);
}
__device__ __forceinline__ lds_int_t *lds_int_at(uint32_t address) { return reinterpret_cast<lds_int_t *>(address); }

template <int DEPTH, int BLOCK>
struct LdsStackW<DEPTH, false, BLOCK> {
    uint32_t top;         /* LDS address of the next free slot */
    uint32_t wave_base;   /* of slot 0 of the wave's lane 0 (wave-uniform): slot k of thread l lives at (k BLOCK + l) ints, bank = lane */
    __device__ __forceinline__ void init(char *smem, int *, uint32_t) {
        wave_base = (uint32_t) __builtin_amdgcn_readfirstlane((int) (lds_address(smem) + (threadIdx.x & ~63u) * 4u)); top = 0u;
    }
    /* the lane's column is found anew at every reset (two v_mbcnt in a volatile statement): as a value the compiler knows to be
       constant it would live in a register for the whole kernel -- the one it then spills */
    __device__ __forceinline__ void reset() {
        uint32_t lane;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
        const uint32_t base = wave_base + lane * 4u;
        *lds_int_at(base) = kTravDone; top = base + BLOCK * 4u;
    }
    __device__ __forceinline__ void push(int v) { *lds_int_at(top) = v; top += BLOCK * 4u; }
    __device__ __forceinline__ int pop_or(int) { top -= BLOCK * 4u; return *lds_int_at(top); }
    static constexpr int kLdsEntries = DEPTH + 1;
};

/* The stack of the hand-written node loop for trees deeper than DEPTH: the LDS stack above, and what does not fit goes to a
   per-lane column of a global buffer.  The loop itself only knows the LDS part (one register: `top`); a lane whose LDS part
   is full makes it hand the step to the C++ code (wf_extend), which pushes and pops through this class.  The number of
   entries a lane has in the global column is kept in the LDS slot behind its last stack slot -- the slot `top` points at
   exactly when the LDS part is full -- so it costs no register.  Full is a wave-uniform comparison: top >= limit. */
template <int DEPTH, int BLOCK>
struct LdsStackHybrid {
    uint32_t top;
    uint32_t wave_base, limit;      /* wave-uniform: LDS address of slot 0 of lane 0 / of the counter slot of lane 0 */
    int *spill; uint32_t spill_stride;
    __device__ __forceinline__ void init(char *smem, int *spill_, uint32_t stride_) {
        wave_base = (uint32_t) __builtin_amdgcn_readfirstlane((int) (lds_address(smem) + (threadIdx.x & ~63u) * 4u));
        limit = wave_base + (uint32_t) (DEPTH + 1) * BLOCK * 4u; top = 0u; spill = spill_; spill_stride = stride_;
    }
    __device__ __forceinline__ void reset() {
        uint32_t lane;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
        const uint32_t base = wave_base + lane * 4u;
        *lds_int_at(base) = kTravDone; *lds_int_at(base + (uint32_t) (DEPTH + 1) * BLOCK * 4u) = 0; top = base + BLOCK * 4u;
    }
    __device__ __forceinline__ void push(int v) {
        if (top < limit) { *lds_int_at(top) = v; top += BLOCK * 4u; }
        else { const int n = *lds_int_at(top); spill[(size_t) n * spill_stride + blockIdx.x * BLOCK + threadIdx.x] = v; *lds_int_at(top) = n + 1; }
    }
    __device__ __forceinline__ int pop_or(int) {
        if (top >= limit) {
            const int n = *lds_int_at(top);
            if (n > 0) { *lds_int_at(top) = n - 1; return spill[(size_t) (n - 1) * spill_stride + blockIdx.x * BLOCK + threadIdx.x]; }
        }
        top -= BLOCK * 4u; return *lds_int_at(top);
    }
    static constexpr int kLdsEntries = DEPTH + 2;
};
template <int STACK, bool SPILL, bool ASM, int BLOCK> struct ExtendStack { typedef LdsStackW<STACK, SPILL, BLOCK> type; };
template <int STACK, int BLOCK> struct ExtendStack<STACK, true, true, BLOCK> { typedef LdsStackHybrid<STACK, BLOCK> type; };

__device__ __forceinline__ int lane_id() { return (int) (threadIdx.x & 63u); }

/* Streaming accesses to the path state: every record is written once and read once per pass, tens of GB -- nothing of
   it is worth a line of L2 next to the tree.  Nontemporal where it measured faster (A/B on one box, ms per pass):
   level 1 = wf_extend's hit / sample-position stores and wf_shade's read of the hit record (wf_extend 47.9 -> 47.2),
   level 2 = wf_shade's state loads and stores (wf_shade 27.9 -> 27.1).  wf_extend's own state LOADS stay plain: nontemporal
   they cost it 2 ms (the 32 B a path re-reads after its shadow ray then miss). */
constexpr int kNontemporalLevel = 2;
typedef float v4f_t __attribute__((ext_vector_type(4)));
typedef float v2f_t __attribute__((ext_vector_type(2)));
template <int LEVEL> __device__ __forceinline__ void st_f4(f4 *p, const f4 &v) {
    if (kNontemporalLevel >= LEVEL) { v4f_t t = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(t, reinterpret_cast<v4f_t *>(p)); }
    else *p = v;
}
template <int LEVEL> __device__ __forceinline__ void st_f2(f2 *p, const f2 &v) {
    if (kNontemporalLevel >= LEVEL) { v2f_t t = {v.x, v.y}; __builtin_nontemporal_store(t, reinterpret_cast<v2f_t *>(p)); }
    else *p = v;
}
template <int LEVEL> __device__ __forceinline__ f4 ld_f4(const f4 *p) {
    if (kNontemporalLevel >= LEVEL) { const v4f_t t = __builtin_nontemporal_load(reinterpret_cast<const v4f_t *>(p)); f4 r; r.x = t.x; r.y = t.y; r.z = t.z; r.w = t.w; return r; }
    return *p;
}
typedef float v3f_t __attribute__((ext_vector_type(3)));
template <int LEVEL> __device__ __forceinline__ void st_p3(P3 *p, const P3 &v) {      /* 12 B, 4-B aligned: global_store_dwordx3 */
    if (kNontemporalLevel >= LEVEL) { __builtin_nontemporal_store(v.x, &p->x); __builtin_nontemporal_store(v.y, &p->y); __builtin_nontemporal_store(v.z, &p->z); }
    else *p = v;
}
template <int LEVEL> __device__ __forceinline__ P3 ld_p3(const P3 *p) {
    if (kNontemporalLevel >= LEVEL) { P3 r; r.x = __builtin_nontemporal_load(&p->x); r.y = __builtin_nontemporal_load(&p->y); r.z = __builtin_nontemporal_load(&p->z); return r; }
    return *p;
}
template <int LEVEL, class T> __device__ __forceinline__ void st_w(T *p, T v) { if (kNontemporalLevel >= LEVEL) __builtin_nontemporal_store(v, p); else *p = v; }
template <int LEVEL, class T> __device__ __forceinline__ T ld_w(const T *p) { if (kNontemporalLevel >= LEVEL) return __builtin_nontemporal_load(p); return *p; }

/* The hot records of the tree (rt_top.h: the image is built once per acceleration structure) into the workgroup's LDS.
   Returns the link a walk starts with. */
__device__ int top_image_to_lds(const DevScene &sc, f4 *top, const f4 *image, uint32_t quads) {
    if (image == nullptr) {      /* no image: nothing cached, every link is a memory link */
        if (threadIdx.x == 0) { f4 h; h.x = __uint_as_float((uint32_t) sc.root); h.y = h.z = h.w = 0.0f; top[0] = h; }
    } else {
        for (uint32_t q = threadIdx.x; q < quads; q += blockDim.x) top[q] = image[q];
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane((int) __float_as_uint(top[0].x));
}

/* The first vertex of the batch's path p is never stored: its camera sample (renderBlock,
   src/main.cpp:41-46) is recomputed where it is needed -- by the first wf_extend (ray) and the first
   wf_shade (direction, pcg32 state) -- which costs ~100 instructions twice and saves writing and
   re-reading 80 B of state per path.  Returns false for pixels of edge tiles outside the image. */
__device__ __forceinline__ bool first_vertex(const DevScene &sc, const WfBatch &bt, uint32_t p, f2 &ps, RayIn &cam, Rng &rng) {
    const uint32_t per_tile = 256u * bt.n_spp;
    const uint32_t tsel = p / per_tile, rem = p - tsel * per_tile;
    const uint32_t sl = rem >> 8, pix = rem & 255u;
    const uint32_t tile_id = bt.tile_list ? bt.tile_list[bt.tile_first + tsel] : bt.tile_rem + (bt.tile_first + tsel) * bt.tile_mod;
    const int x0 = (int) (tile_id % bt.tiles_x) * kTile, y0 = (int) (tile_id / bt.tiles_x) * kTile;
    int px, py; film_tile_pixel((int) pix, x0, y0, px, py);
    if (px >= sc.camera.width || py >= sc.camera.height) return false;
    rng_seed(rng, (uint64_t) py * (uint64_t) sc.camera.width + (uint64_t) px, (uint64_t) (bt.s_first + sl));
    const f2 j = rng_next_2d(rng);
    ps = mk2((float) px + j.x, (float) py + j.y);
    const f2 ap = rng_next_2d(rng);   /* apertureSample: used by a lens only */
    camera_sample_ray_lens(sc.camera, ps, ap, cam);
    return true;
}

/* Integrator::Li, one vertex: consume the shadow result, shade the closest hit, write the surviving
   path -- with its next shadow / continuation rays -- compacted into the other state copy.
   A workgroup owns a contiguous range of rounds (256 paths each) and reserves output space in
   chunks of <= kShadeChunk records with one atomic per chunk, sized by the survival rate it sees;
   what it leaves unused of its last chunk is marked empty (flags = 0) and dropped by the next pass. */
constexpr int kSB = 256;      /* threads per wf_shade workgroup (128 / 64: slower, DESIGN_HISTORY.md) */
static_assert(kSB == 256, "pass_shape starts the new paths of a pass at a multiple of 256");

/* wf_shade's workgroup barriers wait for LDS only: what the compaction exchanges lives there.  (__syncthreads() is also a fence,
   i.e. s_waitcnt vmcnt(0): a wave then sits out the trip of its own state STORES to L2 in every round.) */
__device__ __forceinline__ void shade_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

/* LDSTAB: the scene's small tables fit LDS (shade_tables.h) -- else they are read from global memory (SceneTables) */
template <bool LDSTAB> struct ShadeTab { typedef SceneTables type; static __device__ __forceinline__ type make(const DevScene &sc, uint4 *) { type t = {&sc}; return t; } };
template <> struct ShadeTab<true> { typedef LdsTables type; static __device__ __forceinline__ type make(const DevScene &sc, uint4 *s_tab) { return shade_tables_copy(sc, s_tab); } };

/* Software pipelining across rounds: the head of the next round's record (continuation direction with the flags, sample index,
   radiance, hit) is requested while this round computes, so that a round starts with its first dependent loads already answered
   (round 3: wf_shade 27.1 -> 26.0 ms; round 5, all-diffuse kernel: 23.7 -> 23.1).  Going further does not pay -- the WHOLE record
   of the next round sent straight into LDS with every gather of the vertex issued at the top of the round: bit-identical and
   0.5 - 1 ms slower (profiles/r4_02_shade_pipeline_ab.txt). */

/* MATSET (rt_path.h): the BSDF types the scene contains -- the kernel of an all-diffuse scene carries no mirror, dielectric or
   microfacet code (the all-diffuse kernel: 117 registers instead of 128; held to the 96 of five workgroups per CU it spills and is
   slower, profiles/r5_01_shade_matset_ab.txt) */
#ifndef NORI_SHADE_WGS
#define NORI_SHADE_WGS 4      /* workgroups per SIMD wf_shade is compiled for (variant builds: 5, 6) */
#endif
/* COMPACT: the compact record of all-diffuse scenes (wf_records.h).  How much of it the kernels use is a build constant, so that each
   step can be measured alone (variant builds): 1 = the pcg32 state is derived, 2 = and no eta: (T, pdf_mat) quad, 12-B L, 3 = and Lsum
   in the place of Ld.  The steps are cumulative. */
#ifndef NORI_WF_COMPACT_LEVEL
#define NORI_WF_COMPACT_LEVEL 3
#endif
static_assert(NORI_WF_COMPACT_LEVEL >= 1 && NORI_WF_COMPACT_LEVEL <= 3, "NORI_WF_COMPACT_LEVEL: 1, 2 or 3");
/* (A_n, G_n) of rng_skip_pair for the draw counts of depths below this, in LDS, filled once per workgroup.  The headline's batches
   reach wf_finish after twelve passes, so wf_shade sees depths up to ~12 there; 32 entries are 512 B, which leaves the workgroups per
   CU as they are.  A deeper path (and every path wf_finish takes) runs rng_skip_pair's loop itself. */
constexpr uint32_t kSkipDepths = 32u;
typedef __attribute__((address_space(3))) const unsigned long long *lds_u64_t;
template <int INTEG> __device__ __forceinline__ void skip_table_fill(unsigned long long *s_skip) {
    if (threadIdx.x < kSkipDepths) {
        const RngSkip k = rng_skip_pair(path_draws_diffuse<INTEG>(threadIdx.x));
        s_skip[2u * threadIdx.x] = k.A; s_skip[2u * threadIdx.x + 1u] = k.G;
    }
    __syncthreads();
}
/* The pcg32 state of the stored path of camera sample `sidx` at `depth` (compact record): the sample index is split as first_vertex
   splits it -- tile ordinal, sample in the pixel, pixel in the tile -- which gives the stream's seed; the depth gives the draws.
   s_skip: the workgroup's table, or null (the loop for every depth). */
template <int INTEG> __device__ __forceinline__ uint64_t derived_rng_state(const DevScene &sc, const WfBatch &bt, uint32_t sidx, uint32_t depth, const unsigned long long *s_skip) {
    const uint32_t per_tile = 256u * bt.n_spp;
    const uint32_t tsel = sidx / per_tile, rem = sidx - tsel * per_tile;
    const uint32_t sl = rem >> 8, pix = rem & 255u;
    const uint32_t tile_id = bt.tile_list ? bt.tile_list[bt.tile_first + tsel] : bt.tile_rem + (bt.tile_first + tsel) * bt.tile_mod;
    const int x0 = (int) (tile_id % bt.tiles_x) * kTile, y0 = (int) (tile_id / bt.tiles_x) * kTile;
    int px, py; film_tile_pixel((int) pix, x0, y0, px, py);
    RngSkip k;
    if (s_skip != nullptr && depth < kSkipDepths) {
        const lds_u64_t t = (lds_u64_t) s_skip;
        k.A = t[2u * depth]; k.G = t[2u * depth + 1u];
    } else k = rng_skip_pair(path_draws_diffuse<INTEG>(depth));
    return rng_state_derived((uint64_t) py * (uint64_t) sc.camera.width + (uint64_t) px, ((uint64_t) (bt.s_first + sl) << 1u) | 1u, k.A, k.G);
}
/* wf_shade<INTEG, MODE, LDSTAB, MATSET> and wf_finish<INTEG, MATSET> (the full record), wf_shade_compact and wf_finish_compact (the
   compact one): the text of wf_path_kernels.h, twice. */
#define NORI_WF_SHADE_KERNEL wf_shade
#define NORI_WF_FINISH_KERNEL wf_finish
#define NORI_WF_KERNELS_COMPACT false
#include "wf_path_kernels.h"
#undef NORI_WF_SHADE_KERNEL
#undef NORI_WF_FINISH_KERNEL
#undef NORI_WF_KERNELS_COMPACT
#define NORI_WF_SHADE_KERNEL wf_shade_compact
#define NORI_WF_FINISH_KERNEL wf_finish_compact
#define NORI_WF_KERNELS_COMPACT true
#include "wf_path_kernels.h"
#undef NORI_WF_SHADE_KERNEL
#undef NORI_WF_FINISH_KERNEL
#undef NORI_WF_KERNELS_COMPACT

} // namespace
